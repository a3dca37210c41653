"""The launches of engine.EncoderStack, traced on the host (tools/stack_trace.py), against tests/golden/stack_schedule.json:
per case the names of the calls in order and the sha256 of the full lines (operands by buffer name, shape, dtype and offset,
dropout descriptors, keyword names, reducer ranges).  The golden file was written by `tools/stack_trace.py --write` at the
commit before the forward / backward schedules of the two operand kinds became one; a change that keeps the stack's launches,
their order and their arguments keeps every digest."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stack_trace  # noqa: E402

with open(stack_trace.GOLDEN) as _f:
    GOLDEN = json.load(_f)


def test_golden_holds_exactly_the_cases_of_the_tool():
    assert list(GOLDEN) == list(stack_trace.CASES)
    assert os.path.getsize(stack_trace.GOLDEN) < 20 * 1024


@pytest.mark.parametrize("case", list(stack_trace.CASES))
def test_stack_launches_match_the_recorded_schedule(case):
    from vitssl_hip import engine
    ops, kind = engine.ops, engine.linear_operands()
    calls, digest = stack_trace.summary(stack_trace.trace(case))
    assert engine.ops is ops and engine.linear_operands() == kind      # the recorder is gone again
    want = GOLDEN[case]
    assert calls == want["calls"]
    assert digest == want["sha256"], f"{case}: same calls, other arguments (python tools/stack_trace.py --dump prints the lines)"
