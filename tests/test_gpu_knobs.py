"""Every environment knob of the HIP library that selects another kernel or schedule (README, "Developer A/B knobs") is reachable
by a user through the environment, so it gets the same op-parity cases as the default path: the NT-GEMM / TN-GEMM tests of
tests/test_gpu_ops.py and tests/test_gpu_round3.py with their bit-exact integer cases of tests/test_gpu_gemm_exact.py, and the
attention tests of tests/test_gpu_ops.py, tests/test_gpu_fp8.py and tests/test_gpu_schedules.py, run again with the knob set.  One fresh child process per knob: the library reads
a knob once and caches it (csrc/common.h VsEnvInt)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NT = "test_gemm_nt_epilogues or test_nt_line_shaped_epilogue or test_gemm_nt_embed_epilogue or test_nt_exact"
TN = "test_gemm_tn or test_tn_exact"
ATTN = "test_attention or test_attn_"

KNOBS = [
    ({"VITSSL_NT_STAGGER": "0", "VITSSL_NT_PERSIST": "1"}, NT),   # no start-up stagger; persistent two-phase loop for every K
    ({"VITSSL_NT_TILE": "3", "VITSSL_NT_GROUPN": "2"}, NT),       # 192-row tiles everywhere, raster groups of two tile columns
    ({"VITSSL_NT_TILE": "4"}, NT),                                # 224-row tiles everywhere (uneven DMA split, ragged last tile)
    ({"VITSSL_TN_BATCH_REM": "0", "VITSSL_TN_BATCH_SPLITS": "3"}, TN),   # batched weight gradients: no helper workgroups, forced split count
    ({"VITSSL_ATTN_STAGGER_FWD": "2000", "VITSSL_ATTN_STAGGER_BWD": "0"}, ATTN),   # start-up stagger in the fused forward, none in the backward
]


@pytest.mark.parametrize("env,select", KNOBS, ids=[" ".join(f"{k}={v}" for k, v in e.items()) for e, _ in KNOBS])
def test_op_parity_holds_under_knob(env, select):
    cmd = [sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_ops.py"), os.path.join(ROOT, "tests", "test_gpu_round3.py"),
           os.path.join(ROOT, "tests", "test_gpu_fp8.py"), os.path.join(ROOT, "tests", "test_gpu_schedules.py"),
           os.path.join(ROOT, "tests", "test_gpu_gemm_exact.py"), "-x", "-q", "-m", "gpu", "-k", select, "-p", "no:cacheprovider"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **env), timeout=900, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    assert " passed" in r.stdout and "no tests ran" not in r.stdout, tail
