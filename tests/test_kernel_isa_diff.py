"""tools/kernel_isa_diff.py: the splitter, the normaliser and the comparison on two short hand-written assembly snippets (no
compiler runs)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_isa_diff", os.path.join(ROOT, "tools", "kernel_isa_diff.py"))
kid = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kid)

PARENT = """\
	.text
	.globl	helper
helper:                                 ; a device function: no kernel descriptor, not a kernel
	s_setpc_b64 s[30:31]
.Lfunc_end0:
	.section	.text.k_one,"axG",@progbits,k_one,comdat
	.globl	k_one
	.p2align	8
	.type	k_one,@function
k_one:                                  ; @k_one
	.cfi_startproc
; %bb.0:
	.file	1 "x.hip"
	.loc	1 12 3 prologue_end
	s_load_dwordx2 s[0:1], s[4:5], 0x0   ; a comment
	v_mov_b32_e32 v1, 0
	s_cbranch_scc1 .LBB1_2
.LBB1_2:
	v_add_u32_e32 v0, v0, v1
	s_endpgm
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel k_one
		.amdhsa_next_free_vgpr 2
	.end_amdhsa_kernel
	.section	.text.k_one,"axG",@progbits,k_one,comdat
.Lfunc_end1:
	.size	k_one, .Lfunc_end1-k_one
	.section	.AMDGPU.csdata,"",@progbits
; Kernel info:
; NumVgprs: 2
; Occupancy: 8
	.section	.text.k_two,"axG",@progbits,k_two,comdat
k_two:
	v_mov_b32_e32 v0, 1
	v_mov_b32_e32 v1, 2
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel k_two
	.end_amdhsa_kernel
.Lfunc_end2:
; Occupancy: 4
	.amdgpu_metadata
---
amdhsa.kernels:
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
    .group_segment_fixed_size: 0
    .kernarg_segment_size: 8
    .name:           k_one
    .private_segment_fixed_size: 16
    .sgpr_count:     10
    .sgpr_spill_count: 3
    .symbol:         k_one.kd
    .vgpr_count:     2
    .vgpr_spill_count: 1
  - .agpr_count:     4
    .group_segment_fixed_size: 1024
    .kernarg_segment_size: 0
    .name:           k_two
    .private_segment_fixed_size: 0
    .sgpr_count:     6
    .sgpr_spill_count: 0
    .vgpr_count:     2
    .vgpr_spill_count: 0
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
...
	.end_amdgpu_metadata
"""

# k_one: another function ordinal, other comments and debug lines, the same code.  k_two: its two moves swapped.
BRANCH = (PARENT.replace(".LBB1_2", ".LBB7_2").replace("; a comment", "; another comment").replace(".loc\t1 12 3", ".loc\t1 40 9")
          .replace("\tv_mov_b32_e32 v0, 1\n\tv_mov_b32_e32 v1, 2\n", "\tv_mov_b32_e32 v1, 2\n\tv_mov_b32_e32 v0, 1\n"))


def test_split_finds_kernels_and_stops_at_the_descriptor():
    k = kid.split_kernels(PARENT)
    assert sorted(k) == ["k_one", "k_two"]                 # `helper` has no kernel descriptor
    assert not any("amdhsa" in line or "Lfunc_end" in line for body in k.values() for line in body)
    assert [s.strip() for s in k["k_two"]] == ["v_mov_b32_e32 v0, 1", "v_mov_b32_e32 v1, 2", "s_endpgm"]


def test_normalise_drops_comments_debug_lines_and_label_ordinals():
    n = kid.normalise(kid.split_kernels(PARENT)["k_one"])
    assert n == ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "v_mov_b32_e32 v1, 0", "s_cbranch_scc1 .LBB_2", ".LBB_2:",
                 "v_add_u32_e32 v0, v0, v1", "s_endpgm"]
    assert kid.instructions(n) == [s for s in n if s != ".LBB_2:"]


def test_compare_identical_reordered_and_changed():
    p = {k: kid.normalise(v) for k, v in kid.split_kernels(PARENT).items()}
    b = {k: kid.normalise(v) for k, v in kid.split_kernels(BRANCH).items()}
    assert kid.compare(p["k_one"], b["k_one"]) == (0, True)
    differing, same_sorted = kid.compare(p["k_two"], b["k_two"])
    assert differing > 0 and same_sorted
    changed = [s.replace("v1, 2", "v1, 3") for s in p["k_two"]]
    differing, same_sorted = kid.compare(p["k_two"], changed)
    assert differing == 1 and not same_sorted


def test_metadata_columns():
    m = kid.metadata(PARENT)
    assert m["k_one"] == dict(VGPR=2, AGPR=0, SGPR=10, scratch=16, vspill=1, sspill=3, LDS=0, kernarg=8, occ=8)
    assert m["k_two"] == dict(VGPR=2, AGPR=4, SGPR=6, scratch=0, vspill=0, sspill=0, LDS=1024, kernarg=0, occ=4)
    assert kid.metadata(BRANCH) == m
