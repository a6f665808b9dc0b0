"""tools/wave_loop_report.py: the parser on a snippet of assembly written for this test (CPU, no compiler)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wave_loop_report as W   # noqa: E402

KERNEL = "5,1,12,1,false,2,14,false"
ASM = """
	.text
_ZN5acnqp16admm_wave_kernelILi5ELi1ELi12ELi1ELb0ELi2ELi14ELb1EEEvNS_9TiledArgsE:
	v_mfma_f64_16x16x4_f64 a[0:7], v[0:1], v[2:3], a[0:7]
	s_endpgm
.Lfunc_end0:
_ZN5acnqp16admm_wave_kernelILi5ELi1ELi12ELi1ELb0ELi2ELi14ELb0EEEvNS_9TiledArgsE: ; @kernel
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v0, 0
.LBB1_1:                                ; the pass loop
	v_mfma_f64_16x16x4_f64 a[0:7], v[0:1], v[2:3], a[0:7]
	global_load_dwordx2 v[4:5], v0, s[0:1]
.LBB1_2:                                ; the solver loop
	v_fma_f64 v[6:7], v[4:5], v[4:5], v[6:7]
	v_mfma_f64_16x16x4_f64 a[0:7], v[0:1], v[2:3], a[0:7] ; comment
	v_add_f64 v[6:7], v[6:7], v[4:5]
	v_accvgpr_read_b32 v8, a0
	v_mul_f64 v[6:7], v[6:7], v[4:5]
	v_mfma_f64_16x16x4_f64 a[8:15], v[0:1], v[2:3], a[8:15]
	ds_write_b64 v9, v[6:7]
	s_waitcnt lgkmcnt(0)
	s_cbranch_vccz .LBB1_4
; %bb.3:
	ds_read_b64 v[6:7], v9
	v_max_f64 v[6:7], v[6:7], v[6:7]
.LBB1_3:                                ; the water-filling loop
	v_min_f64 v[6:7], v[6:7], v[4:5]
	s_cbranch_execnz .LBB1_3
.LBB1_4:
	v_cmp_gt_f64_e32 vcc, v[6:7], v[4:5]
	scratch_load_dword v10, off, off
	s_cbranch_vccnz .LBB1_2
; %bb.5:
	s_cbranch_scc1 .LBB1_1
	s_endpgm
.Lfunc_end1:
"""


def test_symbol_of_an_instantiation():
    assert W.mangled(KERNEL) == "admm_wave_kernelILi5ELi1ELi12ELi1ELb0ELi2ELi14ELb0EE"
    assert W.mangled("5, 2, 6, 2, true, 0, 0, false").endswith("ILi5ELi2ELi6ELi2ELb1ELi0ELi0ELb0EE")


def test_instruction_classes():
    assert [W.classify(op) for op in ("v_mfma_f64_16x16x4_f64", "v_accvgpr_write_b32", "v_fma_f64", "ds_read_b64", "s_waitcnt", "global_load_dwordx2",
                                      "scratch_load_dword", "buffer_load_dword", "flat_load_dword")] == \
        ["mfma", "agpr_copy", "valu", "lds", "scalar", "memory", "memory", "memory", "memory"]


def test_the_solver_loop_of_the_named_kernel_segment_by_segment():
    r = W.report(ASM, KERNEL)
    assert r["kernel"] == "admm_wave_kernel<5, 1, 12, 1, false, 2, 14, false>"
    # the smallest loop with an MFMA: .LBB1_2 ... the branch back to it (not the pass loop, not the loop without one)
    assert [s["label"] for s in r["segments"]] == [".LBB1_2", ".LBB1_2+", ".LBB1_3", ".LBB1_4"]
    first = r["segments"][0]
    assert (first["instructions"], first["valu"], first["mfma"], first["agpr_copy"], first["lds"], first["scalar"]) == (9, 3, 2, 1, 1, 2)
    assert first["valu_between_mfma"] == [1, 2, 0] and first["branches"] == [".LBB1_4"]
    assert "valu_between_mfma" not in r["segments"][1] and r["segments"][1]["lds"] == 1
    assert r["segments"][2]["branches"] == [".LBB1_3"]
    assert (r["segments"][3]["memory"], r["segments"][3]["valu"], r["segments"][3]["branches"]) == (1, 1, [".LBB1_2"])
    assert r["totals"] == {"instructions": 16, "valu": 6, "mfma": 2, "lds": 2, "scalar": 4, "agpr_copy": 1, "memory": 1, "other": 0}


def test_a_kernel_that_is_not_there():
    with pytest.raises(KeyError):
        W.report(ASM, "5,4,6,2,false,2,14,false")
