"""CPU: the fused gate/up + SiLU-mul + quantise grouped FP8 GEMM (include/cln_amd_ext.h: cln_gemm_fp8_block128_grouped_swiglu_fp8 with its
describe entry): exports, the form a shape runs under the rule and under each pin, the grid, the slots and the LDS, and what
is refused. No GPU needed."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_fp8_block128_reference as gr  # noqa: E402
import test_mla_index_surface as si  # noqa: E402  (HDR)
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the readers of the built library)

NAME = "cln_gemm_fp8_block128_grouped_swiglu_fp8"
INT, VP = ctypes.c_int, ctypes.c_void_p


def test_header_library_package_and_host_hold_the_names(built):
    lib, hdr = fs._lib(), open(si.HDR).read()
    from cuda_learn_notes_amd import host
    for n in (NAME, NAME + "_describe"):
        assert hasattr(lib, n) and re.search(r"\bint %s\(" % n, hdr), n
    assert hasattr(built, NAME[4:]) and hasattr(host, NAME[4:]) and hasattr(built.manifest, "describe_" + NAME[4:])


def test_the_offsets_layer_and_the_scale_rule_are_included_not_restated():
    text = open(os.path.join(fs.CSRC, "gemm_fp8_block128_grouped_swiglu.cuh")).read()
    for inc in ("gemm_fp8_block128_core.cuh", "gemm_fp8_block128_offsets.cuh", "fp8_block_scale.cuh"):
        assert '#include "%s"' % inc in text, inc
    assert '#include "gemm_fp8_block128.cuh"' not in text and '#include "kv_append_paged_fp8.cuh"' not in text
    for restated in ("clamped_offset(const", "slot_of(int", "expert_of_slot(const", "auto_skinny(long", "kSkinnyMeanRows =", "kMaxGridY =", "block_scale(float"):
        assert restated not in text, restated
    assert "g8o::tile_of_slot(" in text and "g8o::expert_rows(" in text and "g8o::plan_form(" in text and text.count("cln_fp8_block_scale(") == 2


@pytest.mark.parametrize("M,E,I,K", [(4, 1, 2048, 7168), (5, 1, 2048, 7168), (1024, 256, 2048, 7168), (1025, 256, 256, 384), (280, 7, 256, 1024)])
def test_describe_names_the_form_the_grid_the_slots_and_the_lds_and_reports_no_scratch(built, M, E, I, K):
    d = built.manifest.describe_gemm_fp8_block128_grouped_swiglu_fp8
    rule = "skinny" if M <= 4 * E else "tile"
    slots = M // 128 + E
    texts = {form: d(M, E, I, K, form) for form in (None, "skinny", "tile")}
    for form, t in texts.items():
        ran = form or rule
        assert t.startswith("gemm_fp8_block128_grouped_swiglu_%s_mfma M_total=%d E=%d I=%d K=%d: form %s (" % (ran, M, E, I, K, ran)), t
        assert ("by the rule" in t) == (form is None) and ("pinned; the rule gives " + rule in t) == (form is not None)
        assert "0 bytes scratch" in t and "no spill" in t and "%d slots" % slots in t
    assert texts[None] == texts[rule].replace("pinned; the rule gives " + rule, "by the rule: M_total %s 4 E" % ("<=" if rule == "skinny" else ">"))
    assert "grid %d x %d workgroups of 512 threads" % (I // 128, E) in texts["skinny"] and "4096 bytes static" in texts["skinny"]
    assert "returns before its first weight load when M_e = 0" in texts["skinny"]
    assert "grid %d x %d workgroups of 256 threads" % (I // 128, slots) in texts["tile"]
    assert "2 LDS slots of 49664 bytes" in texts["tile"] and "99328 bytes dynamic" in texts["tile"]


@pytest.mark.parametrize("M,E,I,K,form", [(4, 2, 192, 128, 0), (4, 2, 64, 128, 0), (4, 2, 128, 192, 0), (4, 0, 128, 128, 0), (0, 2, 128, 128, 0),
                                          (4, 2, 128, 128, 3)], ids=["I=192", "I=64", "K=192", "E=0", "M_total=0", "form=3"])
def test_unsupported_shapes_and_forms_are_refused(built, M, E, I, K, form):
    rc = -1 if form == 3 else -2  # the shape first (-2), then pointers and the form (-1)
    buf = ctypes.create_string_buffer(4096)
    assert fs._fn(NAME + "_describe", [INT] * 5 + [ctypes.c_char_p, INT])(M, E, I, K, form, buf, 4096) == rc
    assert fs._fn(NAME, [VP] * 7 + [INT] * 6 + [VP])(None, None, None, None, None, None, None, M, E, I, K, form, 0, None) == rc
    kb = K // 128
    with pytest.raises(ValueError):
        built.manifest.describe_gemm_fp8_block128_grouped_swiglu_fp8(M, E, I, K, "both" if form else None)
    with pytest.raises(ValueError):
        built.gemm_fp8_block128_grouped_swiglu_fp8(torch.zeros(M, K).to(gr.F8), torch.zeros(M, kb), torch.zeros(E, 2 * I, K).to(gr.F8),
                                                   torch.zeros(E, 2 * I // 128, kb), torch.zeros(E + 1, dtype=torch.int32),
                                                   torch.zeros(M, I).to(gr.F8), torch.zeros(M, I // 128), form="both" if form else None)


def test_a_launch_whose_slots_or_experts_pass_the_grid_is_refused(built):
    d = built.manifest.describe_gemm_fp8_block128_grouped_swiglu_fp8
    assert "x 65535 workgroups" in d(128 * 65000, 535, 128, 128, "tile")
    for M, E, form in ((128 * 65000, 536, "tile"), (1, 65536, "skinny"), (1, 65536, None)):
        with pytest.raises(ValueError):
            d(M, E, 128, 128, form)
