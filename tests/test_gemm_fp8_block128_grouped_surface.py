"""CPU: the grouped (MoE) block-scaled FP8 GEMM (include/cln_amd_ext.h: cln_gemm_fp8_block128_grouped_bf16 with its describe entry; DESIGN
4.4.28): exports, the form a shape runs under the rule and under each pin, the slot count, and what is refused. No GPU needed."""
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

NAME = "cln_gemm_fp8_block128_grouped_bf16"
I, VP = ctypes.c_int, ctypes.c_void_p


def test_header_library_package_and_host_hold_the_names(built):
    lib, hdr = fs._lib(), open(si.HDR).read()
    from cuda_learn_notes_amd import host
    for n in (NAME, NAME + "_describe"):
        assert hasattr(lib, n) and re.search(r"\bint %s\(" % n, hdr), n
    assert hasattr(built, NAME[4:]) and hasattr(host, NAME[4:]) and hasattr(built.manifest, "describe_" + NAME[4:])


def test_the_offsets_layer_and_the_tile_body_are_shared_not_restated():
    read = lambda fn: open(os.path.join(fs.CSRC, fn)).read()
    heads = {u: read(u + ".cuh") for u in ("gemm_fp8_block128", "gemm_fp8_block128_grouped", "gemm_fp8_block128_grouped_swiglu")}
    assert sum("while (lo < hi)" in t for t in heads.values()) == 0 and "while (lo < hi)" in read("gemm_fp8_block128_offsets.cuh")  # one search
    for u in ("gemm_fp8_block128_grouped", "gemm_fp8_block128_grouped_swiglu"):
        assert '#include "gemm_fp8_block128_offsets.cuh"' in heads[u] and '#include "gemm_fp8_block128_core.cuh"' in heads[u], u
        assert '#include "gemm_fp8_block128.cuh"' not in heads[u], u  # the dense header defines the dense kernels
    for fn in ("gemm_fp8_block128_core.cuh", "gemm_fp8_block128_offsets.cuh", "fp8_block_scale.cuh"):
        assert "__global__" not in read(fn), fn
    grouped = heads["gemm_fp8_block128_grouped"]
    assert "lds_st<u4>" not in grouped and not re.search(r"\bstruct Stage\b", grouped) and not re.search(r"\bvoid tile\(", grouped)
    assert "g8::tile(" in grouped and re.search(r"\bvoid tile\(const Args& a, int m_t,", read("gemm_fp8_block128_core.cuh"))


@pytest.mark.parametrize("M,E,N,K", [(4, 1, 4096, 7168), (5, 1, 4096, 7168), (1024, 256, 7168, 2048), (1025, 256, 264, 384), (280, 7, 264, 384)])
def test_describe_names_the_form_the_grid_and_the_slots_and_reports_no_scratch(built, M, E, N, K):
    d = built.manifest.describe_gemm_fp8_block128_grouped_bf16
    rule = "skinny" if M <= 4 * E else "tile"
    slots = M // 128 + E
    texts = {form: d(M, E, N, K, form) for form in (None, "skinny", "tile")}
    for form, t in texts.items():
        ran = form or rule
        assert t.startswith("gemm_fp8_block128_grouped_%s_mfma M_total=%d E=%d N=%d K=%d: form %s (" % (ran, M, E, N, K, ran)), t
        assert ("by the rule" in t) == (form is None) and ("pinned; the rule gives " + rule in t) == (form is not None)
        assert "0 bytes scratch" in t and "no spill" in t and "%d slots" % slots in t
    assert texts[None] == texts[rule].replace("pinned; the rule gives " + rule, "by the rule: M_total %s 4 E" % ("<=" if rule == "skinny" else ">"))
    waves = 4 if -(-N // 64) * E >= 256 else 2  # 64-row strips only where strips x E workgroups cover the 256 CUs
    assert "grid %d x %d workgroups of %d threads" % (-(-N // (16 * waves)), E, 64 * waves) in texts["skinny"] and "no LDS" in texts["skinny"]
    assert "returns before its first weight load when M_e = 0" in texts["skinny"]
    assert "grid %d x %d workgroups of 256 threads" % (-(-N // 128), slots) in texts["tile"] and "66560 bytes static" in texts["tile"]


@pytest.mark.parametrize("M,E,N,K,form", [(4, 2, 12, 128, 0), (4, 2, 16, 192, 0), (4, 0, 16, 128, 0), (0, 2, 16, 128, 0), (4, 2, 16, 128, 3)],
                         ids=["N=12", "K=192", "E=0", "M_total=0", "form=3"])
def test_unsupported_shapes_and_forms_are_refused(built, M, E, N, K, form):
    rc = -1 if form == 3 else -2  # the shape first (-2), then pointers and the form (-1)
    buf = ctypes.create_string_buffer(3072)
    assert fs._fn(NAME + "_describe", [I] * 5 + [ctypes.c_char_p, I])(M, E, N, K, form, buf, 3072) == rc
    assert fs._fn(NAME, [VP] * 6 + [I] * 5 + [VP])(None, None, None, None, None, None, M, E, N, K, form, None) == rc
    kb, nb = K // 128, -(-N // 128)
    with pytest.raises(ValueError):
        built.manifest.describe_gemm_fp8_block128_grouped_bf16(M, E, N, K, "both" if form else None)
    with pytest.raises(ValueError):
        built.gemm_fp8_block128_grouped_bf16(torch.zeros(M, K).to(gr.F8), torch.zeros(M, kb), torch.zeros(E, N, K).to(gr.F8), torch.zeros(E, nb, kb),
                                             torch.zeros(E + 1, dtype=torch.int32), torch.zeros(M, N, dtype=gr.BF), form="both" if form else None)


def test_a_launch_whose_slots_or_experts_pass_the_grid_is_refused(built):
    d = built.manifest.describe_gemm_fp8_block128_grouped_bf16
    assert "x 65535 workgroups" in d(128 * 65000, 535, 8, 128, "tile")
    for M, E, form in ((128 * 65000, 536, "tile"), (1, 65536, "skinny"), (1, 65536, None)):
        with pytest.raises(ValueError):
            d(M, E, 8, 128, form)
