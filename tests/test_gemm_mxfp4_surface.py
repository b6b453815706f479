"""CPU: the MXFP4-weight GEMMs and their MXFP8 quantiser (include/cln_amd_ext.h: cln_gemm_mxfp4_bf16, cln_gemm_mxfp4_grouped_bf16,
cln_quant_mxfp8_bf16 with their describe entries): exports, the form a shape runs under the rule and under each pin, and what
is refused. No GPU needed."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_mxfp4_reference as mr  # noqa: E402
import test_mla_index_surface as si  # noqa: E402  (HDR)
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the readers of the built library)

NAMES = ("cln_gemm_mxfp4_bf16", "cln_gemm_mxfp4_grouped_bf16", "cln_quant_mxfp8_bf16")
I, VP = ctypes.c_int, ctypes.c_void_p


def test_header_library_package_and_host_hold_the_six_names(built):
    lib, hdr = fs._lib(), open(si.HDR).read()
    from cuda_learn_notes_amd import host
    for name in NAMES:
        for n in (name, name + "_describe"):
            assert hasattr(lib, n) and re.search(r"\bint %s\(" % n, hdr), n
        assert hasattr(built, name[4:]) and hasattr(host, name[4:]) and hasattr(built.manifest, "describe_" + name[4:]), name


@pytest.mark.parametrize("M,N,K", [(1, 2880, 2880), (64, 5760, 2880), (65, 136, 416), (4096, 2880, 2880)])
def test_dense_describe_names_the_form_why_the_grid_and_the_lds(built, M, N, K):
    d = built.manifest.describe_gemm_mxfp4_bf16
    rule, steps = "skinny" if M <= 64 else "tile", -(-K // 128)
    texts = {form: d(M, N, K, form) for form in (None, "skinny", "tile")}
    for form, t in texts.items():
        ran = form or rule
        assert t.startswith("gemm_mxfp4_mfma<%s" % ran) and "M=%d N=%d K=%d: form %s (" % (M, N, K, ran) in t, t
        assert ("by the rule: M %s 64" % ("<=" if rule == "skinny" else ">") in t) == (form is None)
        assert ("pinned; the rule gives " + rule in t) == (form is not None)
        assert "0 bytes scratch" in t and "no spill" in t and "%d K steps" % steps in t
    waves = 4 if -(-N // 64) >= 256 else 2
    assert "grid %d workgroups of %d threads" % (-(-N // (16 * waves)), 64 * waves) in texts["skinny"] and "no LDS" in texts["skinny"]
    assert "grid %d x %d workgroups of 256 threads" % (-(-N // 128), -(-M // 128)) in texts["tile"] and "51200 bytes static" in texts["tile"]


@pytest.mark.parametrize("M,E,N,K", [(4, 1, 2880, 2880), (5, 1, 2880, 2880), (512, 128, 5760, 2880), (513, 128, 136, 416)])
def test_grouped_describe_names_the_form_the_grid_and_the_slots(built, M, E, N, K):
    d = built.manifest.describe_gemm_mxfp4_grouped_bf16
    rule, slots = "skinny" if M <= 4 * E else "tile", M // 128 + E
    texts = {form: d(M, E, N, K, form) for form in (None, "skinny", "tile")}
    for form, t in texts.items():
        ran = form or rule
        assert t.startswith("gemm_mxfp4_grouped_%s_mfma M_total=%d E=%d N=%d K=%d: form %s (" % (ran, M, E, N, K, ran)), t
        assert ("by the rule" in t) == (form is None) and ("pinned; the rule gives " + rule in t) == (form is not None)
        assert "0 bytes scratch" in t and "no spill" in t and "%d slots" % slots in t
    waves = 4 if -(-N // 64) * E >= 256 else 2
    assert "grid %d x %d workgroups of %d threads" % (-(-N // (16 * waves)), E, 64 * waves) in texts["skinny"] and "no LDS" in texts["skinny"]
    assert "returns before its first weight load when M_e = 0" in texts["skinny"]
    assert "grid %d x %d workgroups of 256 threads" % (-(-N // 128), slots) in texts["tile"] and "51200 bytes static" in texts["tile"]


def test_quantiser_describe_states_the_rule_and_no_scratch(built):
    t = built.manifest.describe_quant_mxfp8_bf16(130, 416)
    assert t.startswith("quant_mxfp8_bf16_rows M=130 K=416:") and "clamp(E - 8, 0, 254)" in t and "0 bytes scratch" in t and "no spill" in t


@pytest.mark.parametrize("M,E,N,K,form", [(4, 2, 16, 48, 0), (4, 2, 12, 64, 0), (4, 0, 16, 64, 0), (0, 2, 16, 64, 0), (4, 2, 16, 64, 3)],
                         ids=["K=48", "N=12", "E=0", "M=0", "form=3"])
def test_unsupported_shapes_and_forms_are_refused(built, M, E, N, K, form):
    rc = -1 if form == 3 else -2  # the shape first (-2), then pointers and the form (-1)
    buf = ctypes.create_string_buffer(4096)
    assert fs._fn(NAMES[1] + "_describe", [I] * 5 + [ctypes.c_char_p, I])(M, E, N, K, form, buf, 4096) == rc
    assert fs._fn(NAMES[1], [VP] * 7 + [I] * 5 + [VP])(None, None, None, None, None, None, None, M, E, N, K, form, None) == rc
    pin = "both" if form else None
    a, sa = torch.zeros(M, K).to(mr.F8), torch.zeros(M, K // 32, dtype=torch.uint8).view(mr.E8)
    with pytest.raises(ValueError):
        built.manifest.describe_gemm_mxfp4_grouped_bf16(M, E, N, K, pin)
    with pytest.raises(ValueError):
        built.gemm_mxfp4_grouped_bf16(a, sa, torch.zeros(E, N, K // 2, dtype=torch.uint8), torch.zeros(E, N, K // 32, dtype=torch.uint8),
                                      torch.zeros(E + 1, dtype=torch.int32), torch.zeros(M, N, dtype=mr.BF), form=pin)
    if E:  # the dense entry and the quantiser have no E
        assert fs._fn(NAMES[0] + "_describe", [I] * 4 + [ctypes.c_char_p, I])(M, N, K, form, buf, 4096) == rc
        assert fs._fn(NAMES[0], [VP] * 6 + [I] * 4 + [VP])(None, None, None, None, None, None, M, N, K, form, None) == rc
        with pytest.raises(ValueError):
            built.gemm_mxfp4_bf16(a, sa, torch.zeros(N, K // 2, dtype=torch.uint8), torch.zeros(N, K // 32, dtype=torch.uint8),
                                  torch.zeros(M, N, dtype=mr.BF), form=pin)
        if rc == -2 and N % 8 == 0:
            assert fs._fn(NAMES[2], [VP] * 3 + [I] * 2 + [VP])(None, None, None, M, K, None) == -2
            with pytest.raises(ValueError):
                built.quant_mxfp8_bf16(torch.zeros(M, K, dtype=mr.BF), a, sa)
