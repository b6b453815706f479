"""CPU: the block-scaled FP8 GEMM and its quantiser (include/cln_amd_ext.h: cln_gemm_fp8_block128_bf16, cln_quant_fp8_block128_bf16 with their
describe entries): exports, the form a shape runs, the shapes that are refused, and the test helper's own reference. No GPU
needed."""
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

GEMM, QUANT = "cln_gemm_fp8_block128_bf16", "cln_quant_fp8_block128_bf16"
I, VP = ctypes.c_int, ctypes.c_void_p


def test_header_library_package_and_host_hold_the_four_names(built):
    lib, hdr = fs._lib(), open(si.HDR).read()
    from cuda_learn_notes_amd import host
    for n in (GEMM, GEMM + "_describe", QUANT, QUANT + "_describe"):
        assert hasattr(lib, n) and re.search(r"\bint %s\(" % n, hdr), n
    for n in (GEMM, QUANT):
        assert hasattr(built, n[4:]) and hasattr(host, n[4:]) and hasattr(built.manifest, "describe_" + n[4:]), n


def test_describe_names_the_form_by_m_alone_and_reports_no_scratch(built):
    m = built.manifest
    for N, K in ((1536, 7168), (576, 512), (8, 128)):
        skinny, tile = m.describe_gemm_fp8_block128_bf16(64, N, K), m.describe_gemm_fp8_block128_bf16(65, N, K)
        assert skinny.startswith("gemm_fp8_block128_mfma<skinny, MT=4> M=64 N=%d K=%d: form skinny" % (N, K)) and "no LDS" in skinny
        assert tile.startswith("gemm_fp8_block128_mfma<tile> M=65 N=%d K=%d: form tile" % (N, K)) and "66560 bytes static" in tile
        assert "0 bytes scratch" in skinny and "0 bytes scratch" in tile and "no spill" in skinny and "no spill" in tile
    assert "MT=1" in m.describe_gemm_fp8_block128_bf16(16, 64, 128) and "MT=2" in m.describe_gemm_fp8_block128_bf16(17, 64, 128)
    assert "a strip of 32 weight rows" in m.describe_gemm_fp8_block128_bf16(1, 1536, 7168)
    assert "a strip of 64 weight rows" in m.describe_gemm_fp8_block128_bf16(1, 24576, 1536)
    assert "0 bytes scratch" in m.describe_quant_fp8_block128_bf16(3, 7168, True)


@pytest.mark.parametrize("M,N,K", [(4, 12, 128), (4, 16, 192), (4, 16, 0), (0, 16, 128)], ids=["N=12", "K=192", "K=0", "M=0"])
def test_unsupported_shapes_are_refused_before_anything_else(built, M, N, K):
    buf = ctypes.create_string_buffer(2048)
    assert fs._fn(GEMM + "_describe", [I] * 3 + [ctypes.c_char_p, I])(M, N, K, buf, 2048) == -2
    assert fs._fn(GEMM, [VP] * 5 + [I] * 3 + [VP])(None, None, None, None, None, M, N, K, None) == -2
    with pytest.raises(ValueError):
        built.manifest.describe_gemm_fp8_block128_bf16(M, N, K)
    kb, nb = K // 128, -(-N // 128)
    with pytest.raises(ValueError):
        built.gemm_fp8_block128_bf16(torch.zeros(M, K).to(gr.F8), torch.zeros(M, kb), torch.zeros(N, K).to(gr.F8), torch.zeros(nb, kb),
                                     torch.zeros(M, N, dtype=gr.BF))
    if N % 8 == 0:  # the quantiser has no N
        assert fs._fn(QUANT, [VP] * 3 + [I] * 3 + [VP])(None, None, None, M, K, 0, None) == -2
        with pytest.raises(ValueError):
            built.quant_fp8_block128_bf16(torch.zeros(M, K, dtype=gr.BF), torch.zeros(M, K).to(gr.F8), torch.zeros(M, kb))


def test_the_scale_rule_is_written_in_one_file_under_csrc():
    holders = [os.path.relpath(os.path.join(d, fn), fs.CSRC) for d, _, fns in os.walk(fs.CSRC) for fn in fns
               if "1e-4f) / 448.0f" in open(os.path.join(d, fn), errors="replace").read()]
    assert holders == ["fp8_block_scale.cuh"], holders
    for u in ("quant_fp8_block128_bf16", "gemm_fp8_block128_grouped_swiglu", "kv_append_paged_index_bf16_fp8", "kv_append_paged_mla_bf16_fp8_tile"):
        text = open(os.path.join(fs.CSRC, u + ".cuh")).read()
        assert '#include "fp8_block_scale.cuh"' in text and "cln_fp8_block_scale(" in text, u  # one rule, called by all four


def test_the_library_holds_the_four_dense_kernels_once(built, tmp_path):
    """The grouped units include the kernel-free core header, not the dense header: only the dense unit instantiates the dense kernels."""
    sys.path.insert(0, os.path.join(fs.ROOT, "cuda-learn-notes_amd", "tools"))
    import mfma_overlap_scan as scan
    from cuda_learn_notes_amd import _loader
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    names = []
    scan.shared_object_spills(_loader.so_path("libcln_amd.so"), str(tmp_path), names)
    dense = sorted(n for n in names if "gemm_fp8_block128_mfmaILb" in n)
    assert len(dense) == 4 and len(set(dense)) == 4, dense
    for form in ("gemm_fp8_block128_grouped_skinny_mfma", "gemm_fp8_block128_grouped_tile_mfma", "gemm_fp8_block128_grouped_swiglu_skinny_mfma",
                 "gemm_fp8_block128_grouped_swiglu_tile_mfma"):
        assert sum(form in n for n in names) == 1, form


def test_the_helpers_reference_is_dequantise_then_matmul():
    _, a, sa, b, sb, (ref, S) = gr.gaussian(17, 264, 384)
    ad = a.double() * sa.double().repeat_interleave(128, dim=1)
    bd = b.double() * sb.double().repeat_interleave(128, dim=0)[:264].repeat_interleave(128, dim=1)
    direct = ad @ bd.T
    assert float((ref - direct).abs().max()) <= 1e-12 * float(direct.abs().max()) and bool((S * (1 + 1e-12) >= ref.abs()).all())
    assert len({float(v) for v in sb.flatten()}) == sb.numel() and len({float(v) for v in sa.flatten()}) > sa.numel() // 2  # (amax is a bf16)
    assert not bool(((sb.flatten().view(torch.int32) & 0x007FFFFF) == 0).any())  # no weight scale is a power of two
