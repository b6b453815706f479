"""CPU: the MoE token path (include/cln_amd_ext.h: cln_moe_route_topk, cln_moe_sort_plan, cln_moe_sort, cln_moe_dispatch_fp8_block128_bf16,
cln_moe_dispatch_mxfp8_bf16, cln_moe_combine_bf16 with their describe entries): exports, what the describe texts state, and what
is refused through the C entries (null pointers: the shape is judged first) and through Python. No GPU needed."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_mla_index_surface as si  # noqa: E402  (HDR)
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the readers of the built library)

NAMES = ("moe_route_topk", "moe_sort_plan", "moe_sort", "moe_dispatch_fp8_block128_bf16", "moe_dispatch_mxfp8_bf16", "moe_combine_bf16")
I, VP, F = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
BF, F8, E8, I32 = torch.bfloat16, torch.float8_e4m3fn, torch.float8_e8m0fnu, torch.int32


def test_header_library_package_and_host_hold_the_six_names(built):
    lib, hdr = fs._lib(), open(si.HDR).read()
    from cuda_learn_notes_amd import host
    for name in NAMES:
        for n in ("cln_" + name, "cln_" + name + "_describe"):
            assert hasattr(lib, n) and re.search(r"\bint %s\(" % n, hdr), n
        assert hasattr(built, name) and hasattr(host, name) and hasattr(built.manifest, "describe_" + name), name


def test_describe_texts_name_kernel_grid_launches_chunk_and_no_scratch(built):
    m = built.manifest
    blocks, chunk, ws = built.moe_sort_plan(3 * 2048 + 17, 256)
    assert (blocks, chunk, ws) == (4, 2048, 4 * 4 * 256) and built.moe_sort_plan(2048, 256) == (1, 2048, 0)
    texts = {
        "moe_route_topk_wave<bf16, 2> T=5 E=128 k=4 softmax renormalize: one launch": m.describe_moe_route_topk(5, 128, 4),
        "grid 2 workgroups of 256 threads, one wave a token": m.describe_moe_route_topk(5, 128, 4),
        "moe_route_topk_wave<float, 8> T=3 E=512 k=10 sigmoid:": m.describe_moe_route_topk(3, 512, 10, True, "sigmoid", False),
        "blocks 1, chunk 2048 slots, 1 launch, no workspace: moe_sort_rank<one>, grid 1 workgroup": m.describe_moe_sort(2048, 256),
        "blocks 4, chunk 2048 slots, 3 launches on the stream, workspace 4096 bytes": m.describe_moe_sort(3 * 2048 + 17, 256),
        "moe_sort_hist (grid 4 workgroups": m.describe_moe_sort_plan(3 * 2048 + 17, 256),
        "moe_dispatch_rows<fp8_block128> rows=27 T=9 k=3 K=384 scale_pow2=1: one launch": m.describe_moe_dispatch_fp8_block128_bf16(27, 9, 3, 384, True),
        "grid 7 x 1 workgroups of 256 threads, 64 thread places": m.describe_moe_dispatch_fp8_block128_bf16(27, 9, 3, 384),
        "moe_dispatch_rows<mxfp8> rows=27 T=9 k=3 K=416: one launch": m.describe_moe_dispatch_mxfp8_bf16(27, 9, 3, 416),
        "grid 27 x 2 workgroups of 256 threads": m.describe_moe_dispatch_mxfp8_bf16(27, 9, 3, 2880),
        "moe_combine_rows M_total=500 T=67 N=2880 k=8: one launch": m.describe_moe_combine_bf16(500, 67, 2880, 8),
        "grid 67 x 2 workgroups of 192 threads": m.describe_moe_combine_bf16(500, 67, 2880, 8),
    }
    for want, text in texts.items():
        assert want in text and "0 bytes scratch" in text and "no spill" in text and "deterministic" in text, (want, text)


def _c(name, types):
    return fs._fn("cln_" + name, types)


CASES = {  # id -> (C call on null pointers, its status, the Python call that must raise ValueError)
    "E=513": (lambda: _c(NAMES[0], [VP] * 4 + [I] * 6 + [F, VP])(None, None, None, None, 4, 513, 2, 0, 0, 1, 1.0, None), -2,
              lambda c: c.moe_route_topk(torch.zeros(4, 513), torch.zeros(4, 2, dtype=I32), torch.zeros(4, 2))),
    "k=17": (lambda: _c(NAMES[0], [VP] * 4 + [I] * 6 + [F, VP])(None, None, None, None, 4, 64, 17, 0, 0, 1, 1.0, None), -2,
             lambda c: c.moe_route_topk(torch.zeros(4, 64), torch.zeros(4, 17, dtype=I32), torch.zeros(4, 17))),
    "k>E": (lambda: _c(NAMES[0], [VP] * 4 + [I] * 6 + [F, VP])(None, None, None, None, 4, 3, 4, 0, 0, 1, 1.0, None), -2,
            lambda c: c.moe_route_topk(torch.zeros(4, 3), torch.zeros(4, 4, dtype=I32), torch.zeros(4, 4))),
    "softmax+bias": (lambda: _c(NAMES[0], [VP] * 4 + [I] * 6 + [F, VP])(None, 64, None, None, 4, 8, 2, 0, 0, 1, 1.0, None), -2,
                     lambda c: c.moe_route_topk(torch.zeros(4, 8), torch.zeros(4, 2, dtype=I32), torch.zeros(4, 2), bias=torch.zeros(8))),
    "K=48 fp8": (lambda: _c(NAMES[3], [VP] * 4 + [I] * 5 + [VP])(None, None, None, None, 6, 3, 2, 48, 0, None), -2,
                 lambda c: c.moe_dispatch_fp8_block128_bf16(torch.zeros(3, 48, dtype=BF), torch.zeros(6, dtype=I32), 2,
                                                            torch.zeros(6, 48).to(F8), torch.zeros(6, 0))),
    "K=48 mx": (lambda: _c(NAMES[4], [VP] * 4 + [I] * 4 + [VP])(None, None, None, None, 6, 3, 2, 48, None), -2,
                lambda c: c.moe_dispatch_mxfp8_bf16(torch.zeros(3, 48, dtype=BF), torch.zeros(6, dtype=I32), 2, torch.zeros(6, 48).to(F8),
                                                    torch.zeros(6, 1, dtype=torch.uint8).view(E8))),
    "N=12": (lambda: _c(NAMES[5], [VP] * 5 + [I] * 4 + [VP])(None, None, None, None, None, 6, 3, 12, 2, None), -2,
             lambda c: c.moe_combine_bf16(torch.zeros(6, 12, dtype=BF), torch.zeros(3, 2, dtype=I32), torch.zeros(3, 2), torch.zeros(3, 12, dtype=BF))),
    "n_slots=0": (lambda: _c(NAMES[2], [VP] * 5 + [I] * 2 + [VP])(None, None, None, None, None, 0, 8, None), -1,
                  lambda c: c.moe_sort(torch.zeros(0, 2, dtype=I32), 8, torch.zeros(9, dtype=I32), torch.zeros(0, dtype=I32),
                                       torch.zeros(0, 2, dtype=I32))),
}


@pytest.mark.parametrize("case", list(CASES))
def test_unsupported_shapes_are_refused_before_any_pointer_is_looked_at(built, case):
    c_call, rc, py_call = CASES[case]
    assert c_call() == rc
    with pytest.raises(ValueError):
        py_call(built)


def test_a_supported_shape_with_null_pointers_is_a_bad_argument(built):
    assert _c(NAMES[0], [VP] * 4 + [I] * 6 + [F, VP])(None, None, None, None, 4, 64, 2, 0, 0, 1, 1.0, None) == -1
    assert _c(NAMES[2], [VP] * 5 + [I] * 2 + [VP])(None, None, None, None, None, 4096, 8, None) == -1
    assert _c(NAMES[5], [VP] * 5 + [I] * 4 + [VP])(None, None, None, None, None, 6, 3, 16, 2, None) == -1
    with pytest.raises(ValueError):
        built.moe_sort_plan(16, 65536)
