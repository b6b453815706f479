"""CPU: the latent cache in DeepSeek-V3.2's own FP8 row of 656 bytes: exports and describes, the decodes' status order against
the sparse FP8 siblings', the plans, the views against the documented byte offsets, the compiled kernels' resources. No GPU needed."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_dsa_varlen_surface as vs  # noqa: E402  (its readers of the built library; fs = the sibling surface test's helpers)


fs = vs.fs
I, LL, VP, F = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_float
APPEND, FIXED, PACKED = "cln_kv_append_paged_mla_bf16_fp8_tile", "cln_fa2_decode_paged_mla_sparse_bf16_fp8_tile", "cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8_tile"
NAMES = (APPEND, FIXED, PACKED) + tuple(n + "_describe" for n in (APPEND, FIXED, PACKED)) + (FIXED + "_plan", PACKED + "_plan")


def test_library_header_manifest_package_host_and_build_hold_the_entries(built):
    lib = fs._lib()
    from cuda_learn_notes_amd import host
    for n in NAMES:
        assert hasattr(lib, n), n
        if not n.endswith("_describe"):
            assert hasattr(built, n[4:]) and hasattr(host, n[4:]), n
    m, buf = built.manifest, ctypes.create_string_buffer(8192)
    for name, mirror, dims in ((FIXED, m.describe_decode_paged_mla_sparse_bf16_fp8_tile, (3, 2, 40, 1024, 128, 16)),
                               (PACKED, m.describe_decode_paged_mla_sparse_varlen_bf16_fp8_tile, (7, 81, 128, 2048, 128, 16))):
        rc = fs._fn(name + "_describe", [I] * 6 + [F, ctypes.c_char_p, I])(*dims, 0.1, buf, 8192)
        text = buf.value.decode()
        assert rc == len(text) and text == mirror(*dims, 0.1) and "656 bytes" in text and "75776 bytes static" in text and "workspace" in text
    rc = fs._fn(APPEND + "_describe", [I] * 7 + [ctypes.c_char_p, I])(4, 27, 3, 8, 16, 1, 1, buf, 8192)
    assert rc == len(buf.value) and buf.value.decode() == m.describe_kv_append_paged_mla_bf16_fp8_tile(4, 27, 3, 8, 16, "half", True)


@pytest.mark.parametrize("packed", [False, True], ids=["fixed-T", "packed"])
def test_decode_statuses_are_the_sparse_fp8_siblings_without_kv_scale(built, packed):
    """One battery of bad calls through the new entry and through the sibling (its kv_scale slot always good): the same statuses in order."""
    n_int = 4 if packed else 3  # block_table, seqlens, [cu_q,] indices
    dims = (2, 6, 128, 2048, 5, 128, 16)  # B, T or total_q, Hq, topk, P, max_pages, page: the plan splits
    plan_dims = (6, 128, 2048, 128, 16) if packed else (2, 6, 128, 2048, 128, 16)
    new, sib = (PACKED, "cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8") if packed else (FIXED, "cln_fa2_decode_paged_mla_sparse_bf16_fp8")
    need = fs._plan(new + "_plan", *plan_dims)[1][2]
    assert need > 0 and fs._plan(new + "_plan", *plan_dims) == fs._plan(sib + "_plan", *plan_dims)
    keep, (*ptrs, scale_ptr) = vs._ptrs(2 + n_int + 3 + 1)

    def battery(name, with_scale):
        fn = fs._fn(name, [VP] * (len(ptrs) + with_scale) + [LL] + [I] * 7 + [F, VP])

        def call(a, ws=need, d=dims, s=0.1):
            a = list(a)
            if with_scale:
                a.insert(2 + n_int - 1, scale_ptr)  # kv_scale stands in front of indices
            return fn(*a, ws, *d, s, None)
        bad_hq = (2, 6, 129, 2048, 5, 128, 16)  # every call that could pass its pointer checks is refused by the plan: nothing is launched
        out = [call(ptrs, s=s, d=bad_hq) for s in (0.0, -1.0, float("nan"), float("inf"))]
        for i in range(len(ptrs)):
            out += [call(ptrs[:i] + [bad] + ptrs[i + 1:], d=bad_hq) for bad in (None, ptrs[i] + 2, ptrs[i] + 8)]
        out += [call(ptrs[:2 + n_int] + [ptrs[i]] + ptrs[3 + n_int:], d=bad_hq) for i in range(2 + n_int)]  # o equal to an input
        for i in range(7):
            out += [call(ptrs, d=dims[:i] + (v,) + dims[i + 1:]) for v in (0, -3)]
        out += [call(ptrs, d=d) for d in (bad_hq, (2, 6, 128, 2048, 5, 128, 48), (2, 6, 128, 2048, 5, 1 << 23, 256), (2, 6, 129, 2048, 0, 128, 16))]
        return out + [call(ptrs, ws=need - 1), call(ptrs, ws=need - 1, d=bad_hq)]

    got, want = battery(new, 0), battery(sib, 1)
    assert got == want and set(got) == {-1, -2} and got[:4] == [-1] * 4 and got[-2:] == [-1, -2]


def test_plans_are_the_bf16_sparse_plans(built):
    for B, T, Hq, topk, mp, page in ((1, 1, 1, 1, 128, 16), (3, 2, 40, 1024, 128, 16), (64, 1, 128, 2048, 2048, 64), (2, 3, 129, 64, 128, 16), (2, 3, 64, 64, 128, 48), (0, 1, 1, 1, 1, 16)):
        assert fs._plan(FIXED + "_plan", B, T, Hq, topk, mp, page) == fs._plan("cln_fa2_decode_paged_mla_sparse_bf16_plan", B, T, Hq, topk, mp, page)
        assert fs._plan(PACKED + "_plan", B * T, Hq, topk, mp, page) == fs._plan("cln_fa2_decode_paged_mla_sparse_varlen_bf16_plan", B * T, Hq, topk, mp, page)


def test_views_alias_the_storage_at_the_documented_offsets(built):
    pool = torch.zeros(3, 16, 656, dtype=torch.uint8)
    codes, scales, k_pe = built.latent_pool_fp8_tile_views(pool)
    assert [(t.dtype, tuple(t.shape)) for t in (codes, scales, k_pe)] == [(torch.float8_e4m3fn, (3, 16, 512)), (torch.float32, (3, 16, 4)), (torch.bfloat16, (3, 16, 64))]
    base = pool.data_ptr()
    assert (codes.data_ptr(), scales.data_ptr(), k_pe.data_ptr()) == (base, base + 512, base + 528)
    assert codes[1, 2].data_ptr() - base == scales[1, 2].data_ptr() - base - 512 == k_pe[1, 2].data_ptr() - base - 528 == (16 + 2) * 656
    codes.view(torch.uint8)[1, 2, 7], scales[1, 2, 3], k_pe[1, 2, 63] = 0x38, 0.5, 2.0  # written through the views, read from the bytes
    row = pool[1, 2]
    assert row[7] == 0x38 and row[524:528].view(torch.float32).item() == 0.5 and row[654:].view(torch.bfloat16).item() == 2.0
    for bad in (pool[:, :, :655], pool.view(3, 656, 16), torch.zeros(3, 48, 656, dtype=torch.uint8), pool.float()):
        with pytest.raises(RuntimeError):
            built.latent_pool_fp8_tile_views(bad)


def test_kernel_resources_in_the_built_library_and_the_loop_mfmas(built, tmp_path):
    """The built library: two instantiations, no spill, no scratch, 75776 bytes of LDS. The compile units: 136 bf16 MFMAs in the one loop, no _f16."""
    mine = sorted((n, k) for n, k in vs._built_kernels(tmp_path).items() if "fp8_tile_mfma" in n)
    assert len(mine) == 2 and "ILb0E" in mine[0][0] and "ILb1E" in mine[1][0], [n for n, _ in mine]
    for n, k in mine:
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
        assert k["group_segment_fixed_size"] == 75776 and k["vgpr_count"] <= 512, (n, k)
    for unit in ("flash_attn_decode_paged_mla_sparse_bf16_fp8_tile.hip", "flash_attn_decode_paged_mla_sparse_varlen_bf16_fp8_tile.hip"):
        main = [(k, b) for k, b in fs._bodies(unit, tmp_path) if "combine" not in k["name"]]  # asserts no spill, no scratch, no _f16
        assert len(main) == 1 and fs._loop_mfmas(main[0][1]) == 136 and "v_cvt_pk_bf16_f32" in main[0][1]
