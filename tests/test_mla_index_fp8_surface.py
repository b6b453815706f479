"""CPU: the DSA indexer's FP8 cache (include/cln_amd_ext.h: cln_kv_append_paged_index_bf16_fp8, cln_mla_index_logits_paged_bf16_fp8 with their
describe entries; csrc/kv_append_paged_index_bf16_fp8.*, csrc/mla_index_logits_paged_bf16_fp8.*) -- every status that returns
before a device call in its documented order, the Python entries' refusals, the describe texts against their manifest mirrors, the kernels'
resources in the built library, the plan of the large-pool test, index_pool_fp8_views against the documented byte offsets, the append reference against itself, and the
condition that the parity cases of tests/test_gpu_mla_index_fp8.py bite: each wrong reading of the scale or of the ReLU lies at least
20 x the bound from the reference at some visible position of every case. No GPU needed."""
import ctypes
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_kv_reference as fk  # noqa: E402
import mla_index_fp8_reference as x8  # noqa: E402
import mla_index_reference as ix  # noqa: E402
import test_mla_index_surface as si  # noqa: E402  (the bf16 sibling's readers of the built library)
import test_paged_bf16_fp8_surface as fs  # noqa: E402

APPEND, LOGITS = "cln_kv_append_paged_index_bf16_fp8", "cln_mla_index_logits_paged_bf16_fp8"
NAMES = (APPEND, APPEND + "_describe", LOGITS, LOGITS + "_describe")
UNITS = ("kv_append_paged_index_bf16_fp8", "mla_index_logits_paged_bf16_fp8")
I, LL, VP = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
APPEND_ARGS = [VP] * 5 + [I] * 6 + [VP]
BF, U8 = torch.bfloat16, torch.uint8
_fn, _ptrs = fs._fn, si._ptrs


# ---------------------------------------------------------------------------------------------------- header, exports

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_four_prototypes(tmp_path, lang, cc):
    import shutil
    import subprocess
    assert shutil.which(cc), cc
    protos = ("const void*, void*, const int*, const int*, const int*, int, int, int, int, int, int, void*", "int, int, int, int, int, char*, int",
              "const void*, const float*, const void*, const int*, const int*, float*, int, int, int, long long, int, int, int, void*",
              "int, int, int, long long, int, int, char*, int")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n' + "".join("int (*f%d)(%s) = %s;\n" % (i, p, n) for i, (p, n) in enumerate(zip(protos, NAMES)))
                   + "int main(void) { return f0 && f1 && f2 && f3 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(si.HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_header_manifest_package_host_and_build_hold_the_entries(built):
    lib, hdr = fs._lib(), open(si.HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in (APPEND, LOGITS):
        assert hasattr(built, n[4:]) and hasattr(host, n[4:]), n
        assert hasattr(built.manifest, "describe_" + n[4:]), n
    assert hasattr(built, "index_pool_fp8_views") and hasattr(host, "index_pool_fp8_views")
    build = open(os.path.join(si.ROOT, "cuda-learn-notes_amd", "_build.py")).read()
    for u in UNITS:
        assert '"%s.hip"' % u in build and all(os.path.exists(os.path.join(fs.CSRC, u + e)) for e in (".hip", ".cuh")), u


# ---------------------------------------------------------------------------------------------------- statuses

def test_append_statuses_in_their_order(built):
    """The bf16 entry's order with scale_pow2 between P and the shape: pointers, the pool equal to an input, P, scale_pow2, non-positive
    dimensions (-1), then the -2s. Nothing is launched before a refusal."""
    fn = _fn(APPEND, APPEND_ARGS)
    keep, (kn, pool, bt, sl, cu) = _ptrs(5)
    call = lambda *a, d=(2, 7, 5, 20, 16, 1): fn(*a, *d, None)  # noqa: E731  B, total_q, P, max_pages, page, scale_pow2
    for i in range(5):
        args = [kn, pool, bt, sl, cu]
        args[i] = None
        assert call(*args) == -1 and call(*args, d=(2, 7, 5, 20, 48, 1)) == -1, i
    for i, off in ((0, 8), (1, 8), (2, 2), (3, 2), (4, 2)):
        args = [kn, pool, bt, sl, cu]
        args[i] += off
        assert call(*args) == -1, i
    for i in (0, 2, 3, 4):  # the pool equal to an input
        args = [kn, pool, bt, sl, cu]
        args[1] = args[i]
        assert call(*args) == -1, i
    assert call(kn, pool, bt + 4, sl + 4, cu + 4, d=(2, 7, 0, 20, 48, 1)) == -1 and call(kn, pool, bt + 4, sl + 4, cu + 4, d=(2, 7, 5, 20, 48, 1)) == -2
    for pow2 in (2, -1, 256):  # neither 0 nor 1: -1, ahead of an unsupported page
        assert call(kn, pool, bt, sl, cu, d=(2, 7, 5, 20, 16, pow2)) == -1 and call(kn, pool, bt, sl, cu, d=(2, 7, 5, 20, 48, pow2)) == -1, pow2
    for pow2 in (0, 1):
        assert call(kn, pool, bt, sl, cu, d=(2, 7, 5, 20, 48, pow2)) == -2
    for d in ((0, 7, 5, 20, 16, 0), (2, 0, 5, 20, 16, 0), (2, 7, 5, 0, 16, 1), (2, 7, 5, 20, 0, 1)):
        assert call(kn, pool, bt, sl, cu, d=d) == -1, d
    for d in ((2, 7, 5, 20, 48, 0), (2, 7, 5, 20, 8, 1), (2, 7, 5, 1 << 23, 256, 1)):
        assert call(kn, pool, bt, sl, cu, d=d) == -2, d
    rc, _ = fs._describe(APPEND + "_describe", 2, 7, 20, 16, 2)
    assert rc == -1 and fs._describe(APPEND + "_describe", 2, 7, 20, 48, 1)[0] == -2 and fs._describe(APPEND + "_describe", 2, 0, 20, 16, 1)[0] == -1


def test_logits_statuses_in_their_order(built):
    """Exactly the bf16 entry's: pointers (q_idx, idx_pool 16 bytes; weights, block_table, seqlens, logits 4), output equal to an input, P,
    non-positive dimensions, then the -2s."""
    fn = _fn(LOGITS, si.LOGITS_ARGS)
    keep, (q, w, pool, bt, sl, lg) = _ptrs(6)
    dims = (2, 3, 64, 320, 5, 20, 16)  # B, T, Hi, ld, P, max_pages, page
    call = lambda *a, d=dims: fn(*a, *d, None)  # noqa: E731
    for i in range(6):
        args = [q, w, pool, bt, sl, lg]
        args[i] = None
        assert call(*args) == -1 and call(*args, d=(2, 3, 65, 320, 5, 20, 16)) == -1, i
    for i, off in ((0, 8), (1, 2), (2, 8), (3, 2), (4, 2), (5, 2)):
        args = [q, w, pool, bt, sl, lg]
        args[i] += off
        assert call(*args) == -1, i
    assert call(q, w + 4, pool, bt + 4, sl + 4, lg + 4, d=(2, 3, 64, 320, 0, 20, 16)) == -1
    assert call(q, w + 4, pool, bt + 4, sl + 4, lg + 4, d=(2, 3, 65, 320, 5, 20, 16)) == -2
    for i in range(5):
        args = [q, w, pool, bt, sl, lg]
        args[5] = args[i]
        assert call(*args, d=(2, 3, 65, 320, 5, 20, 16)) == -1, i
    assert call(q, w, pool, bt, sl, lg, d=(2, 3, 65, 320, 0, 20, 16)) == -1 and call(q, w, pool, bt, sl, lg, d=(2, 3, 65, 320, -1, 20, 48)) == -1
    for d in ((0, 3, 64, 320, 5, 20, 16), (2, 0, 64, 320, 5, 20, 16), (2, 3, 0, 320, 5, 20, 16), (2, 3, 64, 0, 5, 20, 16), (2, 3, 64, 320, 5, 0, 16),
              (2, 3, 64, 320, 5, 20, 0), (2, -1, 65, 320, 5, 20, 48)):
        assert call(q, w, pool, bt, sl, lg, d=d) == -1, d
    for d in ((2, 3, 65, 320, 5, 20, 16), (2, 3, 64, 320, 5, 20, 48), (2, 3, 64, 320, 5, 20, 8), (2, 3, 64, 320, 5, 20, 512),
              (2, 3, 64, 320, 5, 1 << 23, 256), (1 << 16, 1 << 15, 64, 320, 5, 20, 16), (1 << 12, 1 << 12, 64, 1 << 20, 5, 1 << 22, 256)):
        assert call(q, w, pool, bt, sl, lg, d=d) == -2, d
    dsc = _fn(LOGITS + "_describe", [I, I, I, LL, I, I, ctypes.c_char_p, I])
    buf = ctypes.create_string_buffer(4096)
    assert dsc(2, 3, 64, 320, 20, 16, None, 4096) == -1 and dsc(2, 3, 64, 320, 20, 16, buf, 0) == -1
    assert dsc(2, 3, 65, 320, 20, 16, buf, 4096) == -2 and dsc(2, 3, 64, 0, 20, 16, buf, 4096) == -1 and dsc(2, 3, 64, 1 << 40, 20, 16, buf, 4096) > 0


# ---------------------------------------------------------------------------------------------------- describe texts

def test_describe_texts_equal_their_manifest_mirrors(built):
    m = built.manifest
    buf = ctypes.create_string_buffer(8192)
    dl = _fn(LOGITS + "_describe", [I, I, I, LL, I, I, ctypes.c_char_p, I])
    for B, T, Hi, ld, mp, page in ((64, 1, 64, 131072, 2048, 64), (8, 3, 17, 320, 20, 16), (1, 2048, 1, 5000, 64, 64), (4, 4, 33, 100, 20, 256)):
        rc = dl(B, T, Hi, ld, mp, page, buf, 8192)
        text = buf.value.decode()
        cap = min(mp * page, ld)
        chunks = -(-cap // ix.CHUNK)
        assert rc == len(text) < 4000 and text == m.describe_mla_index_logits_paged_bf16_fp8(B, T, Hi, ld, mp, page)
        assert text.startswith("mla_index_logits_paged_bf16_fp8_mfma<NHB=%d> T=%d Hi=%d ld=%d cap=%d page=%d: " % (-(-Hi // 16), T, Hi, ld, cap, page))
        assert "%d workgroups of 4 waves" % (B * T * chunks) in text and "chunk of 1024 keys; %d chunks a token" % chunks in text
        assert "v_mfma_f32_16x16x32_bf16, %d MFMAs per block" % (4 * -(-Hi // 16)) in text and "%d padding heads" % (-Hi % 16) in text
        assert "a page is %d bytes: codes [%d,128] e4m3fn, then scales [%d] fp32" % (132 * page, page, page) in text
        assert "two dwordx4" in text and "v_cvt_scalef32_pk_bf16_fp8" in text and "scale once" in text
        assert "no LDS" in text and "nothing else" in text and text.endswith("; deterministic") and "_f16" not in text
    for B, tq, mp, page, pow2 in ((64, 64, 2048, 64, 1), (3, 100, 20, 16, 0), (1, 2048, 8, 256, 1)):
        rc, text = fs._describe(APPEND + "_describe", B, tq, mp, page, pow2)
        assert rc == len(text) < 2000 and text == m.describe_kv_append_paged_index_bf16_fp8(B, tq, mp, page, pow2)
        assert text.startswith("kv_append_paged_index_bf16_fp8_rows B=%d total_q=%d page=%d scale_pow2=%d: " % (B, tq, page, pow2))
        assert "%d workgroups of 256 threads (16 packed rows each" % (-(-tq // 16)) in text and ("power of two" in text) == bool(pow2)
        assert "a page is %d bytes" % (132 * page) in text and "at byte %d + 4 r" % (128 * page) in text and "four DPP moves" in text
    with pytest.raises(ValueError, match="status -2"):
        m.describe_mla_index_logits_paged_bf16_fp8(1, 1, 65, 320, 20, 16)
    with pytest.raises(ValueError, match="status -2"):
        m.describe_kv_append_paged_index_bf16_fp8(1, 1, 20, 48)
    with pytest.raises(ValueError, match="status -1"):
        m.describe_kv_append_paged_index_bf16_fp8(1, 1, 20, 16, 2)


# ---------------------------------------------------------------------------------------------------- the Python entries

def test_python_entries_refuse_bad_tensors_before_any_device_call(built, monkeypatch):
    """No GPU: the device check is replaced, and a call that gets as far as the C entry shows it by raising Reached."""
    from cuda_learn_notes_amd import host

    class Reached(Exception):
        pass

    def reached(name, argtypes):
        raise Reached(name)

    b = lambda *sh: torch.zeros(*sh, dtype=BF)  # noqa: E731
    f = lambda *sh: torch.zeros(*sh, dtype=torch.float32)  # noqa: E731
    i = lambda *sh: torch.zeros(*sh, dtype=torch.int32)  # noqa: E731
    u = lambda *sh: torch.zeros(*sh, dtype=U8)  # noqa: E731
    with pytest.raises(RuntimeError, match="expected a GPU"):
        built.mla_index_logits_paged_bf16_fp8(b(2, 3, 17, 128), f(2, 3, 17), u(5, 16, 132), i(2, 20), i(2), f(2, 3, 320))
    with pytest.raises(RuntimeError, match="expected a GPU"):
        built.kv_append_paged_index_bf16_fp8(b(7, 128), u(5, 16, 132), i(2, 20), i(2), i(3), True)
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)
    good = dict(q_idx=b(2, 3, 17, 128), weights=f(2, 3, 17), idx_pool=u(5, 16, 132), block_table=i(2, 20), seqlens=i(2), logits=f(2, 3, 320))
    lg = lambda **kw: built.mla_index_logits_paged_bf16_fp8(**{**good, **kw})  # noqa: E731
    for kw in (dict(q_idx=good["q_idx"].half()), dict(weights=good["weights"].double()), dict(idx_pool=b(5, 16, 132)),
               dict(idx_pool=torch.zeros(5, 16, 132, dtype=torch.int8)), dict(idx_pool=torch.zeros(5, 16, 132, dtype=torch.float8_e4m3fn)),
               dict(block_table=torch.zeros(2, 20, dtype=torch.int64)), dict(seqlens=torch.zeros(2, dtype=torch.int64)), dict(logits=good["logits"].half())):
        with pytest.raises(RuntimeError, match="values must be"):
            lg(**kw)
    with pytest.raises(RuntimeError, match="q_idx of 64 dims not supported"):
        lg(q_idx=b(2, 3, 17, 64))
    for kw in (dict(idx_pool=u(5, 16, 128)), dict(idx_pool=u(5, 16, 136)), dict(idx_pool=u(80, 132)), dict(idx_pool=u(5, 16 * 132)), dict(weights=f(2, 3, 16)),
               dict(seqlens=i(3)), dict(block_table=i(3, 20)), dict(logits=f(2, 2, 320)), dict(q_idx=b(6, 17, 128))):
        with pytest.raises(RuntimeError, match="size mismatch"):
            lg(**kw)
    with pytest.raises(RuntimeError, match="65 index heads not supported"):
        lg(q_idx=b(2, 3, 65, 128), weights=f(2, 3, 65))
    with pytest.raises(RuntimeError, match="page size 48"):
        lg(idx_pool=u(5, 48, 132))
    ap = lambda **kw: built.kv_append_paged_index_bf16_fp8(**{**dict(k_idx_new=b(7, 128), idx_pool=u(5, 16, 132), block_table=i(2, 20),  # noqa: E731
                                                                   seqlens=i(2), cu_q=i(3)), **kw})
    for kw in (dict(k_idx_new=b(7, 128).half()), dict(cu_q=torch.zeros(3, dtype=torch.int64)), dict(idx_pool=b(5, 16, 132)),
               dict(idx_pool=torch.zeros(5, 16, 132, dtype=torch.float8_e4m3fn))):
        with pytest.raises(RuntimeError, match="values must be"):
            ap(**kw)
    for kw in (dict(k_idx_new=b(7, 64)), dict(k_idx_new=b(7, 1, 128)), dict(idx_pool=u(5, 16, 128)), dict(idx_pool=u(5, 16, 576)), dict(seqlens=i(3)),
               dict(cu_q=i(2))):
        with pytest.raises(RuntimeError, match="size mismatch"):
            ap(**kw)
    with pytest.raises(RuntimeError, match="page size 48"):
        ap(idx_pool=u(5, 48, 132))
    monkeypatch.setattr(host, "_ext_fn", reached)  # a good call reaches the C entry
    for name, call in ((LOGITS, lg), (APPEND, ap), (APPEND, lambda: ap(scale_pow2=True))):
        with pytest.raises(Reached, match=name):
            call()


@pytest.mark.parametrize("page", [16, 256])
def test_index_pool_fp8_views_alias_the_storage_at_the_documented_offsets(built, page):
    P = 3
    pool = torch.zeros(P, page, 132, dtype=U8)
    codes, scales = built.index_pool_fp8_views(pool)
    assert codes.dtype == torch.float8_e4m3fn and tuple(codes.shape) == (P, page, 128) and scales.dtype == torch.float32 and tuple(scales.shape) == (P, page)
    base = pool.data_ptr()
    for p, r in ((0, 0), (1, 5), (2, page - 1)):
        assert codes[p, r].data_ptr() == base + p * 132 * page + 128 * r and codes[p, r, 127].data_ptr() == codes[p, r].data_ptr() + 127
        assert scales[p, r].data_ptr() == base + p * 132 * page + 128 * page + 4 * r
    codes.view(U8)[1, 5, 7] = 0x38  # 1.0
    scales[2, page - 1] = 0.5
    flat = pool.view(-1)
    assert int(flat[132 * page + 128 * 5 + 7]) == 0x38 and int(flat.sum()) == 0x38 + 0x3F  # 0.5f = 0x3F000000: one non-zero byte
    assert int(flat[2 * 132 * page + 128 * page + 4 * (page - 1) + 3]) == 0x3F
    rc, rs = x8.views(pool)  # the tests' own reading of the layout agrees
    assert rc.data_ptr() == codes.data_ptr() and rs.data_ptr() == scales.data_ptr() and torch.equal(rs, scales)
    for bad in (pool.view(torch.int8), pool[:, :, :128], torch.zeros(P, page, 128, dtype=U8), pool.view(-1)[4:4 + 2 * page * 132].view(2, page, 132)):
        with pytest.raises(RuntimeError):
            built.index_pool_fp8_views(bad)


# ---------------------------------------------------------------------------------------------------- the append reference against itself

def test_append_reference_scales_and_codes():
    g = torch.Generator().manual_seed(1)
    k = (torch.randn(4000, 128, generator=g) * 2.0 ** (torch.rand(4000, 1, generator=g) * 8 - 4)).to(BF)
    plain, p2 = x8.token_scales(k, False), x8.token_scales(k, True)
    assert plain.dtype == p2.dtype == torch.float32 and bool(((p2.view(torch.int32) & 0x007FFFFF) == 0).all())  # exact powers of two
    assert bool((p2 >= plain).all()) and bool((p2 < 2 * plain).all()) and bool((p2 > plain).any())
    assert float(plain.max() / plain.min()) > 100  # neighbouring tokens differ in scale
    for pow2 in (False, True):
        codes, s = x8.quantise_rows(k, pow2)
        deq = fk.dequantize(codes, s[:, None], torch.float64)
        err = (deq - k.double()).abs()
        bound = fk.bound(k.double(), s[:, None].double(), k.double().abs())
        assert bool((err <= bound).all()) and not bool(torch.isnan(codes.float()).any())
        top = codes.float().abs().amax(dim=-1)
        assert bool((top == 448).all()) if not pow2 else bool(((top >= 224) & (top <= 448)).all())  # the amax lands on 448, or in the binade below it
    sp = x8.special_rows()
    for pow2 in (False, True):
        codes, s = x8.quantise_rows(sp, pow2)
        floor = torch.tensor(1e-4, dtype=torch.float32) / torch.tensor(448.0, dtype=torch.float32)
        want_floor = x8.token_scales(torch.zeros(1, 128, dtype=BF), pow2)[0]
        assert float(want_floor) == (float(floor) if not pow2 else 2.0 ** -22) and 2.0 ** -23 < float(floor) < 2.0 ** -22
        assert float(s[0]) == float(s[1]) == float(want_floor) and bool((codes[0].view(U8) == 0).all())  # the all-zero key
        assert set(codes[1].view(U8).tolist()) == {0x00, 0x80}                                            # +-0 keep their signs
        assert float(s[4]) == 2.0 ** -3 and codes[4].float()[3] == 448 and codes[4].float()[4] == -56 and codes[4].float()[64] == 3.5  # already a power of two
        assert float(codes[2].float()[5]) == -448 and float(codes[3].float()[100]) == 448 and float(s[2]) == float(s[3]) == 2.0 ** -7  # 3.5 / 448 = 2^-7
        assert int(codes[2].view(U8)[7]) == 0x80 and int(codes[3].view(U8)[0]) == 0x80 and int(codes[2].view(U8)[6]) == 0
        assert float(s[5]) == float(want_floor)  # below the floor: the floor's scale


@pytest.mark.parametrize("page", x8.APPEND_PAGES)
@pytest.mark.parametrize("name", ix.APPEND_CASES)
def test_append_problems_are_the_edges_they_claim(name, page):
    p = x8.append_problem(name, page)
    P, bt, lens, cu, k_new, new = (p[k] for k in ("P", "bt", "lens", "cu", "k_new", "new"))
    c, Ts = ix.append_clamped(cu, k_new.shape[0])
    assert Ts == new and c[0] >= 0 and c[-1] <= k_new.shape[0]
    Nmax = bt.shape[1] * page
    start = x8.marked_pool(P, page)
    want = x8.append_ref(start, bt, lens, cu, k_new, True)
    codes, scales = x8.views(want)
    wrote_codes = (codes.view(U8) != x8.MARK_BYTE).any(dim=-1)
    wrote_scale = scales.view(torch.int32) != torch.tensor([x8.MARK_BYTE] * 4, dtype=U8).view(torch.int32)
    live = sum(1 for b, t in enumerate(Ts) for i in range(t) if 0 <= lens[b] - t + i < Nmax and 0 <= int(bt[b, (lens[b] - t + i) // page]) < P)
    assert int(wrote_scale.sum()) == live > 0 and bool((wrote_codes <= wrote_scale).all())
    dropped = sum(Ts) - live
    assert (dropped > 0) == (name in ("short_len", "past_nmax", "bad_entries")), (name, dropped)
    if name == "bad_entries":
        assert dropped == 14 and sorted(int(v) for v in bt.flatten() if not 0 <= int(v) < P) == [-1, P]
    assert bool((x8.token_scales(k_new, False).max() / x8.token_scales(k_new, False).min() > 4) or k_new.shape[0] < 4)


# ---------------------------------------------------------------------------------------------------- the parity cases bite

@pytest.mark.parametrize("name", sorted(x8.PARITY))
def test_the_parity_cases_bite(name):
    """For every parity case of tests/test_gpu_mla_index_fp8.py: a reference that drops the scale, takes slot r + 1's scale, takes the scale
    at the offset a page of another size would give, applies the ReLU after the head sum, or applies none, lies at least 20 x the bound
    from the reference at some visible position (a reading that is not finite there counts as far)."""
    q, w, (pool, bt), lens, ld = x8.parity_case(name)
    refs, bound, vis = x8.logits_ref(q, w, pool, bt, lens, ld, modes=x8.MODES)
    ref = refs["right"]
    fin = torch.isfinite(ref)
    assert int(fin.sum()) == sum(max(v, 0) for row in vis for v in row) > 0 and bool((bound[fin] > 0).all())
    assert torch.equal(torch.nan_to_num(ref, nan=-7.0), torch.nan_to_num(x8.reference(name)[0], nan=-7.0))
    for mode in x8.MODES[1:]:
        ratio = torch.nan_to_num((refs[mode][fin] - ref[fin]).abs() / bound[fin], nan=float("inf"))
        worst = float(ratio.max())
        print("mla index fp8 %s %s: largest |wrong - ref| / bound %.3g, %d of %d positions at 20 or more" % (name, mode, worst, int((ratio >= 20).sum()), int(fin.sum())))
        assert worst >= 20, (name, mode, worst)


def test_parity_cases_cover_what_the_issue_lists():
    cases = list(x8.PARITY.values())
    assert {c[1] for c in cases} >= {1, 16, 17, 33, 64} and {c[2] for c in cases} == {1, 3} and {c[3] for c in cases} == {16, 64, 256}
    assert set(x8.SMALL_LENS + x8.LONG_LENS) >= {1, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025} and max(x8.LONG_LENS) > 2048
    assert min(x8.LONG_LENS) < 0 and 0 in x8.SMALL_LENS[1:-1]
    lds = {(c[0], c[4]) for c in cases}
    assert ("small", 100) in lds and ("small", 513) in lds and ("small", 5002) in lds and ("small", None) in lds and any(c[4] and c[4] % 4 for c in cases)
    assert x8.LONG_NMAX % 256 == 0 and x8.SMALL_NMAX % 256 == 0


def test_exact_case_is_exact():
    for unit in (False, True):
        q, w, (pool, bt), lens, ld = x8.exact_case(64, 3, 16, unit)
        refs, bound, vis = x8.logits_ref(q, w, pool, bt, lens, ld)
        ref = refs["right"]
        fin = torch.isfinite(ref)
        codes, scales = x8.views(pool)
        live = torch.isfinite(scales)
        assert bool((scales[live].log2() % 1 == 0).all()) and float(scales[live].max()) == (1 if unit else 8) and float(scales[live].min()) == (1 if unit else 0.125)
        assert bool((codes[live].float() % 1 == 0).all()) and float(codes[live].float().abs().max()) == 8
        a = bound / (x8.EPS_TERMS * 2.0 ** -23)  # A = s sum_h |w_h| sum_d |q c|: above every partial sum
        assert 0 < float((a[fin] / 0.125).max()) < 2 ** 24  # in units of the smallest scale
        assert torch.equal(ref[fin], ref[fin].float().double())


# ---------------------------------------------------------------------------------------------------- the plan of the large pool

@pytest.mark.parametrize("n_live", [7, 30, 61, 344])
def test_large_pool_plan_names_both_sides_of_every_boundary_and_poisons_every_wrap_image(n_live):
    """tests/test_gpu_mla_index_fp8_large_pool.py: a page is 2112 bytes, no power of two, so the wrap images are listed directly. For every
    named page and every byte offset class inside it (the first and last byte of the code rows, of the scales, of the page), the offset
    taken mod 2^32 falls in a poison page or is the true offset; no named page is poison, a neighbour or an image of another."""
    P, PB = x8.large_pages(), x8.LARGE_PB
    plan = x8.large_plan(n_live, seed=n_live)
    named, poison, must = plan["named"], set(plan["poison"]), plan["must"]
    assert plan["P"] == P and P * PB + x8.LARGE_BASE <= x8.LARGE_BUF_BYTES and P * PB > 2 ** 33
    assert len(named) == len(set(named)) == n_live and not set(named) & poison and named[:7] == must and must[0] == P - 1
    assert set(range(x8.LARGE_LOW_PAGES)) <= poison and plan["dead"] in poison and all(x8.LARGE_LOW_PAGES <= n < P for n in named)
    for k, (b, above, below) in zip(x8.LARGE_BOUNDS, (must[1:4], must[4:7])):
        assert b * PB <= 2 ** k < (b + 1) * PB and above == b + 1 and below == b - 1  # the page that holds byte 2^k, one wholly above, one wholly below
        assert (below + 1) * PB <= 2 ** k <= above * PB
    wrapped = 0
    for n in named:
        assert all(m in poison or m in named for m in (n - 1, n + 1) if 0 <= m < P)
        for off in (0, 127, 128, PB - 4 * 16 - 1, 128 * 16, 128 * 16 + 4 * 15 + 3, PB - 1):
            true = n * PB + off
            image = true % 2 ** 32
            if image != true:
                wrapped += 1
                assert image // PB in poison and image // PB in x8.large_images(n), (n, off)
        assert all(m in poison for m in x8.large_images(n))
    assert wrapped > 7 * (n_live - 5)  # all but the three pages around 2^31 and the one below 2^32 wrap, the page that holds byte 2^32 in part
    assert x8.large_images(must[6]) == [] and x8.large_images(must[4]) == [0] and len(x8.large_images(P - 1)) == 2


# ---------------------------------------------------------------------------------------------------- registers and LDS

def test_kernel_resources_in_the_built_library(built, tmp_path):
    """No spill, no scratch; the four logits kernels take no LDS and fit two workgroups a CU (__launch_bounds__(256, 2): at most 256
    registers); the append kernel takes no LDS either."""
    got = si._built_kernels(tmp_path)
    logits = sorted((n, k) for n, k in got.items() if "mla_index_logits_paged_bf16_fp8_mfma" in n)
    append = [(n, k) for n, k in got.items() if "kv_append_paged_index_bf16_fp8_rows" in n]
    assert len(logits) == 4 and len(append) == 1, sorted(got)
    for n, k in logits + append:
        print(n, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
        assert k["group_segment_fixed_size"] == 0, (n, k)
    for nhb, (n, k) in enumerate(logits, 1):
        assert "ILi%dE" % nhb in n and k["vgpr_count"] <= 256, (n, k)
    assert append[0][1]["vgpr_count"] <= 64


def test_logits_kernel_loop(tmp_path):
    """The loop's MFMAs per wave and block of 16 keys: 4 k-steps per block of 16 heads, all bf16 16x16x32; the codes become bf16 by
    v_cvt_scalef32_pk_bf16_fp8, 16 of them a block; the keys come as dwordx4 loads; no LDS instruction at all."""
    got = fs._bodies("mla_index_logits_paged_bf16_fp8.hip", tmp_path)  # asserts no spill, no scratch, no atomics
    assert len(got) == 4, [k["name"] for k, _ in got]
    for k, body in got:
        nhb = int(re.search(r"mfmaILi(\d)E", k["name"]).group(1))
        print(k["name"], {x: k.get(x) for x in ("vgpr", "agpr", "sgpr", "lds")})
        assert fs._loop_mfmas(body) == 4 * nhb and k["lds"] == 0
        assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", "") and "ds_" not in body and "v_readlane_b32" in body
        assert body.count("v_cvt_scalef32_pk_bf16_fp8") == 16 and "global_load_dwordx4" in body


def test_append_kernel_body(tmp_path):
    """The row's amax by DPP moves inside the row: no LDS instruction (a ds_bpermute among them), no atomics; four fp8 conversions a thread."""
    got = fs._bodies("kv_append_paged_index_bf16_fp8.hip", tmp_path)
    assert len(got) == 1
    k, body = got[0]
    assert k["lds"] == 0 and "ds_" not in body and body.count("v_cvt_pk_fp8_f32") == 4
    assert all(s in body for s in ("quad_perm:[1,0,3,2]", "quad_perm:[2,3,0,1]", "row_half_mirror", "row_mirror"))
