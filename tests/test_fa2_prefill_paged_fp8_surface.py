"""CPU: the FP8 paged prefill attention entries (include/cln_amd_ext.h: cln_fa2_prefill_paged_fp8, cln_fa2_prefill_paged_fp8_describe;
csrc/flash_attn_prefill_paged_fp8.hip) -- header, exports, every status code before any device access (the scale pointers among them), the
describe text against its Python mirror (tests/fp8_paged_attn_reference.py), the Python entry's messages, the reference against brute force on
pools with a NaN-byte page, the all-codes problem of the GPU tests, and the kernels' code (MFMA on both products, the transposing LDS read, no
spill, no scratch, registers and LDS for two workgroups per CU). No GPU needed: hipcc cross-compiles."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cln_amd_ext.h")
CSRC = os.path.join(ROOT, "cuda-learn-notes_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "cuda-learn-notes_amd", "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_kv_reference as f8  # noqa: E402
import fp8_paged_attn_cases as cs  # noqa: E402
import fp8_paged_attn_reference as fr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402

NAMES = ("cln_fa2_prefill_paged_fp8", "cln_fa2_prefill_paged_fp8_describe")
LDS_PER_CU = 160 * 1024


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_both_prototypes(tmp_path, lang, cc):
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*a1)(const void*, const void*, const void*, const int*, const int*, const float*, const float*, void*, float*, int, int,"
                   " int, int, int, int, int, int, void*) = cln_fa2_prefill_paged_fp8;\n"
                   "int (*t1)(int, int, int, int, int, int, int, char*, int) = cln_fa2_prefill_paged_fp8_describe;\n"
                   "int main(void) { return a1 && t1 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _prefill():
    fn = _lib().cln_fa2_prefill_paged_fp8
    fn.argtypes = [ctypes.c_void_p] * 9 + [ctypes.c_int] * 8 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def _describe_fn():
    fn = _lib().cln_fa2_prefill_paged_fp8_describe
    fn.argtypes, fn.restype = [ctypes.c_int] * 7 + [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    return fn


def _describe(*dims):
    buf = ctypes.create_string_buffer(1280)
    rc = _describe_fn()(*dims, buf, 1280)
    return rc, buf.value.decode()


def test_product_library_and_package_export_the_entries(built):
    lib = _lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    from cuda_learn_notes_amd import host
    assert hasattr(built, "fa2_prefill_paged_fp8") and hasattr(host, "fa2_prefill_paged_fp8")
    assert hasattr(built.manifest, "describe_prefill_paged_fp8")
    names = {e.name for e in built.manifest.ENTRIES}
    for n in NAMES:
        assert n not in names and n.replace("cln_", "") not in names


# q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, o, lse: never dereferenced, every call below fails its checks first
PTR = [0x10000 * (i + 1) for i in range(9)]
DIMS = (2, 40, 8, 2, 40, 6, 16, 128)  # B, T, Hq, Hkv, P, max_pages, page, D
BAD_D = DIMS[:7] + (96,)              # the same with an unsupported D: what a call that passed every -1 check ends on


def test_prefill_checks_arguments_before_any_device_access(built):
    f = _prefill()
    p = list(PTR)
    assert f(*p, *BAD_D, None) == -2 and f(*p[:8], None, *BAD_D, None) == -2  # with and without lse
    for i in range(8):  # a null required pointer, the scales among them
        a = list(p)
        a[i] = None
        assert f(*a, *DIMS, None) == -1, i
    for i in (0, 1, 2, 7):  # 16-byte alignment
        a = list(p)
        a[i] = p[i] + 8
        assert f(*a, *DIMS, None) == -1, i
    for i in (3, 4, 5, 6, 8):  # block_table, seqlens, k_scale, v_scale, lse: 4-byte alignment, and no more than that
        a = list(p)
        a[i] = p[i] + 2
        assert f(*a, *DIMS, None) == -1, i
        a[i] = p[i] + 4
        assert f(*a, *BAD_D, None) == -2, i
    for out in (7, 8):  # an output equal to an input (a scale among them) or to the other output
        for src in range(9):
            if src != out:
                a = list(p)
                a[out] = p[src]
                assert f(*a, *DIMS, None) == -1, (out, src)
    for i in range(8):  # each dimension non-positive
        for bad in (0, -2):
            d = list(DIMS)
            d[i] = bad
            assert f(*p, *d, None) == -1, d
    assert f(*p, 2, 40, 8, 3, 40, 6, 16, 128, None) == -1  # Hq % Hkv
    for D in (32, 96, 256, 512):
        assert f(*p, *DIMS[:7], D, None) == -2, D
    for (Hq, Hkv) in ((3, 1), (6, 2), (16, 1), (5, 1)):  # G = 3, 3, 16, 5
        assert f(*p, 2, 40, Hq, Hkv, 40, 6, 16, 128, None) == -2, (Hq, Hkv)
    for page in (1, 8, 48, 100, 512):
        assert f(*p, 2, 40, 8, 2, 40, 6, page, 128, None) == -2, page
    assert f(*p, 2, 40, 8, 2, 40, 1 << 23, 256, 128, None) == -2  # max_pages page = 2^31
    assert f(*p, 1, 1 << 28, 8, 1, 40, 6, 16, 128, None) == -2  # T G = 2^31 rows of a KV head
    assert f(*p, 1 << 12, 1 << 19, 8, 8, 40, 6, 16, 64, None) == -2  # 2^15 pairs x 2^12 tiles: 2^27 workgroups of 256 threads
    assert f(*p, 2, 1 << 20, 8, 2, 40, 6, 16, 96, None) == -2 and _describe(2, 1 << 20, 8, 2, 6, 16, 128)[0] > 0  # any T


def test_describe_names_the_instantiation_and_matches_the_python_mirror(built):
    m = built.manifest
    for D in (64, 128):
        for G in pr.GROUPS:
            for page in pr.PAGES:
                for (B, T, Hkv, mp) in ((1, 1, 1, 1), (3, 19, 3, 3), (4, 512, 8, 64), (2, 4096, 2, 300), (256, 129, 2, 7)):
                    Hq = Hkv * G
                    rc, text = _describe(B, T, Hq, Hkv, mp, page, D)
                    assert rc == len(text) > 0, (rc, text)
                    assert text == m.describe_prefill_paged_fp8(B, T, Hq, Hkv, mp, page, D)
                    assert text == fr.describe_prefill_text(B, T, Hq, Hkv, mp, page, D)
                    assert text.startswith("fa2_prefill_paged_fp8<D=%d,G=%d> T=%d page=%d rows=%d keys=%d: one launch, no workspace"
                                           % (D, G, T, page, fr.ROW_TILE, fr.PREFILL_KEY_STEP)), text
                    assert text.endswith("deterministic") and "k_scale" in text and "v_scale" in text, text
                    assert "%d workgroups of 256 threads" % (B * Hkv * -(-T * G // fr.ROW_TILE)) in text, text
                    assert "v_mfma_f32_16x16x32_f16" in text and "ds_read_b64_tr_b16" in text
    rc, text = _describe(1, 1, 8, 2, 4, 16, 64)
    fn = _describe_fn()
    small = ctypes.create_string_buffer(b"\xff" * 24, 24)
    assert fn(1, 1, 8, 2, 4, 16, 64, small, 16) == 15 and small.raw[:16] == text[:15].encode() + b"\0" and small.raw[16:] == b"\xff" * 8
    assert fn(1, 1, 8, 2, 4, 16, 64, None, 16) == -1 and fn(1, 1, 8, 2, 4, 16, 64, small, 0) == -1
    for dims in ((1, 2, 8, 8, 4, 16, 96), (1, 2, 3, 1, 4, 16, 64), (1, 2, 8, 8, 4, 48, 64), (1, 2, 8, 3, 4, 16, 64), (0, 2, 8, 8, 4, 16, 64),
                 (1, 0, 8, 8, 4, 16, 64), (1, 2, 8, 8, 1 << 23, 256, 64), (1, 1 << 28, 8, 1, 4, 16, 64)):
        with pytest.raises(ValueError):
            m.describe_prefill_paged_fp8(*dims)


class _Fake:
    """What the Python entry looks at before it asks for a pointer: enough of a tensor to reach the checks under test without a GPU."""
    is_cuda = True

    def __init__(self, dtype, *shape):
        self.dtype, self.shape, self.device = dtype, torch.Size(shape), "cuda:0"

    def dim(self):
        return len(self.shape)


def test_error_messages_of_the_python_entry(built, monkeypatch):
    f = built.fa2_prefill_paged_fp8
    h, i32, f32 = torch.float16, torch.int32, torch.float32
    p8 = lambda *s: torch.zeros(*s, dtype=torch.uint8).view(f8.F8)  # noqa: E731
    q = torch.zeros(2, 40, 8, 64, dtype=h)
    rest = (torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), torch.ones(2), torch.ones(2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(q, p8(9, 2, 16, 64), p8(9, 2, 16, 64), *rest, q.clone())
    with pytest.raises(RuntimeError, match="values must be"):
        f(q.float(), p8(9, 2, 16, 64), p8(9, 2, 16, 64), *rest, q)
    from cuda_learn_notes_amd import host
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)

    def call(D=64, page=16, Hq=8, Hkv=2, T=40, pool=f8.F8, sdt=f32, ns=None, **bad):
        ns = Hkv if ns is None else ns
        a = dict(q=_Fake(h, 2, T, Hq, D), k=_Fake(pool, 9, Hkv, page, D), v=_Fake(pool, 9, Hkv, page, D), bt=_Fake(i32, 2, 4), sl=_Fake(i32, 2),
                 ks=_Fake(sdt, ns), vs=_Fake(sdt, ns), o=_Fake(h, 2, T, Hq, D))
        a.update(bad)
        f(a["q"], a["k"], a["v"], a["bt"], a["sl"], a["ks"], a["vs"], a["o"], a.get("lse"))
    for kw in (dict(pool=h), dict(pool=torch.float8_e4m3fnuz), dict(pool=torch.uint8), dict(sdt=torch.float64),
               dict(lse=_Fake(h, 2, 40, 8))):  # fp16 pools are the other entry's
        with pytest.raises(RuntimeError, match="values must be"):
            call(**kw)
    for kw in (dict(ns=1), dict(v=_Fake(f8.F8, 8, 2, 16, 64)), dict(o=_Fake(h, 2, 39, 8, 64)), dict(sl=_Fake(i32, 3)), dict(bt=_Fake(i32, 3, 4)),
               dict(lse=_Fake(f32, 2, 8)), dict(q=_Fake(h, 2, 8, 64)), dict(vs=_Fake(f32, 2, 1))):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            call(**kw)
    with pytest.raises(RuntimeError, match="fa2_prefill_paged_fp8: headdim 96 not supported"):
        call(D=96)
    with pytest.raises(RuntimeError, match=r"fa2_prefill_paged_fp8: group size 3 \(= Hq 6 / Hkv 2\) not supported"):
        call(Hq=6)
    with pytest.raises(RuntimeError, match="fa2_prefill_paged_fp8: page size 48 not supported"):
        call(page=48)
    with pytest.raises(RuntimeError, match="fa2_prefill_paged_fp8: 8 query heads are no multiple of 3 KV heads"):
        call(Hkv=3)
    with pytest.raises(RuntimeError, match="values must be"):  # FP8 pools to the fp16 entry
        built.fa2_prefill_paged(_Fake(h, 2, 40, 8, 64), _Fake(f8.F8, 9, 2, 16, 64), _Fake(f8.F8, 9, 2, 16, 64), _Fake(i32, 2, 4), _Fake(i32, 2),
                                _Fake(h, 2, 40, 8, 64))
    for T in (1, 9, 4096):  # a supported shape, whatever T is, gets as far as the pointers
        with pytest.raises(AttributeError, match="data_ptr"):
            call(T=T)


def test_reference_is_the_brute_force_masked_softmax_on_a_tiny_case_with_a_nan_page():
    g = torch.Generator().manual_seed(11)
    B, T, Hkv, G, page, mp, D = 3, 20, 2, 2, 16, 2, 64
    P = 7
    q = torch.randn(B, T, Hkv * G, D, generator=g).half()
    ks, vs = torch.tensor([0.011, 0.023]), torch.tensor([0.5, 0.017])
    kp, vp = (f8.quantize(torch.randn(P, Hkv, page, D, generator=g), f8.per_head(torch.full((Hkv,), 0.01))) for _ in range(2))
    kp, vp = f8.bits(kp).clone(), f8.bits(vp).clone()
    kp[0], vp[0] = f8.NAN_BYTE, f8.NAN_BYTE  # a page no entry names
    kp, vp = kp.view(f8.F8), vp.view(f8.F8)
    bt = torch.tensor([[5, 1], [3, 6], [2, 4]], dtype=torch.int32)
    lens = [2, 21, 99]  # fewer than T (right-aligned), a page and a bit, past the capacity (clamped to 32)
    O, L = fr.ref_prefill_paged_fp8(q, kp, vp, ks, vs, bt, lens)
    O2, L2 = fr.ref_decode_paged_multi_fp8(q[:, :8].contiguous(), kp, vp, ks, vs, bt, [n - 12 for n in [2 + 12, 21, 32]])
    assert bool(torch.isfinite(O).all())
    assert (O[1:, :8] - O2[1:]).abs().max().item() <= 1e-12  # the two references: query t of T = 8 at len - 12 is query t of T = 20 at len
    for b in range(B):
        n_b = min(lens[b], mp * page)
        for t in range(T):
            n = n_b - (T - 1 - t)
            for h in range(Hkv * G):
                if n <= 0:
                    assert bool((O[b, t, h] == 0).all()) and L[b, t, h].item() == float("-inf")
                    continue
                kv = h // G
                rows_k = torch.stack([kp[int(bt[b, j // page]), kv, j % page].float() for j in range(n)]).mul(ks[kv]).double()
                rows_v = torch.stack([vp[int(bt[b, j // page]), kv, j % page].float() for j in range(n)]).mul(vs[kv]).double()
                s = (rows_k @ q[b, t, h].double()) / D ** 0.5
                o1 = torch.softmax(s, dim=0) @ rows_v
                # the rows dequantised in fp32 as fp8_kv_reference.dequantize does; |O| reaches 0.5 x 448
                assert (O[b, t, h] - o1).abs().max().item() <= 1e-10 and abs(L[b, t, h].item() - torch.logsumexp(s, dim=0).item()) <= 1e-10


@pytest.mark.parametrize("D", [64, 128])
def test_all_codes_problem_selects_every_finite_byte_below_the_causal_edges(D):
    for (T, G) in ((70, 2), (8, 2)):  # the prefill and the multi-token GPU case
        k8, v8, ks, vs, want_v, score, cases = cs.all_codes_problem(D, T, G)
        assert len(cs.FINITE_CODES) == 254 and set(f8.bits(v8).flatten().tolist()) == set(cs.FINITE_CODES)
        assert bool(torch.isfinite(want_v.float()).all()) and score > 0
        for n, target, q in cases:
            assert q.shape == (1, T, G, D) and int(target[T - 1, 0]) == n - 1


def test_kernels_run_both_products_on_the_matrix_pipe_and_keep_registers(tmp_path):
    import kernel_resources as kr
    kernels, s = kr.report(os.path.join(CSRC, "flash_attn_prefill_paged_fp8.hip"), keep=str(tmp_path))
    assert len(kernels) == 2 and all("fa2pp::fa2_prefill_paged_fp8_mfma<" in k["demangled"] for k in kernels), [k["demangled"] for k in kernels]
    text = open(s).read()
    for k in kernels:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        assert 0 < 2 * k["lds"] <= LDS_PER_CU, k  # two workgroups resident per CU ...
        assert k["vgpr"] <= 256, k                # ... whose 8 waves, two per SIMD, share the 512 registers of a lane
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "v_mfma_f32_16x16x32_f16" in body and "ds_read_b64_tr_b16" in body and "global_load_dwordx2" in body, k["demangled"]
        assert "global_load_ubyte" not in body and "global_load_ushort" not in body, k  # no pool byte is loaded on its own
