"""CPU: the attention-sink entries of the bf16 sliding-window paged KV-cache path (include/cln_amd_ext.h:
cln_fa2_prefill_paged_varlen_window_sink_bf16, cln_fa2_decode_paged_multi_window_sink_bf16 with their plan / describe entries;
csrc/*_window_sink_bf16.{cuh,hip}) -- the fp64 reference of tests/paged_sink_reference.py against a literal transcription of HF's eager sink
attention, the sensitivity of the GPU cases to a dropped or double-counted sink, header, exports, the plan against the window sibling's, every
status code before any device access against the sibling's and then those of `sinks`, the describe texts, the Python errors, and the kernels'
resources. No GPU needed: hipcc cross-compiles."""
import ctypes
import itertools
import os
import re
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
import paged_bf16_reference as br  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import paged_sink_reference as sr  # noqa: E402
import paged_window_reference as wr  # noqa: E402

PREFILL, PREFILL_D = "cln_fa2_prefill_paged_varlen_window_sink_bf16", "cln_fa2_prefill_paged_varlen_window_sink_bf16_describe"
MULTI, MULTI_P, MULTI_D = ("cln_fa2_decode_paged_multi_window_sink_bf16", "cln_fa2_decode_paged_multi_window_sink_bf16_plan",
                           "cln_fa2_decode_paged_multi_window_sink_bf16_describe")
NAMES = (PREFILL, PREFILL_D, MULTI, MULTI_P, MULTI_D)
SIBLING = {n: n.replace("_window_sink_bf16", "_window_bf16") for n in NAMES}
LDS_PER_CU = 160 * 1024
INT_MAX = sr.INT_MAX
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------------- the reference

def hf_eager(q, k, v, hidden, sinks):
    """HF GptOssAttention's eager formulation, transcribed: q [H,T,D], k, v [H,N,D] (the KV heads already repeated), hidden [T,N] bool, sinks [H],
    all fp64. The sink column is concatenated to the scaled, masked logits, softmax, the column dropped, @ V. (HF subtracts the row maximum of the
    combined logits before the softmax, which changes nothing in exact arithmetic and is what torch.softmax does anyway.)"""
    H, T, D = q.shape
    attn_weights = torch.matmul(q, k.transpose(1, 2)) * D ** -0.5
    attn_weights = attn_weights.masked_fill(hidden[None], float("-inf"))
    combined_logits = torch.cat([attn_weights, sinks.reshape(H, 1, 1).expand(H, T, 1)], dim=-1)
    probs = torch.softmax(combined_logits, dim=-1)
    scores = probs[..., :-1]
    return torch.matmul(scores, v)


@pytest.mark.parametrize("W", [1, 5, 40, None])
def test_reference_is_hf_eager_sink_attention(W):
    """Random small inputs, Hq 4 over Hkv 2, T = 6 new tokens of a sequence of 37 keys: 1e-12 relative, the rows that see no key excluded (there
    are none here: every token sees itself)."""
    T, Hq, Hkv, D, n, page = 6, 4, 2, 64, 37, 16
    g = torch.Generator().manual_seed(5 if W is None else W)
    q = torch.randn(1, T, Hq, D, generator=g).to(BF)
    k, v = (torch.randn(1, Hkv, 48, D, generator=g).to(BF) for _ in range(2))
    sinks = torch.randn(Hq, generator=g) * 2
    kp, vp, bt = pr.make_pool(k, v, page, [n])
    vis = torch.tensor([n - (T - 1 - t) for t in range(T)])
    j = torch.arange(n)[None, :]
    hidden = (j >= vis[:, None]) | (j < (vis - (INT_MAX if W is None else W)).clamp(min=0)[:, None])
    kd, vd = (t[0, :, :n].double().repeat_interleave(Hq // Hkv, dim=0) for t in (k, v))
    want = hf_eager(q[0].double().transpose(0, 1), kd, vd, hidden, sinks.double()).transpose(0, 1)
    for got in (sr.decode(q, kp, vp, bt, [n], W, sinks)[0][0], sr.prefill(q[0], kp, vp, bt, [n], [0, T], W, sinks)[0]):
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # and the LSE is the log of the denominator that was used
    lse = sr.decode(q, kp, vp, bt, [n], W, sinks)[1][0]
    s = (torch.einsum("thd,hnd->htn", q[0].double(), kd) * D ** -0.5).masked_fill(hidden[None], float("-inf"))
    den = torch.exp(s).sum(-1) + torch.exp(sinks.double())[:, None]
    assert float((lse - torch.log(den).T).abs().max()) <= 1e-12 * float(lse.abs().max())


def _wrong_by(ref, bound, *args, **kw):
    """min over count in (0, 2) of max|O_count - O| / bound."""
    fn = args[0]
    out = []
    for count in (0, 2):
        o = fn(*args[1:], count=count, **kw)[0]
        fin = torch.isfinite(ref)
        out.append(float((o[fin] - ref[fin]).abs().max()) / bound)
    return min(out)


def test_the_sensitive_gpu_cases_would_notice_a_dropped_or_a_double_counted_sink():
    """Every several-splits decode case and every prefill case of tests/test_gpu_paged_sink_attention.py with its mixed sink set: the reference
    with the sink counted zero times and counted twice is further than 4 x the case's o_bound from the right one."""
    worst = float("inf")
    for T, G, D in itertools.product(sr.DECODE_T, sr.DECODE_G, (64, 128)):
        for n, W in itertools.product([x for x in sr.DECODE_LENS if x > 0], sr.SPLIT_WINDOWS):
            if (T, G) not in ((1, 1), (3, 4), (8, 8)) and n != 4096:  # the other shapes at the longest length only: the arithmetic is the same
                continue
            q, lens, pool = sr.decode_split_case(T, G, D, n)
            sinks = sr.decode_split_sinks(G, n, W)
            ro, _, emul = sr.decode(q, *pool, lens, W, sinks)
            r = _wrong_by(ro, br.o_bound(emul, ro), sr.decode, q, *pool, lens, W, sinks)
            assert r > 4, ("decode", T, G, D, n, W, r)
            worst = min(worst, r)
    for D, (Hq, Hkv), page, W in itertools.product((64, 128), sr.PREFILL_HEADS, sr.PREFILL_PAGES, sr.PREFILL_WINDOWS):
        qs, lens, pool = sr.prefill_case(D, Hq, Hkv, page)
        q, cu = sr.pack(qs)
        sinks = sr.prefill_sinks(Hq, W)
        ro, _, emul = sr.prefill(q, *pool, lens, cu, W, sinks)
        r = _wrong_by(ro, br.o_bound(emul, ro), sr.prefill, q, *pool, lens, cu, W, sinks)
        assert r > 4, ("prefill", D, Hq, Hkv, page, W, r)
        worst = min(worst, r)
    print("smallest wrong / bound: %.1f" % worst)


def test_reference_rows_without_a_key_stay_rows_without_a_key_and_minus_inf_sinks_are_the_window_reference():
    D, Hq, Hkv, page = 64, 8, 2, 16
    qs, lens, pool = sr.prefill_case(D, Hq, Hkv, page)
    q, cu = sr.pack(qs)
    o, lse, emul = sr.prefill(q, *pool, lens, cu, 65, sr.sinks_const(Hq, 3.0))
    dead = slice(cu[4], cu[4] + 2)  # len 2 < T 4: the first two tokens
    assert bool((o[dead] == 0).all()) and bool((lse[dead] == float("-inf")).all()) and bool((emul[dead] == 0).all())
    assert bool(torch.isfinite(lse[cu[4] + 2:cu[5]]).all())
    for value in (float("-inf"), -1e30):
        got = sr.prefill(q, *pool, lens, cu, 65, sr.sinks_const(Hq, value))
        want = wr.prefill(q, *pool, lens, cu, 65)
        for a, b in zip(got, want):
            assert torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
    o, lse, emul = sr.prefill(q, *pool, lens, cu, 65, sr.sinks_const(Hq, 1e30))
    live = torch.isfinite(lse)
    assert bool((o[live] == 0).all()) and bool((emul[live] == 0).all()) and bool((lse[live] == float(torch.tensor(1e30))).all())  # the fp32 the sinks hold


# ---------------------------------------------------------------------------------------------------- header, exports, plan

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_five_prototypes(tmp_path, lang, cc):
    """The window siblings' argument lists with `const float* sinks` as the last input pointer."""
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*a1)(const void*, const void*, const void*, const int*, const int*, const int*, const float*, void*, float*, int, int, int,"
                   " int, int, int, int, int, int, void*) = %s;\n"
                   "int (*t1)(int, int, int, int, int, int, int, int, char*, int) = %s;\n"
                   "int (*a3)(const void*, const void*, const void*, const int*, const int*, const float*, void*, float*, void*, long long, int, int,"
                   " int, int, int, int, int, int, int, void*) = %s;\n"
                   "int (*p3)(int, int, int, int, int, int, int, int, int*, int*, long long*) = %s;\n"
                   "int (*t3)(int, int, int, int, int, int, int, int, char*, int) = %s;\n"
                   "int main(void) { return a1 && t1 && a3 && p3 && t3 ? 0 : 1; }\n" % NAMES)
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _fn(name, argtypes):
    fn = getattr(_lib(), name)
    fn.argtypes, fn.restype = argtypes, ctypes.c_int
    return fn


def _prefill(sink):
    return _fn(PREFILL if sink else SIBLING[PREFILL], [ctypes.c_void_p] * (8 + sink) + [ctypes.c_int] * 9 + [ctypes.c_void_p])


def _multi(sink):
    return _fn(MULTI if sink else SIBLING[MULTI], [ctypes.c_void_p] * (8 + sink) + [ctypes.c_longlong] + [ctypes.c_int] * 9 + [ctypes.c_void_p])


def _plan(name, *dims):
    fn = _fn(name, [ctypes.c_int] * len(dims) + [ctypes.c_void_p] * 3)
    s, c, w = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
    rc = fn(*dims, ctypes.addressof(s), ctypes.addressof(c), ctypes.addressof(w))
    return rc, (s.value, c.value, w.value)


def _describe(name, *dims):
    fn = _fn(name, [ctypes.c_int] * len(dims) + [ctypes.c_char_p, ctypes.c_int])
    buf = ctypes.create_string_buffer(4096)
    rc = fn(*dims, buf, 4096)
    return rc, buf.value.decode()


def test_library_header_and_package_hold_the_entries(built):
    lib, hdr = _lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in ("fa2_prefill_paged_varlen_window_sink_bf16", "fa2_decode_paged_multi_window_sink_bf16", "fa2_decode_paged_multi_window_sink_bf16_plan"):
        assert hasattr(built, n) and hasattr(host, n), n
    for n in ("describe_prefill_paged_varlen_window_sink_bf16", "describe_decode_paged_multi_window_sink_bf16"):
        assert hasattr(built.manifest, n), n
    names = {e.name for e in built.manifest.ENTRIES}
    for n in NAMES:  # none of the new names is a manifest name
        assert n not in names and n.replace("cln_", "") not in names


def test_plan_is_the_window_siblings_plan(built):
    n = split = 0
    for B, T, (Hq, Hkv), (mp, page), D, W in itertools.product((1, 5, 64), (1, 3, 8), ((1, 1), (8, 1), (64, 8)),
                                                               ((19, 16), (256, 16), (1024, 16), (64, 256)), (64, 128),
                                                               (1, 33, 128, 1000, 4096, 1 << 20, INT_MAX)):
        got = _plan(MULTI_P, B, T, Hq, Hkv, mp, page, D, W)
        assert got[0] == 0 and got == _plan(SIBLING[MULTI_P], B, T, Hq, Hkv, mp, page, D, W), (B, T, Hq, Hkv, mp, page, D, W)
        assert got[1] == wr.plan(B, T, Hq, Hkv, mp, page, D, W) == built.fa2_decode_paged_multi_window_sink_bf16_plan(B, T, Hq, Hkv, mp, page, D, W)
        n += 1
        split += got[1][0] > 1
    assert n > 1000 and split > 100
    for B, T, Hq, Hkv, mp, page, D in ((1, 1, 8, 1, 1024, 16, 64), (5, 8, 64, 8, 256, 16, 128)):  # window = None: no window
        assert (built.fa2_decode_paged_multi_window_sink_bf16_plan(B, T, Hq, Hkv, mp, page, D, None)
                == built.fa2_decode_paged_multi_window_bf16_plan(B, T, Hq, Hkv, mp, page, D, INT_MAX)
                == built.fa2_decode_paged_multi_bf16_plan(B, T, Hq, Hkv, mp, page, D))
    for dims in ((0, 2, 8, 8, 4, 16, 64), (1, 9, 8, 8, 4, 16, 64), (1, 2, 8, 3, 4, 16, 64), (1, 2, 8, 8, 4, 16, 96), (1, 2, 8, 8, 4, 48, 64)):
        for W in (5, 0):
            assert _plan(MULTI_P, *dims, W) == _plan(SIBLING[MULTI_P], *dims, W)
            for name in (PREFILL_D, MULTI_D):
                a, b = _describe(name, *dims, W)[0], _describe(SIBLING[name], *dims, W)[0]
                assert min(a, 0) == min(b, 0) and (a < 0 or name == PREFILL_D), (name, dims, W, a, b)  # T = 9 is a total_q the prefill takes


# ---------------------------------------------------------------------------------------------------- status codes

# q, k_pages, v_pages, block_table, seqlens, cu_q, o, lse | sinks: never dereferenced, every call below fails its checks first
PTR = [0x10000 * (i + 1) for i in range(8)]
SINKS = 0x10000 * 20
DIMS = (3, 170, 8, 2, 40, 6, 16, 128)  # B, total_q, Hq, Hkv, P, max_pages, page, D
BAD_D = DIMS[:7] + (96,)


def test_prefill_statuses_are_the_siblings_then_those_of_sinks(built):
    f, g = _prefill(1), _prefill(0)
    p = list(PTR)

    def both(ptrs, dims, want, W=5):
        a, b = f(*ptrs[:6], SINKS, *ptrs[6:], *dims, W, None), g(*ptrs, *dims, W, None)
        assert a == b == want, (ptrs, dims, a, b)
    both(p, BAD_D, -2)
    both(p[:7] + [None], BAD_D, -2)
    for i in range(7):  # a null required pointer
        a = list(p)
        a[i] = None
        both(a, DIMS, -1)
    for i, off in ((0, 8), (1, 8), (2, 8), (6, 8), (3, 2), (4, 2), (5, 2), (7, 2)):
        a = list(p)
        a[i] = p[i] + off
        both(a, DIMS, -1)
    for out in (6, 7):  # an output equal to an input or to the other output
        for src in range(8):
            if src != out:
                a = list(p)
                a[out] = p[src]
                both(a, DIMS, -1)
    for i in range(8):  # each dimension non-positive
        d = list(DIMS)
        d[i] = 0
        both(p, d, -1)
    both(p, (3, 170, 8, 3, 40, 6, 16, 128), -1)  # Hq % Hkv
    for d in ((3, 170, 6, 2, 40, 6, 16, 128), (3, 170, 8, 2, 40, 6, 48, 128), (3, 170, 8, 2, 40, 1 << 23, 256, 128), (1, 1 << 28, 8, 1, 40, 6, 16, 128)):
        both(p, d, -2)
    for W in (0, -1, -INT_MAX - 1):
        both(p, DIMS, -1, W)
        both(p, BAD_D, -2, W)
    # sinks: null, at an odd address, equal to an output -- -1, and before the shape as for seqlens: an unsupported D does not turn it into -2
    for dims in (DIMS, BAD_D):
        assert f(*p[:6], None, *p[6:], *dims, 5, None) == -1
        assert f(*p[:6], SINKS + 1, *p[6:], *dims, 5, None) == -1 and f(*p[:6], SINKS + 2, *p[6:], *dims, 5, None) == -1
        assert f(*p[:6], p[6], *p[6:], *dims, 5, None) == -1 and f(*p[:6], p[7], *p[6:], *dims, 5, None) == -1
        a = list(p)
        a[4] = None  # what a bad seqlens gives there
        assert g(*a, *dims, 5, None) == -1
    assert f(*p[:6], SINKS + 4, *p[6:], *BAD_D, 5, None) == -2  # 4-byte alignment is enough: the shape is looked at


MPTR = [0x10000 * (i + 1) for i in range(8)]  # q, k_pages, v_pages, block_table, seqlens, o, lse, workspace
MDIMS = (3, 4, 8, 2, 40, 6, 16, 128)          # B, T, Hq, Hkv, P, max_pages, page, D: one split, no workspace needed
MBAD_D = MDIMS[:7] + (96,)
WS = 1 << 30


def test_multi_statuses_are_the_siblings_then_those_of_sinks(built):
    f, g = _multi(1), _multi(0)
    p = list(MPTR)

    def both(ptrs, ws, dims, want, W=5):
        a, b = f(*ptrs[:5], SINKS, *ptrs[5:], ws, *dims, W, None), g(*ptrs, ws, *dims, W, None)
        assert a == b == want, (ptrs, dims, a, b)
    both(p, WS, MBAD_D, -2)
    both(p[:6] + [None, None], 0, MBAD_D, -2)
    for i in range(6):
        a = list(p)
        a[i] = None
        both(a, WS, MDIMS, -1)
    for i, off in ((0, 8), (1, 8), (2, 8), (5, 8), (6, 8), (7, 8), (3, 2), (4, 2)):
        a = list(p)
        a[i] = p[i] + off
        both(a, WS, MDIMS, -1)
    for out in (5, 6, 7):
        for src in range(8):
            if src != out:
                a = list(p)
                a[out] = p[src]
                both(a, WS, MDIMS, -1)
    for i in range(8):
        d = list(MDIMS)
        d[i] = 0
        both(p, WS, d, -1)
    both(p, WS, (3, 4, 8, 3, 40, 6, 16, 128), -1)
    for d in ((3, 9, 8, 2, 40, 6, 16, 128), (3, 4, 6, 2, 40, 6, 16, 128), (3, 4, 8, 2, 40, 6, 48, 128), (3, 4, 8, 2, 40, 1 << 23, 256, 128)):
        both(p, WS, d, -2)
    for W in (0, -1, -INT_MAX - 1):
        both(p, WS, MDIMS, -1, W)
        both(p, WS, MBAD_D, -2, W)
    split = (1, 2, 4, 1, 40, 256, 16, 128)  # max_pages page = 4096 and W = 1000: 3 splits, the workspace is required, and large enough
    rc, (S, C, need) = _plan(MULTI_P, *split[:4], *split[5:], 1000)
    assert rc == 0 and (S, C) == (3, 384) and need == 1 * 2 * 4 * 3 * 130 * 4
    assert f(*p[:5], SINKS, *p[5:7], None, 0, *split, 1000, None) == -1 and f(*p[:5], SINKS, *p[5:], need - 1, *split, 1000, None) == -1
    for dims in (MDIMS, MBAD_D):  # sinks: null, at an odd address, equal to o, lse or the workspace
        assert f(*p[:5], None, *p[5:], WS, *dims, 5, None) == -1
        assert f(*p[:5], SINKS + 1, *p[5:], WS, *dims, 5, None) == -1 and f(*p[:5], SINKS + 2, *p[5:], WS, *dims, 5, None) == -1
        for out in (5, 6, 7):
            assert f(*p[:5], p[out], *p[5:], WS, *dims, 5, None) == -1
        a = list(p)
        a[4] = None
        assert g(*a, WS, *dims, 5, None) == -1
    assert f(*p[:5], SINKS + 4, *p[5:], WS, *MBAD_D, 5, None) == -2


# ---------------------------------------------------------------------------------------------------- describe, Python errors

def test_describe_texts_match_the_python_mirrors(built):
    m = built.manifest
    splits = set()
    for D, G, page, W in itertools.product((64, 128), pr.GROUPS, (16, 64, 256), (1, 128, 1024, INT_MAX)):
        for (B, tq, Hkv, mp) in ((1, 1, 1, 1), (5, 204, 1, 32), (65, 2112, 8, 300)):
            Hq = Hkv * G
            rc, text = _describe(PREFILL_D, B, tq, Hq, Hkv, mp, page, D, W)
            assert rc == len(text) > 0, (rc, text)
            assert text == m.describe_prefill_paged_varlen_window_sink_bf16(B, tq, Hq, Hkv, mp, page, D, W)
            assert text == sr.describe_prefill_text(B, tq, Hq, Hkv, mp, page, D, W)
            assert text.startswith("fa2_prefill_paged_varlen_window_sink_bf16_mfma<D=%d,G=%d> B=%d" % (D, G, B)) and "in the epilogue" in text
        for (B, T, Hkv, mp) in ((1, 1, 1, 256), (7, 3, 2, 19), (64, 8, 8, 300), (1, 8, 1, 4096)):
            Hq = Hkv * G
            rc, text = _describe(MULTI_D, B, T, Hq, Hkv, mp, page, D, W)
            assert rc == len(text) > 0, (rc, text)
            assert text == m.describe_decode_paged_multi_window_sink_bf16(B, T, Hq, Hkv, mp, page, D, W)
            assert text == sr.describe_multi_text(B, T, Hq, Hkv, mp, page, D, W)
            S = wr.plan(B, T, Hq, Hkv, mp, page, D, W)[0]
            splits.add(S > 1)
            assert text.startswith("fa2_decode_paged_multi_window_sink_bf16_mfma<D=%d,MT=%d> T=%d G=%d W=%d " % (D, -(-T * G // 16), T, G, W))
            assert ("fa2_decode_combine_window_sink_bf16_rows<D=%d>" % D in text) == (S > 1) == ("into the merged fp32" in text)
            assert ("at its final store" in text) == (S == 1)
    assert splits == {False, True}
    for name, dims in ((PREFILL_D, (1, 1, 8, 2, 4, 16, 64, 9)), (MULTI_D, (1, 1, 8, 2, 4, 16, 64, 9))):
        rc, text = _describe(name, *dims)
        f = getattr(_lib(), name)
        small = ctypes.create_string_buffer(b"\xff" * 24, 24)
        assert f(*dims, small, 16) == 15 and small.raw[:16] == text[:15].encode() + b"\0" and small.raw[16:] == b"\xff" * 8
        assert f(*dims, None, 16) == -1 and f(*dims, small, 0) == -1
    with pytest.raises(ValueError):
        m.describe_prefill_paged_varlen_window_sink_bf16(3, 8, 8, 2, 40, 16, 128, 0)
    with pytest.raises(ValueError):
        m.describe_decode_paged_multi_window_sink_bf16(1, 9, 8, 8, 4, 16, 64, 5)


def test_python_entries_refuse_bad_sinks_before_any_device_call_and_forward_no_window(built, monkeypatch):
    from cuda_learn_notes_amd import host
    i32 = torch.int32
    ints = (torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), torch.zeros(3, dtype=i32))
    b = lambda *s: torch.zeros(*s, dtype=BF)  # noqa: E731
    pre = lambda W, sinks: built.fa2_prefill_paged_varlen_window_sink_bf16(  # noqa: E731
        b(40, 8, 64), b(9, 2, 16, 64), b(9, 2, 16, 64), *ints, W, sinks, b(40, 8, 64))
    dec = lambda W, sinks: built.fa2_decode_paged_multi_window_sink_bf16(  # noqa: E731
        b(2, 3, 8, 64), b(9, 2, 16, 64), b(9, 2, 16, 64), *ints[:2], W, sinks, b(2, 3, 8, 64))
    good = torch.zeros(8)
    for call in (pre, dec):
        for bad, text in ((torch.zeros(8, dtype=torch.float16), r"^values must be torch::kFloat32$"),
                          (torch.zeros(8, dtype=BF), r"^values must be torch::kFloat32$"),
                          (torch.zeros(9), r"^Tensor size mismatch!$"), (torch.zeros(1, 8), r"^Tensor size mismatch!$"),
                          (torch.zeros(16)[::2], r"^tensor must be contiguous")):
            with pytest.raises(RuntimeError, match=text):
                call(5, bad)
        with pytest.raises(RuntimeError, match="no CPU path"):  # sinks -- like every tensor here -- on the CPU
            call(5, good)
        for W in (0, -3):
            with pytest.raises(RuntimeError, match=r"window %d not supported \(>= 1\)" % W):
                call(W, good)
    with pytest.raises(RuntimeError, match=r"fa2_decode_paged_multi_window_sink_bf16: window 0 not supported"):
        built.fa2_decode_paged_multi_window_sink_bf16_plan(2, 3, 8, 2, 4, 16, 64, 0)
    with pytest.raises(RuntimeError, match=r"fa2_decode_paged_multi_window_sink_bf16: T 9 not supported"):
        built.fa2_decode_paged_multi_window_sink_bf16_plan(1, 9, 8, 2, 4, 16, 64, None)
    # window = None reaches the C entries as 2^31 - 1, and sinks as the last input pointer: the device checks are switched off, the C entry is
    # replaced by a recorder
    seen = []
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)
    monkeypatch.setattr(host, "_stream", lambda: None)
    monkeypatch.setattr(host, "_lse_fns", {"cln_" + n: (lambda n: lambda *a: seen.append((n, a)) or 0)(n)
                                           for n in ("fa2_prefill_paged_varlen_window_sink_bf16", "fa2_decode_paged_multi_window_sink_bf16")})
    sinks = torch.zeros(8)
    pre(None, sinks)
    dec(None, sinks)
    pre(77, sinks)
    (n0, a0), (n1, a1), (n2, a2) = seen
    assert n0 == n2 == "fa2_prefill_paged_varlen_window_sink_bf16" and n1 == "fa2_decode_paged_multi_window_sink_bf16"
    assert a0[-2] == INT_MAX and a1[-2] == INT_MAX and a2[-2] == 77
    assert a0[6] == sinks.data_ptr() and a1[5] == sinks.data_ptr()  # behind cu_q / behind seqlens
    assert len(a0) == 19 and len(a1) == 20


# ---------------------------------------------------------------------------------------------------- registers

def _bodies(src, tmp_path):
    import kernel_resources as kres
    kernels, s = kres.report(os.path.join(CSRC, src), keep=str(tmp_path))
    text = open(s).read()
    out = []
    for k in kernels:
        body = text[text.index("\n" + k["name"] + ":"):]
        out.append((k, body[:body.index(".Lfunc_end")]))
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        assert not k["name"].endswith("_kernel") and "_kernelI" not in k["name"], k["name"]
        assert "_f16" not in body and "atomic" not in body, k["name"]  # no fp16 MFMA, no conversion through fp16
    return out


def test_prefill_kernels_keep_two_workgroups_per_cu_without_spill_or_scratch(tmp_path):
    got = _bodies("flash_attn_prefill_paged_varlen_window_sink_bf16.hip", tmp_path)
    assert len(got) == 2 and all("fa2_prefill_paged_varlen_window_sink_bf16_mfma" in k["name"] for k, _ in got), [k["name"] for k, _ in got]
    for k, body in got:
        print(k["name"], {x: k[x] for x in ("vgpr", "sgpr", "lds")})
        D = 128 if k["lds"] > 30000 else 64
        assert 0 < 2 * k["lds"] <= LDS_PER_CU and k["vgpr"] <= 256, k  # two workgroups per CU, two waves per SIMD
        assert body.count("v_mfma_f32_16x16x32_bf16") == D // 2 and "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body, k["name"]


def test_multi_kernels_and_the_sink_combine_without_spill_or_scratch(tmp_path):
    got = _bodies("flash_attn_decode_paged_multi_window_sink_bf16.hip", tmp_path)
    stream = [(k, b) for k, b in got if "fa2_decode_paged_multi_window_sink_bf16_mfma" in k["name"]]
    combine = [(k, b) for k, b in got if "fa2_decode_combine_window_sink_bf16_rows" in k["name"]]
    assert len(stream) == 8 and len(combine) == 2 and len(got) == 10, [k["name"] for k, _ in got]
    for k, body in stream:
        print(k["name"], {x: k[x] for x in ("vgpr", "sgpr", "lds")})
        assert "v_mfma_f32_16x16x32_bf16" in body and "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body, k["name"]
        assert k["vgpr"] <= 512, k
    for k, body in combine:
        assert "v_cvt_pk_bf16_f32" in body and "global_store_short" in body and "v_mfma" not in body, k["name"]
