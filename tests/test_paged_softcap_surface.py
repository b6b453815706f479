"""CPU: the paged bf16 attention entries with a softmax scale and logit soft-capping (include/cln_amd_ext.h:
cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16[_fp8], cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16[_fp8] with their plan /
describe entries; csrc/*_softcap_anyg_*.{cuh,hip}, csrc/paged_softcap.cuh) -- header, exports and package, the plan against the
any-G entries', the status of the two floats, the describe texts, the kernels' resources and MFMA counts against the any-G kernels', the fp64
reference against a dense computation written out, and the sensitivity of the GPU cases to the six defects of paged_softcap_reference. No GPU
needed: hipcc cross-compiles."""
import ctypes
import itertools
import math
import os
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cln_amd_ext.h")
sys.path.insert(0, os.path.join(ROOT, "cuda-learn-notes_amd", "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paged_anyg_cases as ac  # noqa: E402
import paged_bf16_reference as br  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import paged_sink_reference as sr  # noqa: E402
import paged_softcap_reference as cr  # noqa: E402
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the sibling surface test's readers of a code object)

PRE, PRE8 = "cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16", "cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8"
DEC, DEC8 = "cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16", "cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8"
NAMES = (PRE, PRE + "_describe", DEC, DEC + "_plan", DEC + "_describe", PRE8, PRE8 + "_describe", DEC8, DEC8 + "_plan", DEC8 + "_describe")
ANYG = lambda n: n.replace("_softcap_", "_")  # noqa: E731
INT_MAX = sr.INT_MAX
NAN, INF = float("nan"), float("inf")
BAD = (-1.0, NAN, INF, -INF, -1e-30)
_fn, _plan = fs._fn, fs._plan


def _describe(name, *dims, scale=0.0, cap=0.0):
    fn = _fn(name, [ctypes.c_int] * len(dims) + [ctypes.c_float] * 2 + [ctypes.c_char_p, ctypes.c_int])
    buf = ctypes.create_string_buffer(4096)
    rc = fn(*dims, scale, cap, buf, 4096)
    return rc, buf.value.decode()


# ---------------------------------------------------------------------------------------------------- header, exports

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_ten_prototypes(tmp_path, lang, cc):
    assert shutil.which(cc), cc
    pre = ("const void*, const void*, const void*, const int*, const int*, const int*, %sconst float*, void*, float*, " + "int, " * 9
           + "float, float, void*")
    dec = ("const void*, const void*, const void*, const int*, const int*, %sconst float*, void*, float*, void*, long long, " + "int, " * 9
           + "float, float, void*")
    text, plan = "int, int, int, int, int, int, int, int, float, float, char*, int", "int, int, int, int, int, int, int, int, int*, int*, long long*"
    protos = (pre % "", text, dec % "", plan, text, pre % "const float*, const float*, ", text, dec % "const float*, const float*, ", plan, text)
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n' + "".join("int (*f%d)(%s) = %s;\n" % (i, p, n) for i, (p, n) in enumerate(zip(protos, NAMES)))
                   + "int main(void) { return f0 && f9 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_header_manifest_and_package_hold_the_entries(built):
    lib, hdr = fs._lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in (PRE, DEC, DEC + "_plan", PRE8, DEC8, DEC8 + "_plan"):
        assert hasattr(built, n[4:]) and hasattr(host, n[4:]), n
    for n in (PRE, DEC, PRE8, DEC8):
        assert hasattr(built.manifest, "describe_" + n[len("cln_fa2_"):]), n
    build = open(os.path.join(ROOT, "cuda-learn-notes_amd", "_build.py")).read()
    for k, t in itertools.product(("prefill_paged_varlen", "decode_paged_multi"), ("bf16", "bf16_fp8")):
        assert '"flash_attn_%s_window_sink_softcap_anyg_%s.hip"' % (k, t) in build


# ---------------------------------------------------------------------------------------------------- plan

def test_plan_is_the_any_g_plan_status_included(built):
    n = split = 0
    for B, (T, G), Hkv, (mp, page), D, W in itertools.product((1, 5, 64), ((1, 1), (3, 4), (8, 8), (1, 3), (3, 5), (8, 7), (5, 12), (4, 16)), (1, 2, 8),
                                                              ((19, 16), (256, 16), (1024, 16), (64, 256)), (64, 128),
                                                              (1, 33, 1000, 4096, INT_MAX)):
        Hq = G * Hkv
        want = _plan(ANYG(DEC) + "_plan", B, T, Hq, Hkv, mp, page, D, W)
        assert want[0] == 0
        for name in (DEC, DEC8):
            assert _plan(name + "_plan", B, T, Hq, Hkv, mp, page, D, W) == want, (name, B, T, Hq, Hkv, mp, page, D, W)
        py = (built.fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan, built.fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan)
        assert py[n % 2](B, T, Hq, Hkv, mp, page, D, None if W == INT_MAX else W) == want[1]
        n += 1
        split += want[1][0] > 1
    assert n > 1000 and split > 100
    # refusals: -2 for G = 17, for T G = 65 and for D = 96; and the any-G entry's status for the other bad shapes
    for name in (DEC, DEC8):
        assert _plan(name + "_plan", 1, 1, 17, 1, 4, 16, 64, 5)[0] == -2
        assert _plan(name + "_plan", 1, 5, 13, 1, 4, 16, 64, 5)[0] == -2
        assert _plan(name + "_plan", 1, 2, 8, 8, 4, 16, 96, 5)[0] == -2
        for dims in ((0, 2, 8, 8, 4, 16, 64), (1, 9, 8, 8, 4, 16, 64), (1, 2, 8, 3, 4, 16, 64), (1, 2, 8, 8, 4, 48, 64), (1, 2, 8, 8, 1 << 23, 256, 64)):
            for W in (5, 0):
                assert _plan(name + "_plan", *dims, W) == _plan(ANYG(name) + "_plan", *dims, W), (name, dims, W)
    with pytest.raises(RuntimeError, match=r"T 5 x group size 13 = 65 query rows"):
        built.fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan(1, 5, 13, 1, 4, 16, 64, 5)
    with pytest.raises(RuntimeError, match=r"group size 17 "):
        built.fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan(1, 1, 17, 1, 4, 16, 64, 5)


# ---------------------------------------------------------------------------------------------------- the two floats

def test_describe_refuses_bad_floats_names_the_scale_and_the_cap_clause(built):
    m = built.manifest
    for name, dims in ((PRE, (3, 170, 12, 2, 6, 16, 128, 33)), (PRE8, (3, 170, 12, 2, 6, 16, 64, INT_MAX)), (DEC, (3, 4, 12, 2, 6, 16, 128, 33)),
                       (DEC8, (1, 3, 5, 1, 256, 16, 64, 1000))):
        d = name + "_describe"
        for bad in BAD:
            assert _describe(d, *dims, scale=bad)[0] == -1 and _describe(d, *dims, cap=bad)[0] == -1, (name, bad)
            assert _describe(d, *dims[:6], 96, dims[7], scale=bad)[0] == -1  # the floats come first: -1, not the shape's -2
        assert _describe(d, *dims[:6], 96, dims[7])[0] == -2 and _describe(d, *dims[:7], 0)[0] == -1
        D = dims[6]
        base = fs._describe(ANYG(d), *dims)[1]
        for scale, cap in ((0.0, 0.0), (144 ** -0.5, 0.0), (0.0, 50.0), (168 ** -0.5, 30.0)):
            rc, text = _describe(d, *dims, scale=scale, cap=cap)
            assert rc == len(text) > 0 and text.endswith("otherwise " + base), (rc, text)
            assert text == getattr(m, "describe_" + name[len("cln_fa2_"):])(*dims, scale or None, cap or None)
            x = cr.f32(scale) if scale else 1.0 / math.sqrt(D)
            assert text.startswith("%s_mfma<D=%d,CAP=%d> softmax_scale=%.9g (%s)" % (name[4:], D, cap != 0, x, "the caller's" if scale else
                                                                                      "the default 1 / sqrt(D)")), text
            mult = torch.tensor(x * cr.LOG2E, dtype=torch.float32).item() if scale else torch.tensor(cr.LOG2E / D ** 0.5, dtype=torch.float32).item()
            assert "score multiplier x log2(e) = %.9g" % mult in text
            clause = "capped before the window and causal mask (a hidden key is -inf, not -cap), the sink neither scaled nor capped"
            assert (clause in text) == (cap != 0) and ("softcap=%.9g: every score is cap tanh(q.k x / cap)" % cap in text) == (cap != 0)
            assert ("no cap: the any-G body with this multiplier" in text) == (cap == 0)
            assert ("with k_scale inside the tanh" in text) == (cap != 0 and name in (PRE8, DEC8))
        with pytest.raises(ValueError):
            getattr(m, "describe_" + name[len("cln_fa2_"):])(*dims, -1.0, None)


def test_entries_check_the_floats_before_anything_else(built):
    """Never dereferenced: every call fails its checks. A bad float is -1 whatever else is wrong -- a null pointer, a shape that alone is -2 --
    and with good floats the any-G entry's status comes back."""
    p = [0x10000 * (i + 1) for i in range(11)]
    i9 = [ctypes.c_int] * 9
    fl = [ctypes.c_float] * 2
    for name, n_ptr, tail, dims in ((PRE, 9, (), (3, 170, 12, 2, 40, 6, 16, 96)), (PRE8, 11, (), (3, 170, 12, 2, 40, 6, 16, 96)),
                                    (DEC, 9, (1 << 30,), (3, 4, 12, 2, 40, 6, 16, 96)), (DEC8, 11, (1 << 30,), (3, 4, 12, 2, 40, 6, 16, 96))):
        f = _fn(name, [ctypes.c_void_p] * n_ptr + [ctypes.c_longlong] * len(tail) + i9 + fl + [ctypes.c_void_p])
        g = _fn(ANYG(name), [ctypes.c_void_p] * n_ptr + [ctypes.c_longlong] * len(tail) + i9 + [ctypes.c_void_p])
        for scale, cap in ((0.0, 0.0), (0.1, 0.0), (0.0, 50.0), (0.1, 30.0)):
            assert f(*p[:n_ptr], *tail, *dims, 5, scale, cap, None) == g(*p[:n_ptr], *tail, *dims, 5, None) == -2
            assert f(*p[:n_ptr], *tail, *dims, 0, scale, cap, None) == -2 and f(*p[:n_ptr], *tail, *dims[:7], 128, 0, scale, cap, None) == -1
            assert f(None, *p[1:n_ptr], *tail, *dims, 5, scale, cap, None) == -1
        for bad in BAD:
            assert f(*p[:n_ptr], *tail, *dims, 5, bad, 0.0, None) == -1 and f(*p[:n_ptr], *tail, *dims, 5, 0.0, bad, None) == -1, (name, bad)


def test_python_entries_refuse_bad_floats_and_forward_none_as_zero(built, monkeypatch):
    from cuda_learn_notes_amd import host
    import fp8_kv_reference as f8
    BF, i32 = torch.bfloat16, torch.int32
    ints = (torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), torch.zeros(3, dtype=i32))
    b = lambda *s: torch.zeros(*s, dtype=BF)  # noqa: E731
    p8 = lambda: torch.zeros(9, 2, 16, 64, dtype=torch.uint8).view(f8.F8)  # noqa: E731
    pb = lambda: b(9, 2, 16, 64)  # noqa: E731
    sc, Hq = torch.ones(2), 12
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)
    monkeypatch.setattr(host, "_stream", lambda: None)
    seen = []
    monkeypatch.setattr(host, "_lse_fns", {n: (lambda n: lambda *a: seen.append((n, a)) or 0)(n) for n in (PRE, DEC, PRE8, DEC8)})
    pre = lambda s, c: built.fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16(b(40, Hq, 64), pb(), pb(), *ints, 5, None, s, c, b(40, Hq, 64))  # noqa: E731
    dec = lambda s, c: built.fa2_decode_paged_multi_window_sink_softcap_anyg_bf16(b(2, 3, Hq, 64), pb(), pb(), *ints[:2], None, None, s, c,  # noqa: E731
                                                                                  b(2, 3, Hq, 64))
    pre8 = lambda s, c: built.fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8(b(40, Hq, 64), p8(), p8(), *ints, sc, sc, 5, None, s, c,  # noqa: E731
                                                                                         b(40, Hq, 64))
    dec8 = lambda s, c: built.fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8(b(2, 3, Hq, 64), p8(), p8(), *ints[:2], sc, sc, 7, None, s, c,  # noqa: E731
                                                                                       b(2, 3, Hq, 64))
    for call in (pre, dec, pre8, dec8):
        for bad in BAD:
            with pytest.raises(RuntimeError, match=r"softmax_scale .* not supported \(finite and > 0, or None\)"):
                call(bad, None)
            with pytest.raises(RuntimeError, match=r"softcap .* not supported \(finite and > 0, or None\)"):
                call(None, bad)
    assert not seen
    pre(None, 0), dec(0.125, None), pre8(0.0, 50.0), dec8(144 ** -0.5, 30)
    (n0, a0), (n1, a1), (n2, a2), (n3, a3) = seen
    assert (n0, n1, n2, n3) == (PRE, DEC, PRE8, DEC8)
    assert a0[-3:-1] == (0.0, 0.0) and a1[-3:-1] == (0.125, 0.0) and a2[-3:-1] == (0.0, 50.0) and a3[-3:-1] == (144 ** -0.5, 30.0)
    assert a0[-4] == 5 and a1[-4] == INT_MAX and a3[-4] == 7
    assert len(a0) == 21 and len(a1) == 22 and len(a2) == 23 and len(a3) == 24


# ---------------------------------------------------------------------------------------------------- the reference is the dense computation

def test_reference_without_a_defect_is_the_dense_computation():
    """fp64, every row of a small ragged prefill and of a decode, bf16 and e4m3 pools, cap and scale on and off, with a window."""
    g = torch.Generator().manual_seed(5)
    D, Hkv, G, page, Nmax = 64, 2, 3, 16, 48
    Hq = Hkv * G
    Ts, lens = [5, 0, 3], [21, 4, 2]
    k, v = (torch.randn(3, Hkv, Nmax, D, generator=g).to(torch.bfloat16) for _ in range(2))
    pool = pr.make_pool(k, v, page, lens, seed=1)
    p8, ks, vs = ac.to_fp8(pool, Hkv)
    qs = tuple((torch.randn(t, Hq, D, generator=g) * 3).to(torch.bfloat16) for t in Ts)
    q, cu = sr.pack(qs)
    sinks = torch.tensor([0.5, cr.NEG_INF, 30.0, -2.0, 1e30, 3.0])
    worst = 0.0
    for (kp, vp, bt), sc in ((pool, {}), (p8, {"ks": ks, "vs": vs})):
        kd, vd = cr._pools(kp, vp, sc.get("ks"), sc.get("vs"))
        kg, vg = (pr.gather(t, bt, lens) for t in (kd, vd))
        for scale, cap, W in ((None, None, 7), (0.2, None, None), (None, 1.5, 7), (0.2, 1.5, None)):
            O, L, _ = cr.prefill(q, kp, vp, bt, lens, cu, W, sinks, scale, cap, **sc)
            x = cr.scale_in_use(scale, D)
            for b, T in enumerate(Ts):
                for t, h in itertools.product(range(T), range(Hq)):
                    n = max(lens[b] - (T - 1 - t), 0)
                    lo = max(0, n - (INT_MAX if W is None else W))
                    o, lse = cr.dense(q[cu[b] + t, h], kg[b, h // G], vg[b, h // G], n, lo, float(sinks[h]), x, None if cap is None else cr.f32(cap))
                    assert (L[cu[b] + t, h] == cr.NEG_INF) == (lse == cr.NEG_INF) == (n == 0)
                    worst = max(worst, float((O[cu[b] + t, h] - o).abs().max()), 0.0 if n == 0 else abs(float(L[cu[b] + t, h]) - lse))
            q4 = torch.stack([qs[0][:3], qs[2], qs[0][2:]])  # a decode of T = 3 over the same pools
            O, L, _ = cr.decode(q4, kp, vp, bt, lens, W, sinks, scale, cap, **sc)
            for b, t, h in itertools.product(range(3), range(3), range(Hq)):
                n = max(lens[b] - (2 - t), 0)
                lo = max(0, n - (INT_MAX if W is None else W))
                o, lse = cr.dense(q4[b, t, h], kg[b, h // G], vg[b, h // G], n, lo, float(sinks[h]), x, None if cap is None else cr.f32(cap))
                worst = max(worst, float((O[b, t, h] - o).abs().max()), 0.0 if n == 0 else abs(float(L[b, t, h]) - lse))
    assert worst <= 1e-12, worst
    # without a cap and a scale it is the families' reference, and so is the emulation, bit for bit
    O, L, E = cr.prefill(q, *pool, lens, cu, 7, sinks)
    O0, L0, E0 = sr.prefill(q, *pool, lens, cu, 7, sinks)
    fin = torch.isfinite(O0)
    assert torch.equal(O[fin], O0[fin]) and torch.equal(E[fin], E0[fin]) and torch.equal(L[fin[..., 0]], L0[fin[..., 0]])


# ---------------------------------------------------------------------------------------------------- the GPU cases see the six defects

def _ratios(kind, args, kw, D, fp8):
    """{defect: |O_defect - O_64| / bound} of one case under the sensitive scale and cap."""
    fn = cr.prefill if kind == "prefill" else cr.decode
    scale, cap = cr.scale_for(D), cr.CAP
    ro, _, emul = fn(*args, scale, cap, **kw)
    fin = torch.isfinite(ro)
    bound = br.o_bound(emul[fin], ro[fin])
    out = {}
    for d in cr.DEFECTS:
        if d == "no_kscale" and not fp8:
            continue
        o = fn(*args, scale, cap, defect=d, **kw)[0]
        out[d] = float((o[fin] - ro[fin]).abs().max()) / bound
    return out


def test_the_gpu_cases_would_notice_the_six_defects():
    """tests/test_gpu_paged_softcap_attention.py's sensitive cases, on the CPU in fp64: each defect moves O past the case's own bound on at least
    one case of every (entry kind, pool format) it applies to. D = 64: the cap and the scale act on q.k x, whose distribution does not depend
    on D."""
    D = 64
    best = {}

    def note(kind, fp8, got):
        for d, r in got.items():
            best[(kind, fp8, d)] = max(best.get((kind, fp8, d), 0.0), r)
    for fp8 in (False, True):
        def fam(pool, Hkv):
            if not fp8:
                return pool, {}
            p8, ks, vs = ac.to_fp8(pool, Hkv)
            return p8, {"ks": ks, "vs": vs}
        for G, W in itertools.product(cr.P1_G, cr.P1_WINDOWS):
            q, cu, lens, bpool = cr.prefill_case(D, G, 16)
            pool, kw = fam(bpool, ac.P1_HKV)
            note("prefill", fp8, _ratios("prefill", (q, *pool, lens, cu, W, ac.sinks_for(ac.P1_HKV * G, 33)), kw, D, fp8))
        for (T, G), W in itertools.product(cr.D3_TG, ac.D3_WINDOWS):
            q, lens, bpool = cr.decode_one_case(T, G, D)
            pool, kw = fam(bpool, ac.D3_HKV)
            note("decode", fp8, _ratios("decode", (q, *pool, lens, W, ac.sinks_for(ac.D3_HKV * G, 33)), kw, D, fp8))
    kinds = {(k, f, d) for k in ("prefill", "decode") for f in (False, True) for d in cr.DEFECTS if f or d != "no_kscale"}
    assert set(best) == kinds
    for key, r in sorted(best.items()):
        print("%s %s %s: %.1f x the bound" % (key[0], "fp8" if key[1] else "bf16", key[2], r))
    print("smallest defect / bound: %.1f" % min(best.values()))
    assert all(r > 1.0 for r in best.values()), {k: r for k, r in best.items() if r <= 1.0}


# ---------------------------------------------------------------------------------------------------- registers and instructions

@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_prefill_kernels_keep_two_workgroups_per_cu_and_the_any_g_mfma_count(tmp_path, fp8):
    tail = "_bf16_fp8" if fp8 else "_bf16"
    got = fs._bodies("flash_attn_prefill_paged_varlen_window_sink_softcap_anyg%s.hip" % tail, tmp_path)  # asserts no spill, no scratch
    sib = dict((k["lds"], (fs._loop_mfmas(b), k)) for k, b in fs._bodies("flash_attn_prefill_paged_varlen_window_sink_anyg%s.hip" % tail, tmp_path))
    assert len(got) == 4 and all("fa2_prefill_paged_varlen_window_sink_softcap_anyg%s_mfma" % tail in k["name"] for k, _ in got), [k["name"] for k, _ in got]
    caps, rcps = set(), {}
    for k, body in got:
        D = 128 if k["lds"] > 30000 else 64
        cap = "ELb1E" in k["name"]
        caps.add((D, cap))
        print(k["name"], {x: k[x] for x in ("vgpr", "sgpr", "lds")}, "any-G:", {x: sib[k["lds"]][1][x] for x in ("vgpr", "sgpr", "lds")})
        assert 0 < 2 * k["lds"] <= fs.LDS_PER_CU and k["vgpr"] <= 256, k  # two workgroups per CU, two waves per SIMD
        assert fs._loop_mfmas(body) == D // 2 == sib[k["lds"]][0], k["name"]
        assert "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body and ("v_cvt_scalef32_pk_bf16_fp8" in body) == fp8, k["name"]
        assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", ""), k["name"]
        rcps[(D, cap)] = body.count("v_rcp_f32")
    assert caps == {(64, False), (64, True), (128, False), (128, True)}
    for D in (64, 128):  # the tanh: a v_rcp_f32 per score of a step's two row tiles, in the CAP kernels only (both softmax steps are inlined)
        assert rcps[(D, True)] >= rcps[(D, False)] + 2 * 16, rcps


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_decode_kernels_the_any_g_mfma_counts_and_the_two_combines(tmp_path, fp8):
    tail = "_bf16_fp8" if fp8 else "_bf16"
    got = fs._bodies("flash_attn_decode_paged_multi_window_sink_softcap_anyg%s.hip" % tail, tmp_path)  # asserts no spill, no scratch
    stream = [(k, b) for k, b in got if "fa2_decode_paged_multi_window_sink_softcap_anyg%s_mfma" % tail in k["name"]]
    combine = [(k, b) for k, b in got if "fa2_decode_combine_window_" in k["name"]]
    assert len(stream) == 16 and len(combine) == 4 and len(got) == 20, [k["name"] for k, _ in got]
    sib_bodies = [(k, b) for k, b in fs._bodies("flash_attn_decode_paged_multi_window_sink_anyg%s.hip" % tail, tmp_path) if "_mfma" in k["name"]]
    sib_regs = {re.search(r"ILi(\d+)ELi(\d)E", k["name"]).groups(): {x: k[x] for x in ("vgpr", "agpr", "sgpr")} for k, _ in sib_bodies}
    want = sorted([8 * mt for mt in (1, 2, 3, 4)] + [16 * mt for mt in (1, 2, 3, 4)])
    rcps = {}
    assert sorted(fs._loop_mfmas(b) for _, b in sib_bodies) == want
    for cap in (False, True):
        assert sorted(fs._loop_mfmas(b) for k, b in stream if ("ELb1E" in k["name"]) == cap) == want
    for k, body in stream:
        m = re.search(r"ILi(\d+)ELi(\d)ELb(\d)E", k["name"])
        D, MT, cap = int(m.group(1)), int(m.group(2)), m.group(3) == "1"
        # the allocation is the compiler's and may differ from the any-G kernel's by a few registers (DESIGN 4.4.14 has both): printed, not pinned
        print(k["name"], {x: k[x] for x in ("vgpr", "agpr", "sgpr")}, "any-G:", sib_regs[m.groups()[:2]])
        assert fs._loop_mfmas(body) == (8 if D == 64 else 16) * MT, k["name"]
        assert "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body and ("v_cvt_scalef32_pk_bf16_fp8" in body) == fp8, k["name"]
        assert k["vgpr"] <= 512, k
        rcps[(D, MT, cap)] = body.count("v_rcp_f32")
    for D, MT in itertools.product((64, 128), (1, 2, 3, 4)):  # the tanh: a v_rcp_f32 per score, 8 per row tile, in the CAP kernels only
        assert rcps[(D, MT, True)] >= rcps[(D, MT, False)] + 8 * MT, rcps
    for k, body in combine:
        assert "v_cvt_pk_bf16_f32" in body and "global_store_short" in body and "v_mfma" not in body, k["name"]
