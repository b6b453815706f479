"""CPU: the prompt path of multi-head latent attention (include/cln_amd_ext.h: cln_fa2_prefill_varlen_mla_bf16, cln_attn_merge_states_bf16,
cln_kv_gather_paged_mla_bf16, each with its describe entry; csrc/flash_attn_prefill_varlen_mla_bf16.*, attn_merge_states_bf16.*,
kv_gather_paged_mla_bf16.*) -- the reference anchored to the existing one, header, exports and package, the statuses, the Python
entries, the describe texts and the kernels' resources. No GPU needed: hipcc cross-compiles."""
import ctypes
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
import mla_prefill_reference as mp  # noqa: E402
import paged_mla_reference as ml  # noqa: E402
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the sibling surface test's readers of a code object)

PRE, MRG, GAT = "cln_fa2_prefill_varlen_mla_bf16", "cln_attn_merge_states_bf16", "cln_kv_gather_paged_mla_bf16"
NAMES = (PRE, PRE + "_describe", MRG, MRG + "_describe", GAT, GAT + "_describe")
UNITS = ("flash_attn_prefill_varlen_mla_bf16", "attn_merge_states_bf16", "kv_gather_paged_mla_bf16")
BF = torch.bfloat16
NAN, INF = float("nan"), float("inf")
BAD_SCALES = (0.0, -1.0, NAN, INF, -INF)
S = mp.SCALE
_fn = fs._fn
PRE_ARGS = [ctypes.c_void_p] * 7 + [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_void_p]
MRG_ARGS = [ctypes.c_void_p] * 6 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]
GAT_ARGS = [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_void_p]


def _describe(name, argtypes, *args):
    fn = _fn(name + "_describe", list(argtypes) + [ctypes.c_char_p, ctypes.c_int])
    buf = ctypes.create_string_buffer(4096)
    rc = fn(*args, buf, 4096)
    return rc, buf.value.decode()


def _describe_pre(B, tq, tk, Hq, causal, scale):
    return _describe(PRE, [ctypes.c_int] * 5 + [ctypes.c_float], B, tq, tk, Hq, causal, scale)


# ---------------------------------------------------------------------------------------------------- the reference

@pytest.mark.parametrize("T", [1, 5, 8])
def test_reference_is_the_latent_decode_reference_with_v_equal_k_nope(T):
    """v = k_nope, one head at a time: the key rows [k_nope_h | k_pe] are latent rows of dk = 192 whose first 128 dims are the value, so the fp64 O
    and LSE are paged_mla_reference.decode(..., dv=128)'s to rounding and the emulation is its emulation (the two form P V from a slice and from
    a tensor of its own: at most one bf16 ulp apart, and equal in nearly every entry)."""
    g = torch.Generator().manual_seed(T)
    Hq, lens, page, scale = 3, [40, T, 2, 0], 16, 0.11
    B = len(lens)
    Ts = [T] * B
    cu_q, cu_k = mp.cu_of(Ts), mp.cu_of(lens)
    q = torch.randn(cu_q[-1], Hq, mp.DQ, generator=g).to(BF)
    kv = torch.randn(cu_k[-1], Hq, mp.DKV, generator=g).to(BF)
    kv[..., mp.DN:] = kv[..., :mp.DN]
    k_pe = torch.randn(cu_k[-1], mp.DR, generator=g).to(BF)
    o, l, e = mp.prefill(q, kv, k_pe, cu_q, cu_k, scale, causal=True)
    assert not bool(torch.isnan(o).any()) and bool((e.bfloat16().double() == e).all())
    for h in range(Hq):
        dense = torch.zeros(B, 48, mp.DQ, dtype=BF)
        for b in range(B):
            dense[b, :lens[b]] = torch.cat([kv[cu_k[b]:cu_k[b + 1], h, :mp.DN], k_pe[cu_k[b]:cu_k[b + 1]]], dim=-1)
        pool, bt = ml.make_pool(dense, page, lens, seed=h)
        ro, rl, re_ = ml.decode(q[:, h].reshape(B, T, 1, mp.DQ), pool, bt, lens, scale, dv=mp.DV)
        ro, rl, re_ = ro.reshape(B * T, mp.DV), rl.reshape(B * T), re_.reshape(B * T, mp.DV)
        fin = torch.isfinite(rl)
        assert torch.equal(torch.isfinite(l[:, h]), fin) and bool((l[:, h][~fin] == mp.NEG_INF).all())
        assert float((l[:, h][fin] - rl[fin]).abs().max()) < 1e-12 and float((o[:, h] - ro).abs().max()) < 1e-12
        diff = (e[:, h] - re_).abs()
        assert float((diff / re_.abs().clamp(min=2.0 ** -126)).max()) <= 2.0 ** -7, "more than one bf16 ulp"
        assert float((diff != 0).double().mean()) < 0.01
    assert bool((l[3 * T:] == mp.NEG_INF).all()) and bool((o[3 * T:] == 0).all())       # the sequence without a key
    if T > 2:
        assert bool((l[2 * T:3 * T - 2] == mp.NEG_INF).all()) and bool(torch.isfinite(l[3 * T - 2:3 * T]).all())  # L = 2 < T
    # non-causal: every row sees all keys, so every row of a sequence equals the causal last row's key set
    on, ln_, _ = mp.prefill(q, kv, k_pe, cu_q, cu_k, scale, causal=False)
    last = [cu_q[b + 1] - 1 for b in range(B)]
    assert torch.equal(ln_[last], l[last]) and torch.equal(on[last], o[last]) and bool(torch.isfinite(ln_[:3 * T]).all())


def test_the_fp64_merge_joins_two_halves_of_one_softmax():
    g = torch.Generator().manual_seed(3)
    s, v = torch.randn(5, 40, generator=g, dtype=torch.float64), torch.randn(40, 8, generator=g, dtype=torch.float64)
    whole = torch.softmax(s, -1) @ v
    parts = [(torch.softmax(s[:, a:b], -1) @ v[a:b], torch.logsumexp(s[:, a:b], -1)) for a, b in ((0, 13), (13, 40))]
    o, l = mp.merge(parts[0][0], parts[0][1], parts[1][0], parts[1][1])
    assert float((o - whole).abs().max()) < 1e-14 and float((l - torch.logsumexp(s, -1)).abs().max()) < 1e-14
    ninf = torch.full((5,), mp.NEG_INF, dtype=torch.float64)
    o, l = mp.merge(parts[0][0], parts[0][1], torch.full((5, 8), NAN, dtype=torch.float64), ninf)
    assert torch.equal(o, parts[0][0]) and torch.equal(l, parts[0][1])
    o, l = mp.merge(parts[0][0], ninf, parts[0][0] * NAN, ninf)
    assert bool((o == 0).all()) and bool((l == mp.NEG_INF).all())


# ---------------------------------------------------------------------------------------------------- header, exports

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_six_prototypes(tmp_path, lang, cc):
    assert shutil.which(cc), cc
    pre = "const void*, const void*, const void*, const int*, const int*, void*, float*, " + "int, " * 5 + "float, void*"
    pre_d = "int, int, int, int, int, float, char*, int"
    mrg = "const void*, const float*, const void*, const float*, void*, float*, long long, int, void*"
    mrg_d = "long long, int, char*, int"
    gat = "const void*, const int*, const int*, const int*, void*, int, int, int, int, int, void*"
    gat_d = "int, int, int, int, char*, int"
    protos = (pre, pre_d, mrg, mrg_d, gat, gat_d)
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n' + "".join("int (*f%d)(%s) = %s;\n" % (i, p, n) for i, (p, n) in enumerate(zip(protos, NAMES)))
                   + "int main(void) { return f0 && f5 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_header_manifest_package_host_and_build_hold_the_entries(built):
    lib, hdr = fs._lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in ("fa2_prefill_varlen_mla_bf16", "attn_merge_states_bf16", "kv_gather_paged_mla_bf16"):
        assert hasattr(built, n) and hasattr(host, n), n
        assert hasattr(built.manifest, "describe_" + n.replace("fa2_", "")), n
    build = open(os.path.join(ROOT, "cuda-learn-notes_amd", "_build.py")).read()
    for unit in UNITS:
        assert '"%s.hip"' % unit in build and os.path.exists(os.path.join(fs.CSRC, unit + ".hip")), unit
        assert os.path.exists(os.path.join(fs.CSRC, unit + ".cuh")), unit


# ---------------------------------------------------------------------------------------------------- statuses of the entries

def _buffers(n):
    buf = (ctypes.c_char * (256 * (n + 1)))()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    return buf, [base + 256 * i for i in range(n)]


def test_prefill_statuses_scale_first_then_the_siblings(built):
    """Nothing is launched: every call here is refused."""
    fn = _fn(PRE, PRE_ARGS)
    keep, (q, kv, kpe, cuq, cuk, o, lse) = _buffers(7)
    dims = (2, 8, 8, 16, 1)  # B, total_q, total_k, Hq, causal
    for bad in BAD_SCALES:
        assert fn(q, kv, kpe, cuq, cuk, o, lse, *dims, bad, None) == -1, bad
        assert fn(None, None, None, None, None, None, None, 0, 0, 0, 129, 7, bad, None) == -1, bad  # before everything else
        assert _describe_pre(2, 8, 8, 16, 1, bad)[0] == -1, bad
    for i in range(6):  # a missing q, kv, k_pe, cu_q, cu_k or o
        args = [q, kv, kpe, cuq, cuk, o]
        args[i] = None
        assert fn(*args, lse, *dims, S, None) == -1, i
        assert fn(*args, lse, 2, 8, 8, 129, 1, S, None) == -1, i  # the pointers come before the shape
    assert fn(q + 8, kv, kpe, cuq, cuk, o, lse, *dims, S, None) == -1 and fn(q, kv + 8, kpe, cuq, cuk, o, lse, *dims, S, None) == -1
    assert fn(q, kv, kpe + 8, cuq, cuk, o, lse, *dims, S, None) == -1 and fn(q, kv, kpe, cuq, cuk, o + 8, lse, *dims, S, None) == -1
    assert fn(q, kv, kpe, cuq + 2, cuk, o, lse, *dims, S, None) == -1 and fn(q, kv, kpe, cuq, cuk + 2, o, lse, *dims, S, None) == -1
    assert fn(q, kv, kpe, cuq, cuk, o, lse + 2, *dims, S, None) == -1
    assert fn(q, kv, kpe, cuq, cuk, q, lse, *dims, S, None) == -1 and fn(q, kv, kpe, cuq, cuk, o, o, *dims, S, None) == -1  # aliases
    assert fn(q, kv, kpe, cuq, cuk, o, cuq, *dims, S, None) == -1
    for bad_dims in ((0, 8, 8, 16, 1), (2, 0, 8, 16, 1), (2, 8, 0, 16, 1), (2, 8, 8, 0, 1), (-1, 8, 8, 16, 0)):
        assert fn(q, kv, kpe, cuq, cuk, o, lse, *bad_dims, S, None) == -1, bad_dims
        assert _describe_pre(*bad_dims, S)[0] == -1, bad_dims
    # the grid: Hq (total_q / 128 + B) workgroups of 256 threads, below 2^32 threads in x
    for bad_dims in ((2, 8, 8, 129, 1), (2, 8, 8, 16, 2), (2, 8, 8, 16, -1), (2 ** 31 - 1, 2 ** 31 - 1, 8, 128, 1), (1, 2 ** 31 - 1, 8, 1, 1),
                     (1, 2 ** 24, 8, 128, 1)):
        assert fn(q, kv, kpe, cuq, cuk, o, lse, *bad_dims, S, None) == -2, bad_dims
        assert _describe_pre(*bad_dims, S)[0] == -2, bad_dims
    assert _describe_pre(2, 8, 8, 128, 0, S)[0] > 0 and _describe_pre(1, 2 ** 31 - 257, 2 ** 31 - 1, 1, 1, S)[0] > 0
    assert _describe_pre(1, 2 ** 24 - 256, 8, 128, 1, S)[0] > 0
    del keep


def test_merge_and_gather_statuses(built):
    fn = _fn(MRG, MRG_ARGS)
    keep, (oa, la, ob, lb, o, lse) = _buffers(6)
    for i in range(5):  # a missing o_a, lse_a, o_b, lse_b or o
        args = [oa, la, ob, lb, o]
        args[i] = None
        assert fn(*args, lse, 4, 128, None) == -1, i
    assert fn(oa + 8, la, ob, lb, o, lse, 4, 128, None) == -1 and fn(oa, la + 2, ob, lb, o, lse, 4, 128, None) == -1
    assert fn(oa, la, ob, lb, o + 8, lse, 4, 128, None) == -1 and fn(oa, la, ob, lb, o, lse + 2, 4, 128, None) == -1
    assert fn(oa, la, ob, lb, ob, lse, 4, 128, None) == -1 and fn(oa, la, ob, lb, o, lb, 4, 128, None) == -1  # o is o_b, lse is lse_b
    assert fn(oa, la, ob, lb, o, o, 4, 128, None) == -1 and fn(oa, la, ob, lb, la, lse, 4, 128, None) == -1
    assert fn(oa, la, ob, lb, o, lse, 0, 128, None) == -1 and fn(oa, la, ob, lb, o, lse, 4, 0, None) == -1 and fn(oa, la, ob, lb, o, lse, -1, 8, None) == -1
    for D in (4, 12, 520, 1024, 129):
        assert fn(oa, la, ob, lb, o, lse, 4, D, None) == -2, D
        assert fn(oa, la, ob, lb, oa, la, 4, D, None) == -2, D  # in place passes the pointer checks
        assert _describe(MRG, [ctypes.c_longlong, ctypes.c_int], 4, D)[0] == -2
    assert fn(oa, la, ob, lb, o, lse, 2 ** 40, 512, None) == -2  # the grid
    for D in (8, 24, 128, 512):
        assert _describe(MRG, [ctypes.c_longlong, ctypes.c_int], 4, D)[0] > 0
    # the gather
    gf = _fn(GAT, GAT_ARGS)
    keep2, (pool, bt, st, cuk, out) = _buffers(5)
    dims = (2, 8, 3, 4, 16)  # B, total_k, P, max_pages, page
    for i in (0, 1, 3, 4):  # a missing pool, table, cu_k or out; starts may be missing
        args = [pool, bt, st, cuk, out]
        args[i] = None
        assert gf(*args, *dims, None) == -1, i
    assert gf(pool + 8, bt, st, cuk, out, *dims, None) == -1 and gf(pool, bt + 2, st, cuk, out, *dims, None) == -1
    assert gf(pool, bt, st + 2, cuk, out, *dims, None) == -1 and gf(pool, bt, st, cuk, out + 8, *dims, None) == -1
    assert gf(pool, bt, st, cuk, pool, *dims, None) == -1  # the output is an input
    assert gf(pool, bt, None, cuk, out, 2, 8, 0, 4, 16, None) == -1 and gf(pool, bt, None, cuk, out, 2, 0, 3, 4, 16, None) == -1
    assert gf(pool, bt, None, cuk, out, 0, 8, 3, 4, 16, None) == -1 and gf(pool, bt, None, cuk, out, 2, 8, 3, 0, 16, None) == -1
    assert gf(pool, bt, None, cuk, out, 2, 8, 3, 4, 48, None) == -2 and gf(pool, bt, None, cuk, out, 2, 8, 3, 4, 512, None) == -2
    assert gf(pool, bt, None, cuk, out, 2, 8, 3, 1 << 23, 256, None) == -2
    del keep, keep2


# ---------------------------------------------------------------------------------------------------- describe texts

def test_describe_texts_equal_their_manifest_mirrors(built):
    m = built.manifest
    for B, tq, tk, Hq, causal in ((1, 4096, 4096, 16, 1), (5, 235, 501, 3, 1), (4, 8192, 8192, 128, 0), (3, 1, 1, 1, 1)):
        rc, text = _describe_pre(B, tq, tk, Hq, causal, S)
        slots = tq // 128 + B
        assert rc == len(text) and text == m.describe_prefill_varlen_mla_bf16(B, tq, tk, Hq, causal, S)
        assert text.startswith("fa2_prefill_varlen_mla_bf16_mfma<Dk=192,Dv=128> softmax_scale=%.9g " % ctypes.c_float(S).value)
        assert "v_mfma_f32_16x16x32_bf16" in text and "_f16" not in text
        assert "%d slots per head (total_q / 128 + B), grid %d workgroups" % (slots, Hq * slots) in text
        assert "45056 bytes static: K rows of 416 bytes, V rows of 288" in text and "80 MFMAs per wave and step" in text
        assert (" causal:" in text) == bool(causal) and (" non-causal:" in text) == (not causal)
        assert text.endswith("; deterministic")
    with pytest.raises(ValueError, match="status -2"):
        m.describe_prefill_varlen_mla_bf16(1, 8, 8, 129, 1, S)
    with pytest.raises(ValueError, match="status -1"):
        m.describe_prefill_varlen_mla_bf16(1, 8, 8, 16, 1, 0.0)
    for rows, D in ((1, 8), (257, 128), (2 ** 32, 512), (100, 24)):
        rc, text = _describe(MRG, [ctypes.c_longlong, ctypes.c_int], rows, D)
        rpw = 256 // (D // 8)
        assert rc == len(text) and text == m.describe_attn_merge_states_bf16(rows, D)
        assert text.startswith("attn_merge_states_bf16_rows rows=%d D=%d: " % (rows, D))
        assert "%d workgroups of 256 threads, %d whole rows each" % (-(-rows // rpw), rpw) in text and text.endswith("; deterministic")
    with pytest.raises(ValueError, match="status -2"):
        m.describe_attn_merge_states_bf16(4, 520)
    for B, tk, mp_, page in ((3, 100, 8, 16), (1, 14336, 64, 256)):
        rc, text = _describe(GAT, [ctypes.c_int] * 4, B, tk, mp_, page)
        assert rc == len(text) and text == m.describe_kv_gather_paged_mla_bf16(B, tk, mp_, page)
        assert text.startswith("kv_gather_paged_mla_bf16_rows B=%d total_k=%d page=%d: " % (B, tk, page))
        assert "%d x 1 workgroups of 256 threads" % tk in text and "the 72 16-byte pieces" in text and "= %d written as zeros" % (mp_ * page) in text
    with pytest.raises(ValueError, match="status -2"):
        m.describe_kv_gather_paged_mla_bf16(3, 100, 8, 48)


# ---------------------------------------------------------------------------------------------------- the Python entries

def test_python_entries_refuse_bad_tensors_before_any_device_call(built, monkeypatch):
    """No GPU. First with the real device check: a CPU tensor is refused. Then the device check is replaced, and a call that gets as far as the
    C entry shows it by raising Reached. (Contiguity is part of the device check: tests/test_gpu_mla_prefill.py has that case.)"""
    from cuda_learn_notes_amd import host

    class Reached(Exception):
        pass

    def reached(name, argtypes):
        raise Reached(name)

    b = lambda *sh: torch.zeros(*sh, dtype=BF)  # noqa: E731
    i = lambda *sh: torch.zeros(*sh, dtype=torch.int32)  # noqa: E731
    f = lambda *sh: torch.zeros(*sh, dtype=torch.float32)  # noqa: E731
    pre, mrg, gat = built.fa2_prefill_varlen_mla_bf16, built.attn_merge_states_bf16, built.kv_gather_paged_mla_bf16
    good = dict(q=b(8, 16, 192), kv=b(9, 16, 256), k_pe=b(9, 64), cu_q=i(3), cu_k=i(3), softmax_scale=S, out=b(8, 16, 128))
    gm = dict(o_a=b(8, 16, 128), lse_a=f(8, 16), o_b=b(8, 16, 128), lse_b=f(8, 16), out=b(8, 16, 128))
    gg = dict(pool=b(3, 16, 576), block_table=i(2, 4), cu_k=i(3), out=b(8, 576))
    call = lambda **kw: pre(**{**good, **kw})  # noqa: E731
    mcall = lambda **kw: mrg(**{**gm, **kw})  # noqa: E731
    gcall = lambda **kw: gat(**{**gg, **kw})  # noqa: E731
    for c in (call, mcall, gcall):
        with pytest.raises(RuntimeError, match="expected a GPU"):
            c()
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)
    for kw in (dict(q=good["q"].half()), dict(kv=good["kv"].float()), dict(k_pe=good["k_pe"].half()), dict(out=good["out"].half()),
               dict(cu_q=torch.zeros(3, dtype=torch.int64)), dict(cu_k=torch.zeros(3, dtype=torch.int64)), dict(lse=torch.zeros(8, 16, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="values must be"):
            call(**kw)
    with pytest.raises(RuntimeError, match="q of 576 dims not supported"):
        call(q=b(8, 16, 576))
    with pytest.raises(RuntimeError, match="q of 128 dims not supported"):
        call(q=b(8, 16, 128))
    for kw in (dict(q=b(8, 192)), dict(kv=b(9, 16, 192)), dict(kv=b(9, 8, 256)), dict(k_pe=b(8, 64)), dict(k_pe=b(9, 16, 64)), dict(k_pe=b(9, 32)),
               dict(cu_k=i(4)), dict(cu_q=i(1)), dict(out=b(8, 16, 192)), dict(out=b(7, 16, 128)), dict(lse=f(8, 15)), dict(lse=f(8, 16, 1))):
        with pytest.raises(RuntimeError, match="size mismatch"):
            call(**kw)
    for bad in BAD_SCALES:
        with pytest.raises(RuntimeError, match="softmax_scale .* not supported"):
            call(softmax_scale=bad)
    with pytest.raises(TypeError):
        pre(good["q"], good["kv"], good["k_pe"], good["cu_q"], good["cu_k"], None, good["out"])  # there is no default
    with pytest.raises(RuntimeError, match="129 query heads not supported"):
        call(q=b(8, 129, 192), kv=b(9, 129, 256), out=b(8, 129, 128))
    # the merge
    for kw in (dict(o_a=gm["o_a"].half()), dict(o_b=gm["o_b"].float()), dict(out=gm["out"].half()), dict(lse_a=gm["lse_a"].double()),
               dict(lse_b=gm["lse_b"].half()), dict(lse=gm["lse_a"].double())):
        with pytest.raises(RuntimeError, match="values must be"):
            mcall(**kw)
    for kw in (dict(o_b=b(8, 16, 64)), dict(out=b(8, 8, 128)), dict(lse_a=f(8, 15)), dict(lse_b=f(128)), dict(lse=f(8, 16, 1)), dict(o_a=b(128), o_b=b(128), out=b(128))):
        with pytest.raises(RuntimeError, match="size mismatch"):
            mcall(**kw)
    for D in (4, 12, 520, 1024):
        with pytest.raises(RuntimeError, match="D %d not supported" % D):
            mrg(b(8, D), f(8), b(8, D), f(8), b(8, D))
    # the gather
    for kw in (dict(pool=gg["pool"].half()), dict(out=gg["out"].float()), dict(cu_k=torch.zeros(3, dtype=torch.int64)), dict(starts=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="values must be"):
            gcall(**kw)
    for kw in (dict(pool=b(3, 16, 512)), dict(out=b(8, 512)), dict(out=b(8, 1, 576)), dict(cu_k=i(2)), dict(starts=i(3)), dict(block_table=i(8))):
        with pytest.raises(RuntimeError, match="size mismatch"):
            gcall(**kw)
    with pytest.raises(RuntimeError, match="page size 48"):
        gcall(pool=b(3, 48, 576))
    # good calls reach the C entries
    monkeypatch.setattr(host, "_ext_fn", reached)
    with pytest.raises(Reached, match=PRE):
        call(lse=f(8, 16), causal=False)
    with pytest.raises(Reached, match=MRG):
        mcall(out=gm["o_a"], lse=gm["lse_a"])
    with pytest.raises(Reached, match=GAT):
        gcall(starts=i(2))


# ---------------------------------------------------------------------------------------------------- registers and instructions

def test_prefill_kernel_resources_and_its_mfmas(tmp_path):
    """Two workgroups per CU (__launch_bounds__(256, 2): at most 256 registers), LDS 64 x 416 + 64 x 288 = 45056 bytes, no spill, no scratch. The
    loop's MFMAs per wave: 4 key blocks x 6 k-steps x 2 row tiles for S^T plus 8 dim blocks x 2 key pairs x 2 row tiles for O^T = 48 + 32 = 80,
    all bf16 16x16x32."""
    got = fs._bodies("flash_attn_prefill_varlen_mla_bf16.hip", tmp_path)  # asserts no spill, no scratch, no _f16
    assert len(got) == 1, [k["name"] for k, _ in got]
    k, body = got[0]
    print(k["name"], {x: k.get(x) for x in ("vgpr", "agpr", "sgpr", "lds", "spill", "sgpr_spill", "scratch")})
    assert "fa2_prefill_varlen_mla_bf16_mfma" in k["name"]
    assert k["lds"] == 64 * (2 * 192 + 32) + 64 * (2 * 128 + 32) == 45056 and 2 * k["lds"] <= fs.LDS_PER_CU
    assert k["vgpr"] + k.get("agpr", 0) <= 256, k  # two waves per SIMD
    assert fs._loop_mfmas(body) == 4 * 6 * 2 + 8 * 2 * 2 == 80
    assert "ds_read_b64_tr_b16" in body and "v_cvt_pk_bf16_f32" in body
    assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", "")


def test_merge_and_gather_kernels_resources(tmp_path):
    for unit, name in (("attn_merge_states_bf16.hip", "attn_merge_states_bf16_rows"), ("kv_gather_paged_mla_bf16.hip", "kv_gather_paged_mla_bf16_rows")):
        got = fs._bodies(unit, tmp_path)  # asserts no spill, no scratch, no _f16, no atomics
        assert len(got) == 1 and name in got[0][0]["name"], [k["name"] for k, _ in got]
        k, body = got[0]
        print(k["name"], {x: k.get(x) for x in ("vgpr", "agpr", "sgpr", "lds", "spill", "sgpr_spill", "scratch")})
        assert k["lds"] == 0 and "v_mfma" not in body and k["vgpr"] <= 128
    assert "v_cvt_pk_bf16_f32" in fs._bodies("attn_merge_states_bf16.hip", tmp_path)[0][1]


# ---------------------------------------------------------------------------------------------------- a scale that is not the data's

@pytest.mark.parametrize("scale", mp.OTHER_SCALES, ids=["yarn", "quarter"])
@pytest.mark.parametrize("causal", [True, False], ids=["causal", "non-causal"])
def test_the_gpu_cases_at_another_scale_would_notice_the_datas_scale(causal, scale):
    """tests/test_gpu_mla_prefill.py runs the ragged packed batch at V3's YaRN scale and at SCALE / 4 (Q_MULT = 1: the data is standard
    normal): a kernel that ran at SCALE whatever it was given would be more than 20 x o_bound from the reference."""
    assert mp.OTHER_SCALES == ml.OTHER_SCALES and mp.Q_MULT == 1
    ref, ref0 = mp.scale_case(causal, scale)[5:]
    diff, need = ml.sees_the_scale(ref, ref0)
    print("mla prefill scale %.5f causal=%d: |O(scale) - O(SCALE)| = %.3e against 20 x o_bound = %.3e" % (scale, causal, diff, need))
    assert diff > need
