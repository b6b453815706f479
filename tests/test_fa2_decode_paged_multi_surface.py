"""CPU: the multi-token paged decode attention entries (include/cln_amd_ext.h: cln_fa2_decode_paged_multi_plan, cln_fa2_decode_paged_multi,
cln_fa2_decode_paged_multi_describe; csrc/flash_attn_decode_paged_multi.hip) -- header, exports, argument checks before any device access, the plan
against its Python mirror and the describe text, the references of tests/multi_decode_reference.py, a numpy model of the kernel's register
dataflow, and the kernels' code (MFMA on both products, no spill, no scratch, no atomics). No GPU needed: hipcc cross-compiles."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cln_amd_ext.h")
CSRC = os.path.join(ROOT, "cuda-learn-notes_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "cuda-learn-notes_amd", "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_kernels as dk  # noqa: E402
import multi_decode_reference as mr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
from test_fragment_layout_model import ds_read_b64_tr_b16, lds_halves, mfma_16x16x32  # noqa: E402

NAMES = ("cln_fa2_decode_paged_multi_plan", "cln_fa2_decode_paged_multi", "cln_fa2_decode_paged_multi_describe")
# the plan grid: (B, Hkv) with B Hkv = 1, 8, 15, 256, 2048; every G, page and T below; max_pages that give Nmax from 16 to 65536
BHKV = ((1, 1), (1, 8), (3, 5), (8, 32), (64, 32))
MAXPAGES = (1, 3, 63, 256)
TS = (1, 2, 5, 8)


def grid():
    for D in (64, 128):
        for (B, Hkv) in BHKV:
            for G in pr.GROUPS:
                for page in pr.PAGES:
                    for mp in MAXPAGES:
                        for T in TS:
                            yield B, T, Hkv * G, Hkv, mp, page, D


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_three_prototypes(tmp_path, lang, cc):
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*p1)(int, int, int, int, int, int, int, int*, int*, long long*) = cln_fa2_decode_paged_multi_plan;\n"
                   "int (*d1)(const void*, const void*, const void*, const int*, const int*, void*, float*, void*, long long, int, int, int, int, int,"
                   " int, int, int, void*) = cln_fa2_decode_paged_multi;\n"
                   "int (*t1)(int, int, int, int, int, int, int, char*, int) = cln_fa2_decode_paged_multi_describe;\n"
                   "int main(void) { return p1 && d1 && t1 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _multi():
    fn = _lib().cln_fa2_decode_paged_multi
    fn.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_longlong] + [ctypes.c_int] * 8 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def _plan(B, T, Hq, Hkv, max_pages, page, D):
    fn = _lib().cln_fa2_decode_paged_multi_plan
    fn.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 3
    fn.restype = ctypes.c_int
    s, c, w = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
    rc = fn(B, T, Hq, Hkv, max_pages, page, D, ctypes.addressof(s), ctypes.addressof(c), ctypes.addressof(w))
    return rc, s.value, c.value, w.value


def test_product_library_and_package_export_the_entries(built):
    lib = _lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    from cuda_learn_notes_amd import host
    for n in ("fa2_decode_paged_multi", "fa2_decode_paged_multi_plan"):
        assert hasattr(built, n) and hasattr(host, n), n
    assert hasattr(built.manifest, "describe_decode_paged_multi")


def test_multi_decode_checks_arguments_before_any_device_access(built):
    f = _multi()
    # q, k_pages, v_pages, block_table, seqlens, o, lse, workspace: never dereferenced, every call below fails its checks first
    p = [0x10000 * (i + 1) for i in range(8)]
    big = 1 << 40
    split = (1, 4, 8, 2, 400, 256, 16, 128)  # B, T, Hq, Hkv, P, max_pages, page, D: a shape whose plan splits the keys
    rc, S, C, need = _plan(1, 4, 8, 2, 256, 16, 128)
    assert rc == 0 and S > 1 and need > 0
    for i in (0, 1, 2, 3, 4, 5):  # a null required pointer
        a = list(p)
        a[i] = None
        assert f(*a, big, *split, None) == -1, i
    for i in (0, 1, 2, 5, 6, 7):  # 16-byte alignment
        a = list(p)
        a[i] = p[i] + 8
        assert f(*a, big, *split, None) == -1, i
    for i in (3, 4):  # block_table, seqlens: 4-byte alignment
        a = list(p)
        a[i] = p[i] + 2
        assert f(*a, big, *split, None) == -1, i
    for out in (5, 6, 7):  # an output equal to an input or to another output
        for src in range(8):
            if src != out:
                a = list(p)
                a[out] = p[src]
                assert f(*a, big, *split, None) == -1, (out, src)
    for i in range(8):  # each dim non-positive
        for bad in (0, -2):
            d = list(split)
            d[i] = bad
            assert f(*p, big, *d, None) == -1, d
    assert f(*p, big, 1, 4, 8, 3, 400, 256, 16, 128, None) == -1  # Hq % Hkv
    for T in (9, 16, 64):
        assert f(*p, big, 1, T, 8, 2, 400, 256, 16, 128, None) == -2, T
    for D in (32, 96, 256, 512):
        assert f(*p, big, 1, 4, 8, 2, 400, 256, 16, D, None) == -2, D
    for (Hq, Hkv) in ((3, 1), (6, 2), (16, 1), (5, 1)):  # G = 3, 3, 16, 5
        assert f(*p, big, 1, 4, Hq, Hkv, 400, 256, 16, 128, None) == -2, (Hq, Hkv)
    for page in (1, 8, 48, 100, 512):
        assert f(*p, big, 1, 4, 8, 2, 400, 256, page, 128, None) == -2, page
    assert f(*p, big, 65536, 2, 256, 256, 4, 1, 16, 64, None) == -2  # 2^24 workgroups of 256 threads: one past what a grid dimension takes
    assert f(*p, big, 1, 2, 8, 2, 400, 1 << 24, 256, 64, None) == -2  # max_pages page = 2^32
    # S > 1: a null workspace, and one too small by a single byte
    a = list(p)
    a[7] = None
    assert f(*a, 0, *split, None) == -1
    assert f(*p, need - 1, *split, None) == -1
    assert f(*p, 0, *split, None) == -1
    assert f(*p, -1, *split, None) == -1


def test_plan_grid(built):
    m = built.manifest
    seen = set()
    for (B, T, Hq, Hkv, mp, page, D) in grid():
        G, Nmax = Hq // Hkv, mp * page
        rc, S, C, need = _plan(B, T, Hq, Hkv, mp, page, D)
        assert rc == 0, (B, T, Hq, Hkv, mp, page, D)
        assert (S, C, need) == mr.plan(B, T, Hq, Hkv, mp, page, D), (B, T, Hq, Hkv, mp, page, D, S, C, need)
        assert S >= 1 and S * C >= Nmax > (S - 1) * C and C % max(page, mr.KEY_STEP) == 0, (B, T, Hq, Hkv, mp, page, D, S, C)
        assert need == (B * T * Hq * S * (D + 2) * 4 if S > 1 else 0)
        assert (S, C) == mr.plan(B, 1, Hq, Hkv, mp, page, D)[:2]  # T does not enter the split
        if T == TS[-1] or mp == 63:
            assert built.fa2_decode_paged_multi_plan(B, T, Hq, Hkv, mp, page, D) == (S, C, need)
            t = m.describe_decode_paged_multi(B, T, Hq, Hkv, mp, page, D)
            tiles = -(-T * G // mr.TILE_ROWS)
            assert t.startswith("fa2_decode_paged_multi<D=%d,MT=%d> T=%d G=%d S=%d C=%d page=%d:" % (D, tiles, T, G, S, C, page)), t
            assert ("; then fa2_decode_combine<D=%d>" % D in t) == (S > 1), t
            assert "v_mfma_f32_16x16x32_f16" in t and t.endswith("deterministic"), t
            if S > 1:
                assert "workspace %d bytes" % need in t, t
        seen.add((D, 1 if S == 1 else 3 if S >= 3 else 2))
    for D in (64, 128):
        assert (D, 1) in seen and (D, 3) in seen, sorted(seen)
    for dims in ((1, 2, 8, 8, 4, 16, 96), (1, 2, 3, 1, 4, 16, 64), (1, 2, 8, 8, 4, 48, 64), (1, 2, 8, 3, 4, 16, 64), (0, 2, 8, 8, 4, 16, 64),
                 (1, 9, 8, 8, 4, 16, 64), (1, 0, 8, 8, 4, 16, 64)):
        with pytest.raises(ValueError):
            m.describe_decode_paged_multi(*dims)


def test_plan_errors_of_the_python_entry(built):
    f = built.fa2_decode_paged_multi_plan
    with pytest.raises(RuntimeError, match=r"T 9 not supported \(1 … 8\)"):
        f(1, 9, 8, 8, 4, 16, 64)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi: headdim 96"):
        f(1, 2, 8, 8, 4, 16, 96)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi: group size 3"):
        f(1, 2, 3, 1, 4, 16, 64)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi: page size 48"):
        f(1, 2, 8, 8, 4, 48, 64)
    with pytest.raises(RuntimeError, match="no multiple"):
        f(1, 2, 8, 3, 4, 16, 64)
    with pytest.raises(RuntimeError):
        f(1, 0, 8, 8, 4, 16, 64)


def test_reference_agrees_with_the_single_query_reference_at_one_token():
    torch.manual_seed(5)
    B, Hkv, G, page, mp, D = 3, 2, 2, 16, 4, 64
    q = torch.randn(B, Hkv * G, D).half()
    k, v = torch.randn(B, Hkv, mp * page, D).half(), torch.randn(B, Hkv, mp * page, D).half()
    lens = [1, 33, 64]
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=2)
    O1, L1 = pr.ref_decode_paged(q, kp, vp, bt, lens)
    O, L = mr.ref_decode_paged_multi(q.view(B, 1, Hkv * G, D), kp, vp, bt, lens)
    assert torch.equal(O[:, 0], O1) and torch.equal(L[:, 0], L1)
    # T > 1: token t of a call with length len is the single query of a call with length len - (T - 1 - t)
    T = 3
    qt = torch.randn(B, T, Hkv * G, D).half()
    lens = [2, 33, 64]
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=3)
    O, L = mr.ref_decode_paged_multi(qt, kp, vp, bt, lens)
    for t in range(T):
        Ot, Lt = pr.ref_decode_paged(qt[:, t].contiguous(), kp, vp, bt, [n - (T - 1 - t) for n in lens])
        assert torch.equal(O[:, t], Ot) and torch.equal(L[:, t], Lt), t
    assert bool((O[0, 0] == 0).all()) and L[0, 0].tolist() == [float("-inf")] * (Hkv * G)  # n(0, 0) = 2 - 2 = 0


def test_reference_is_the_brute_force_masked_softmax_on_a_tiny_case():
    torch.manual_seed(11)
    B, T, Hkv, G, page, mp, D = 2, 3, 1, 2, 16, 2, 64
    P = 7
    q = torch.randn(B, T, Hkv * G, D).half()
    kp, vp = torch.randn(P, Hkv, page, D).half(), torch.randn(P, Hkv, page, D).half()
    bt = torch.tensor([[5, 1], [3, 6]], dtype=torch.int32)
    lens = [2, 21]
    O, L = mr.ref_decode_paged_multi(q, kp, vp, bt, lens)
    for b in range(B):
        rows_k = torch.stack([kp[int(bt[b, j // page]), 0, j % page] for j in range(lens[b])]).double()
        rows_v = torch.stack([vp[int(bt[b, j // page]), 0, j % page] for j in range(lens[b])]).double()
        for h in range(Hkv * G):
            s = (q[b, :, h].double() @ rows_k.T) / D ** 0.5  # [T, len]
            pos = lens[b] - T + torch.arange(T)  # the position of query t
            mask = torch.arange(lens[b])[None, :] <= pos[:, None]
            s = s.masked_fill(~mask, float("-inf"))
            for t in range(T):
                if not bool(mask[t].any()):
                    assert bool((O[b, t, h] == 0).all()) and L[b, t, h].item() == float("-inf")
                    continue
                o1 = torch.softmax(s[t], dim=0) @ rows_v
                assert (O[b, t, h] - o1).abs().max().item() <= 1e-12 and abs(L[b, t, h].item() - torch.logsumexp(s[t], dim=0).item()) <= 1e-12
    assert mr.visible([2, 21, -4, 99], 3, 32) == [0, 1, 2, 19, 20, 21, 0, 0, 0, 30, 31, 32]


def test_register_dataflow_model_of_one_wave_step():
    """flash_attn_decode_paged_multi.cuh in numpy, with the instruction models of test_fragment_layout_model.py: one wave, one 32-key step, one row
    tile. K and Q fragments are plain 16-byte pieces of rows, S^T leaves key 4 g4 + r of block kb in register r, P^T packs the two blocks into the
    8 k-slots of a lane, and the V^T fragment is two transposing reads 16 rows apart from the un-swizzled image with 2 D + 32 byte rows. The
    causal edge runs through the step and rows at the end are zero queries."""
    rng = np.random.default_rng(7)
    for D in (64, 128):
        KS, DB, VROW = D // 32, D // 16, 2 * D + 32
        q, k, v = rng.standard_normal((16, D)), rng.standard_normal((32, D)), rng.standard_normal((32, D))
        nvis = np.array([32 - (15 - i) if i < 13 else 0 for i in range(16)])  # keys each query row sees; rows 13 .. 15 are padding
        q[13:] = 0
        lane = np.arange(64)
        i16, g4 = lane & 15, lane >> 4
        img = np.zeros(32 * VROW // 2)
        for l in range(64):  # the lane's 16-byte stores: row i16 (+ 16 kb), bytes 64 ks + 16 g4
            for kb in range(2):
                for ks in range(KS):
                    a = ((16 * kb + i16[l]) * VROW + 64 * ks + 16 * g4[l]) // 2
                    img[a:a + 8] = v[16 * kb + i16[l], 32 * ks + 8 * g4[l]:32 * ks + 8 * g4[l] + 8]
        st = np.zeros((2, 64, 4))
        for kb in range(2):
            for ks in range(KS):
                kf = np.array([k[16 * kb + i16[l], 32 * ks + 8 * g4[l]:32 * ks + 8 * g4[l] + 8] for l in range(64)])
                qf = np.array([q[i16[l], 32 * ks + 8 * g4[l]:32 * ks + 8 * g4[l] + 8] for l in range(64)])
                st[kb] = mfma_16x16x32(kf, qf, st[kb])
        sc = np.full((64, 8), -np.inf)
        for l in range(64):
            for e in range(8):
                if 4 * g4[l] + 16 * (e >> 2) + (e & 3) < nvis[i16[l]]:
                    sc[l, e] = st[e >> 2, l, e & 3]
        mx = np.array([max(sc[16 * g + j].max() for g in range(4)) for j in range(16)])
        ms = np.where(np.isinf(mx), 0.0, mx)
        pf = np.exp2(sc - ms[i16][:, None])
        l_row = np.array([sum(pf[16 * g + j].sum() for g in range(4)) for j in range(16)])
        v_ld = (4 * g4 + (i16 >> 2)) * VROW + 8 * (i16 & 3)
        out = np.zeros((16, D))
        for db in range(DB):
            vf = np.concatenate([ds_read_b64_tr_b16(img, v_ld + 32 * db), ds_read_b64_tr_b16(img, v_ld + 32 * db + 16 * VROW)], axis=1)
            want = np.array([[v[16 * (e >> 2) + 4 * g4[l] + (e & 3), 16 * db + i16[l]] for e in range(8)] for l in range(64)])
            assert np.array_equal(vf, want), (D, db)
            ot = mfma_16x16x32(vf, pf, np.zeros((64, 4)))
            for l in range(64):
                out[i16[l], 16 * db + 4 * g4[l]:16 * db + 4 * g4[l] + 4] = ot[l]
        for j in range(13):
            s = q[j] @ k[:nvis[j]].T
            p = np.exp2(s - s.max())
            assert np.abs(out[j] / l_row[j] - (p @ v[:nvis[j]]) / p.sum()).max() < 1e-9, (D, j)
        assert np.all(out[13:] == 0) and np.all(l_row[13:] == 0)
        assert lds_halves(img, 0, 8).tolist() == v[0, :8].tolist()
        # bank check of the transposing read (bank = byte address / 4 mod 64, per 32-lane half): the 8-byte pieces of a half cover 64 distinct banks
        for half in range(2):
            banks = {((a + 4 * x) // 4) % 64 for a in v_ld[32 * half:32 * half + 32] for x in range(2)}
            assert len(banks) == 64, (D, half)


def test_names_stay_off_the_manifest_surface(built):
    m = built.manifest
    names = {e.name for e in m.ENTRIES}
    for n in NAMES:
        assert n not in names and n.replace("cln_", "") not in names
    gen = open(os.path.join(ROOT, "include", "cln_amd.h")).read()
    assert not any(n + "(" in gen for n in NAMES)


def test_multi_kernels_in_the_product_library_are_exactly_the_plannable_ones(built):
    from cuda_learn_notes_amd import _loader
    linked = {k for k in dk.linked(_loader.so_path("libcln_amd.so")) if k[0] in ("fa2_decode_paged_multi", "fa2_decode_combine")}
    plannable = set()
    for (B, T, Hq, Hkv, mp, page, D) in grid():
        if mp == 63:
            plannable |= dk.named(built.manifest.describe_decode_paged_multi(B, T, Hq, Hkv, mp, page, D))
    assert len(plannable) == 2 * 4 + 2, sorted(plannable)  # D x row tiles, and the two combines
    assert linked == plannable, sorted(linked ^ plannable)


def test_kernels_run_both_products_on_the_matrix_pipe_and_keep_registers(tmp_path):
    import kernel_resources as kr
    kernels, s = kr.report(os.path.join(CSRC, "flash_attn_decode_paged_multi.hip"), keep=str(tmp_path))
    ks = [k for k in kernels if "fa2pm::" in k["demangled"] or "fa2d::" in k["demangled"]]
    assert len(ks) == 2 * 4 + 2 and len(kernels) == len(ks), [k["demangled"] for k in kernels]  # D x row tiles, and the two combines
    text = open(s).read()
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "atomic" not in body, k["demangled"]
        if "fa2_decode_paged_multi_kernel" in k["demangled"]:
            assert "v_mfma_f32_16x16x32_f16" in body and "ds_read_b64_tr_b16" in body and "global_load_dwordx4" in body, k["demangled"]
            assert k["vgpr"] <= 512, k  # .vgpr_count is the unified file: architectural and accumulation registers together
        else:
            assert "v_mfma" not in body, k["demangled"]
