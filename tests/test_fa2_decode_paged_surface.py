"""CPU: the paged decode attention entries (include/cln_amd_ext.h: cln_fa2_decode_paged_plan, cln_fa2_decode_paged,
cln_fa2_decode_paged_describe; csrc/flash_attn_decode_paged.hip) -- header, exports, argument checks before any device access, the plan against its
Python mirror and the describe text, the references of tests/paged_decode_reference.py, "linked == plannable" for the paged kernels, and their
code (no spill, no scratch, 16-byte loads). No GPU needed: hipcc cross-compiles."""
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
CSRC = os.path.join(ROOT, "cuda-learn-notes_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "cuda-learn-notes_amd", "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decode_kernels as dk  # noqa: E402
import decode_reference as dr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402

NAMES = ("cln_fa2_decode_paged_plan", "cln_fa2_decode_paged", "cln_fa2_decode_paged_describe")
# the plan grid: (B, Hkv) with B Hkv = 1, 8, 15, 256, 2048; every G; max_pages and pages that give Nmax from 16 to 65536
BHKV = ((1, 1), (1, 8), (3, 5), (8, 32), (64, 32))
MAXPAGES = (1, 3, 63, 256)


def grid():
    for D in (64, 128):
        for (B, Hkv) in BHKV:
            for G in pr.GROUPS:
                for page in pr.PAGES:
                    for mp in MAXPAGES:
                        yield B, Hkv * G, Hkv, mp, page, D


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_three_prototypes(tmp_path, lang, cc):
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*p1)(int, int, int, int, int, int, int*, int*, long long*) = cln_fa2_decode_paged_plan;\n"
                   "int (*d1)(const void*, const void*, const void*, const int*, const int*, void*, float*, void*, long long, int, int, int, int, int,"
                   " int, int, void*) = cln_fa2_decode_paged;\n"
                   "int (*t1)(int, int, int, int, int, int, char*, int) = cln_fa2_decode_paged_describe;\n"
                   "int main(void) { return p1 && d1 && t1 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _paged():
    fn = _lib().cln_fa2_decode_paged
    fn.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_longlong] + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def _plan(B, Hq, Hkv, max_pages, page, D):
    fn = _lib().cln_fa2_decode_paged_plan
    fn.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p] * 3
    fn.restype = ctypes.c_int
    s, c, w = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
    rc = fn(B, Hq, Hkv, max_pages, page, D, ctypes.addressof(s), ctypes.addressof(c), ctypes.addressof(w))
    return rc, s.value, c.value, w.value


def test_product_library_and_package_export_the_entries(built):
    lib = _lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    from cuda_learn_notes_amd import host
    for n in ("fa2_decode_paged", "fa2_decode_paged_plan"):
        assert hasattr(built, n) and hasattr(host, n), n
    assert hasattr(built.manifest, "describe_decode_paged")


def test_paged_decode_checks_arguments_before_any_device_access(built):
    f = _paged()
    # q, k_pages, v_pages, block_table, seqlens, o, lse, workspace: never dereferenced, every call below fails its checks first
    p = [0x10000 * (i + 1) for i in range(8)]
    big = 1 << 40
    split = (1, 8, 2, 400, 256, 16, 128)  # B, Hq, Hkv, P, max_pages, page, D: a shape whose plan splits the keys
    rc, S, C, need = _plan(1, 8, 2, 256, 16, 128)
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
    for i in range(7):  # each dim non-positive
        for bad in (0, -2):
            d = list(split)
            d[i] = bad
            assert f(*p, big, *d, None) == -1, d
    assert f(*p, big, 1, 8, 3, 400, 256, 16, 128, None) == -1  # Hq % Hkv
    for D in (32, 96, 256, 512):
        assert f(*p, big, 1, 8, 2, 400, 256, 16, D, None) == -2, D
    for (Hq, Hkv) in ((3, 1), (6, 2), (16, 1), (5, 1)):  # G = 3, 3, 16, 5
        assert f(*p, big, 1, Hq, Hkv, 400, 256, 16, 128, None) == -2, (Hq, Hkv)
    for page in (1, 8, 48, 100, 512):
        assert f(*p, big, 1, 8, 2, 400, 256, page, 128, None) == -2, page
    assert f(*p, big, 65536, 256, 256, 4, 1, 16, 64, None) == -2  # 2^24 workgroups of 256 threads: one past what a grid dimension takes
    assert f(*p, big, 1, 8, 2, 400, 1 << 24, 256, 64, None) == -2  # max_pages page = 2^32
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
    for (B, Hq, Hkv, mp, page, D) in grid():
        G, Nmax, step = Hq // Hkv, mp * page, dr.key_step(D)
        rc, S, C, need = _plan(B, Hq, Hkv, mp, page, D)
        assert rc == 0, (B, Hq, Hkv, mp, page, D)
        assert (S, C, need) == pr.plan(B, Hq, Hkv, mp, page, D), (B, Hq, Hkv, mp, page, D, S, C, need)
        assert built.fa2_decode_paged_plan(B, Hq, Hkv, mp, page, D) == (S, C, need)
        assert S >= 1 and S * C >= Nmax > (S - 1) * C and C % max(page, step) == 0, (B, Hq, Hkv, mp, page, D, S, C)
        assert need == (B * Hq * S * (D + 2) * 4 if S > 1 else 0)
        t = m.describe_decode_paged(B, Hq, Hkv, mp, page, D)
        assert t.startswith("fa2_decode_paged<D=%d,G=%d> S=%d C=%d page=%d:" % (D, G, S, C, page)), t
        assert ("; then fa2_decode_combine<D=%d>" % D in t) == (S > 1), t
        assert t.endswith("deterministic"), t
        if S > 1:
            assert "workspace %d bytes" % need in t, t
        seen.add((D, 1 if S == 1 else 3 if S >= 3 else 2))
    for D in (64, 128):
        assert (D, 1) in seen and (D, 3) in seen, sorted(seen)
    for dims in ((1, 8, 8, 4, 16, 96), (1, 3, 1, 4, 16, 64), (1, 8, 8, 4, 48, 64), (1, 8, 3, 4, 16, 64), (0, 8, 8, 4, 16, 64)):
        with pytest.raises(ValueError):
            m.describe_decode_paged(*dims)


def test_plan_counts_workgroups_per_kv_head_and_never_reads_the_lengths(built):
    # the same B Hkv gives the same split whatever G is; B Hkv alone fills the chip, or the cache is short: one split
    for D in (64, 128):
        assert len({_plan(2, 4 * G, 4, 256, 16, D)[1:3] for G in pr.GROUPS}) == 1
        assert _plan(64, 32, 32, 4096, 16, D)[1] == 1 and _plan(64, 256, 32, 4096, 16, D)[1] == 1
        assert _plan(1, 8, 1, 16, 16, D)[1] == 1
        assert _plan(1, 8, 1, 4096, 16, D)[1] == dr.MAX_SPLITS
    with pytest.raises(RuntimeError, match="headdim 96"):
        built.fa2_decode_paged_plan(1, 8, 8, 4, 16, 96)
    with pytest.raises(RuntimeError, match="group size 3"):
        built.fa2_decode_paged_plan(1, 3, 1, 4, 16, 64)
    with pytest.raises(RuntimeError, match="page size 48"):
        built.fa2_decode_paged_plan(1, 8, 8, 4, 48, 64)
    with pytest.raises(RuntimeError, match="no multiple"):
        built.fa2_decode_paged_plan(1, 8, 3, 4, 16, 64)


def _sdpa64(q, k, v):
    """fp64 softmax(q K^T / sqrt(D)) V and its log-sum-exp for one head: q [D], k, v [n, D]."""
    s = (k.double() @ q.double()) / q.numel() ** 0.5
    return torch.softmax(s, dim=0) @ v.double(), torch.logsumexp(s, dim=0)


def _reference_matches(ref):
    """ref against the plain fp64 softmax on rows gathered by hand, for a shuffled table with G = 2."""
    torch.manual_seed(13)
    B, Hkv, G, page, mp, D = 3, 2, 2, 16, 3, 64
    P = 14
    q = torch.randn(B, Hkv * G, D).half()
    kp, vp = torch.randn(P, Hkv, page, D).half(), torch.randn(P, Hkv, page, D).half()
    bt = torch.tensor([[9, 2, 12], [4, 13, 0], [7, 5, 11]], dtype=torch.int32)
    lens = [1, 20, mp * page]
    O, L = ref(q, kp, vp, bt, lens)
    for b in range(B):
        for h in range(Hkv * G):
            rows_k = torch.stack([kp[int(bt[b, j // page]), h // G, j % page] for j in range(lens[b])])
            rows_v = torch.stack([vp[int(bt[b, j // page]), h // G, j % page] for j in range(lens[b])])
            o1, l1 = _sdpa64(q[b, h], rows_k, rows_v)
            if (O[b, h] - o1).abs().max().item() > 1e-12 or abs(L[b, h].item() - l1.item()) > 1e-12:
                return False
    return True


def test_reference_is_the_plain_softmax_on_hand_gathered_rows():
    assert _reference_matches(pr.ref_decode_paged)


def test_a_reference_that_ignores_the_table_is_caught():
    def broken(q, kp, vp, bt, lens):  # identity mapping: sequence b's i-th page is pool page b max_pages + i
        ident = torch.arange(bt.numel(), dtype=torch.int32).view_as(bt)
        return pr.ref_decode_paged(q, kp, vp, ident, lens)

    assert not _reference_matches(broken)


def test_gather_follows_live_entries_only_and_make_pool_round_trips():
    torch.manual_seed(3)
    B, Hkv, page, mp, D = 2, 2, 16, 4, 64
    k, v = torch.randn(B, Hkv, mp * page, D).half(), torch.randn(B, Hkv, mp * page, D).half()
    lens = [17, 64]
    for order in ("identity", "shuffle"):
        kp, vp, bt = pr.make_pool(k, v, page, lens, order=order, seed=5)
        P = kp.shape[0]
        live = {int(bt[b, i]) for b in range(B) for i in range(-(-lens[b] // page))}
        assert len(live) == 2 + 4 and P >= 3 * len(live) // 2 + 1 and P - 1 not in live
        assert all(int(x) == P - 1 for x in bt[0, 2:]) and bool(torch.isnan(kp[P - 1]).all())
        assert all(bool(torch.isnan(kp[s]).all()) and bool(torch.isnan(vp[s]).all()) for s in range(P) if s not in live)
        gk, gv = pr.gather(kp, bt, lens), pr.gather(vp, bt, lens)
        assert torch.equal(gk[0, :, :32], k[0, :, :32]) and torch.equal(gv[1], v[1]) and bool((gk[0, :, 32:] == 0).all())
    # clamping, and the empty sequence
    q = torch.randn(B, Hkv * 2, D).half()
    kp, vp, bt = pr.make_pool(k, v, page, [64, 64], seed=1)
    O, L = pr.ref_decode_paged(q, kp, vp, bt, [0, 99])
    O2, L2 = pr.ref_decode_paged(q, kp, vp, bt, [-4, 64])
    assert bool((O[0] == 0).all()) and L[0].tolist() == [float("-inf")] * 4 and torch.equal(O, O2) and torch.equal(L, L2)


def test_names_stay_off_the_manifest_surface(built):
    m = built.manifest
    names = {e.name for e in m.ENTRIES}
    for n in NAMES:
        assert n not in names and n.replace("cln_", "") not in names
    gen = open(os.path.join(ROOT, "include", "cln_amd.h")).read()
    assert not any(n + "(" in gen for n in NAMES)
    fast = open(os.path.join(CSRC, "pyext", "cln_fastcall.c")).read()
    assert "fa2_decode_paged" not in fast


def test_fa2p_kernels_in_the_product_library_are_exactly_the_plannable_ones(built):
    from cuda_learn_notes_amd import _loader
    linked = {k for k in dk.linked(_loader.so_path("libcln_amd.so")) if k[0] in ("fa2_decode_paged", "fa2_decode_combine")}
    plannable = set()
    for (B, Hq, Hkv, mp, page, D) in grid():
        plannable |= dk.named(built.manifest.describe_decode_paged(B, Hq, Hkv, mp, page, D))
    assert len(plannable) == 2 * len(pr.GROUPS) + 2, sorted(plannable)
    assert linked == plannable, sorted(linked ^ plannable)


def test_fa2p_kernels_keep_registers_and_load_16_bytes(tmp_path):
    import kernel_resources as kr
    kernels, s = kr.report(os.path.join(CSRC, "flash_attn_decode_paged.hip"), keep=str(tmp_path))
    ks = [k for k in kernels if "fa2d::" in k["demangled"]]
    assert len(ks) == 2 * len(pr.GROUPS) + 2 and len(kernels) == len(ks), [k["demangled"] for k in kernels]
    text = open(s).read()
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "v_mfma" not in body and "atomic" not in body, k["demangled"]
        if "fa2_decode_kernel" in k["demangled"]:
            assert "global_load_dwordx4" in body, k
            if re.search(r"<\d+, 1, ", k["demangled"]):
                assert k["vgpr"] <= 128, k  # G = 1: at least four waves per SIMD, like fa2d::
            assert k["vgpr"] + k["agpr"] <= 512, k
