"""CPU: the decode attention entries (include/cln_amd_ext.h: cln_fa2_decode_plan, cln_fa2_decode; csrc/flash_attn_decode.hip) -- header,
exports, argument checks before any device access, the split plan against its Python mirror and the cln_describe text, the fp64 reference of
tests/decode_reference.py, "linked == plannable" for the fa2d:: kernels, and their code (no spill, no scratch, no MFMA). No GPU needed: hipcc
cross-compiles."""
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
import decode_kernels as dk  # noqa: E402
import decode_reference as dr  # noqa: E402

NAMES = ("cln_fa2_decode_plan", "cln_fa2_decode")
BHS = ((1, 1), (1, 8), (3, 5), (8, 32), (64, 32))  # B H = 1, 8, 15, 256, 2048
NMAXS = (1, 63, 64, 1000, 4096, 65536)


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_both_prototypes(tmp_path, lang, cc):
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*p1)(int, int, int, int, int*, int*, long long*) = cln_fa2_decode_plan;\n"
                   "int (*d1)(const void*, const void*, const void*, const int*, void*, float*, void*, long long, int, int, int, int, void*)"
                   " = cln_fa2_decode;\n"
                   "int main(void) { return p1 && d1 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _decode():
    fn = _lib().cln_fa2_decode
    fn.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_longlong] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def _plan(B, H, Nmax, D):
    fn = _lib().cln_fa2_decode_plan
    fn.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3
    fn.restype = ctypes.c_int
    s, c, w = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
    rc = fn(B, H, Nmax, D, ctypes.addressof(s), ctypes.addressof(c), ctypes.addressof(w))
    return rc, s.value, c.value, w.value


def test_product_library_and_package_export_the_entries(built):
    lib = _lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    from cuda_learn_notes_amd import host
    for n in ("fa2_decode", "fa2_decode_plan"):
        assert hasattr(built, n) and hasattr(host, n), n


def test_decode_checks_arguments_before_any_device_access(built):
    f = _decode()
    p = [0x10000 * (i + 1) for i in range(7)]  # q, k, v, seqlens, o, lse, workspace: never dereferenced, every call below fails its checks first
    big = 1 << 40
    split = (1, 8, 4096, 128)  # a shape whose plan splits the keys
    rc, S, C, need = _plan(*split)
    assert rc == 0 and S > 1 and need > 0
    for i in (0, 1, 2, 3, 4):  # a null required pointer
        a = list(p)
        a[i] = None
        assert f(*a, big, *split, None) == -1, i
    for i in (0, 1, 2, 4, 5, 6):  # 16-byte alignment
        a = list(p)
        a[i] = p[i] + 8
        assert f(*a, big, *split, None) == -1, i
    a = list(p)
    a[3] = p[3] + 2  # seqlens: 4-byte alignment
    assert f(*a, big, *split, None) == -1
    for out in (4, 5, 6):  # an output equal to an input or to another output
        for src in range(7):
            if src != out:
                a = list(p)
                a[out] = p[src]
                assert f(*a, big, *split, None) == -1, (out, src)
    for dims in ((0, 1, 256, 64), (1, 0, 256, 64), (1, 1, 0, 64), (1, 1, 256, 0), (1, -2, 256, 64), (-1, 1, 256, 128)):
        assert f(*p, big, *dims, None) == -1, dims
    for D in (32, 96, 256, 512):
        assert f(*p, big, 1, 8, 256, D, None) == -2, D
    assert f(*p, big, 65536, 65536, 256, 64, None) == -2  # grid size
    assert f(*p, big, 65536, 256, 1, 64, None) == -2  # 2^24 workgroups of 256 threads: one past what a grid dimension takes
    # S > 1: a null workspace, and one too small by a single byte
    a = list(p)
    a[6] = None
    assert f(*a, 0, *split, None) == -1
    assert f(*p, need - 1, *split, None) == -1
    assert f(*p, 0, *split, None) == -1
    assert f(*p, -1, *split, None) == -1


@pytest.mark.parametrize("Nmax", [1, 63, 1000])
def test_plan_accepts_any_cache_length(built, Nmax):
    for D in (64, 128):
        rc, S, C, need = _plan(2, 8, Nmax, D)
        assert rc == 0 and S >= 1 and S * C >= Nmax, (Nmax, D, rc, S, C)
        assert built.fa2_decode_plan(2, 8, Nmax, D) == (S, C, need)
    for dims in ((0, 1, 64, 64), (1, 1, 0, 64), (1, 1, 64, -1)):
        assert _plan(*dims)[0] == -1, dims
    assert _plan(1, 1, 64, 96)[0] == -2
    assert _plan(65536, 65536, 64, 64)[0] == -2
    with pytest.raises(RuntimeError, match="headdim 96"):
        built.fa2_decode_plan(1, 1, 64, 96)


def _sdpa64(q, k, v):
    """fp64 softmax(q K^T / sqrt(D)) V and its log-sum-exp for one head: q [D], k, v [n, D]."""
    s = (k.double() @ q.double()) / q.numel() ** 0.5
    return torch.softmax(s, dim=0) @ v.double(), torch.logsumexp(s, dim=0)


def _reference_matches(ref, lens_of):
    torch.manual_seed(11)
    B, H, Nmax, D = 3, 2, 37, 64
    q = torch.randn(B, H, D).half()
    k, v = torch.randn(B, H, Nmax, D).half(), torch.randn(B, H, Nmax, D).half()
    lens = [1, 20, Nmax]
    O, L = ref(q, k, v, lens)
    for b in range(B):
        n = lens_of(lens[b])
        for h in range(H):
            o1, l1 = _sdpa64(q[b, h], k[b, h, :n], v[b, h, :n])
            if (O[b, h] - o1).abs().max().item() > 1e-12 or abs(L[b, h].item() - l1.item()) > 1e-12:
                return False
    return True


def test_reference_is_the_plain_softmax_on_the_sliced_cache():
    assert _reference_matches(dr.ref_decode, lambda n: n)
    # clamping, and the empty sequence
    q, k, v = torch.randn(4, 1, 64).half(), torch.randn(4, 1, 9, 64).half(), torch.randn(4, 1, 9, 64).half()
    q[3], k[3], v[3] = q[2], k[2], v[2]
    O, L = dr.ref_decode(q, k, v, [0, -3, 9, 16])
    assert torch.equal(O[0], torch.zeros(1, 64, dtype=torch.float64)) and torch.equal(O[1], O[0])
    assert L[0].item() == float("-inf") and L[1].item() == float("-inf")
    assert torch.equal(O[2], O[3]) and torch.equal(L[2], L[3])


def test_a_reference_that_reads_one_key_too_many_is_caught():
    def broken(q, k, v, lens):  # j <= len
        return dr.ref_decode(q, k, v, [n + 1 for n in lens])

    assert not _reference_matches(broken, lambda n: n)


def test_plan_grid(built):
    m = built.manifest
    seen = set()
    for D in (64, 128):
        step = dr.key_step(D)
        for (B, H) in BHS:
            for Nmax in NMAXS:
                rc, S, C, need = _plan(B, H, Nmax, D)
                assert rc == 0, (B, H, Nmax, D)
                assert (S, C, need) == dr.plan(B, H, Nmax, D), (B, H, Nmax, D, S, C, need)
                assert S * C >= Nmax and (S - 1) * C < Nmax and C % step == 0 and S >= 1, (B, H, Nmax, D, S, C)
                assert need == (B * H * S * (D + 2) * 4 if S > 1 else 0)
                t = m.describe("cln_fa2_decode", (B, H, Nmax, D), 2)
                assert t.startswith("fa2_decode<D=%d> S=%d C=%d:" % (D, S, C)), t
                assert ("; then fa2_decode_combine<D=%d>" % D in t) == (S > 1), t
                assert "deterministic" in t and "[one pipeline: stages ignored]" in t, t
                if S > 1:
                    assert "workspace %d bytes" % need in t, t
                for st in (1, 2, 3):
                    assert not m.stages_honoured("cln_fa2_decode", (B, H, Nmax, D), st)
                seen.add((D, 1 if S == 1 else 3 if S >= 3 else 2))
    for D in (64, 128):
        assert (D, 1) in seen and (D, 3) in seen, sorted(seen)
    for dims in ((1, 8, 256, 32), (1, 8, 256, 96), (1, 8, 256, 256)):
        with pytest.raises(ValueError):
            m.describe("cln_fa2_decode", dims, 2)


def test_plan_depends_on_the_shape_alone_and_fills_the_chip_or_stops_splitting(built):
    # B H alone fills the chip, or the cache is short: one split
    assert _plan(64, 32, 65536, 128)[1] == 1
    assert _plan(1, 1, 256, 64)[1] == 1 and _plan(1, 1, 63, 128)[1] == 1
    # few heads and a long cache: the cap on S
    assert _plan(1, 1, 65536, 64)[1] == dr.MAX_SPLITS


def test_names_stay_off_the_manifest_surface(built):
    m = built.manifest
    names = {e.name for e in m.ENTRIES}
    for n in NAMES:
        assert n not in names and n.replace("cln_", "") not in names
    gen = open(os.path.join(ROOT, "include", "cln_amd.h")).read()
    assert not any(n + "(" in gen for n in NAMES)
    fast = open(os.path.join(CSRC, "pyext", "cln_fastcall.c")).read()
    assert "fa2_decode" not in fast


def test_fa2d_kernels_in_the_product_library_are_exactly_the_plannable_ones(built):
    from cuda_learn_notes_amd import _loader
    linked = {k for k in dk.linked(_loader.so_path("libcln_amd.so")) if k[0] in ("fa2_decode", "fa2_decode_combine")}
    plannable = set()
    for D in (32, 64, 96, 128, 256):
        for (B, H) in BHS:
            for Nmax in NMAXS:
                try:
                    plannable |= dk.named(built.manifest.describe("cln_fa2_decode", (B, H, Nmax, D), 2))
                except ValueError:
                    continue
    assert len(plannable) == 4, sorted(plannable)
    assert linked == plannable, sorted(linked ^ plannable)


def test_fa2d_kernels_keep_registers_and_use_no_matrix_core(tmp_path):
    import kernel_resources as kr
    kernels, s = kr.report(os.path.join(CSRC, "flash_attn_decode.hip"), keep=str(tmp_path))
    ks = [k for k in kernels if "fa2d::" in k["demangled"]]
    assert len(ks) == 4 and len(kernels) == 4, [k["demangled"] for k in kernels]
    text = open(s).read()
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["agpr"] == 0, k
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "v_mfma" not in body and "atomic" not in body, k["demangled"]
        if "fa2_decode_kernel" in k["demangled"]:
            assert "global_load_dwordx4" in body and k["vgpr"] <= 128, k  # 16-byte loads; at least four waves per SIMD
