"""CPU: the paged KV-cache append entries (include/cln_amd_ext.h: cln_kv_append_paged, cln_kv_append_paged_describe; csrc/kv_append_paged.hip) --
header, exports, every status code before any device access, the describe text, the Python entry's messages, the rope table, the reference of
tests/kv_append_reference.py against brute force, and the kernels' code (no spill, no scratch, no atomics, 16-byte loads and stores). No GPU
needed: hipcc cross-compiles."""
import ctypes
import math
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
import kv_append_reference as kr  # noqa: E402

NAMES = ("cln_kv_append_paged", "cln_kv_append_paged_describe")
PAGES = (16, 32, 64, 128, 256)


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_both_prototypes(tmp_path, lang, cc):
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*a1)(const void*, const void*, void*, void*, const int*, const int*, const void*, void*, const float*, int, int, int, int,"
                   " int, int, int, int, int, int, void*) = cln_kv_append_paged;\n"
                   "int (*t1)(int, int, int, int, int, int, int, int, char*, int) = cln_kv_append_paged_describe;\n"
                   "int main(void) { return a1 && t1 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _append():
    fn = _lib().cln_kv_append_paged
    fn.argtypes = [ctypes.c_void_p] * 9 + [ctypes.c_int] * 10 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def _describe(*dims):
    fn = _lib().cln_kv_append_paged_describe
    fn.argtypes = [ctypes.c_int] * 8 + [ctypes.c_char_p, ctypes.c_int]
    fn.restype = ctypes.c_int
    buf = ctypes.create_string_buffer(768)
    rc = fn(*dims, buf, 768)
    return rc, buf.value.decode()


def test_product_library_and_package_export_the_entries(built):
    lib = _lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    from cuda_learn_notes_amd import host
    for n in ("kv_append_paged", "kv_append_rope_table"):
        assert hasattr(built, n) and hasattr(host, n), n
    assert hasattr(built.manifest, "describe_kv_append_paged")


def test_names_stay_off_the_manifest_surface(built):
    m = built.manifest
    names = {e.name for e in m.ENTRIES}
    for n in NAMES + ("cln_kv_append_rope_table",):
        assert n not in names and n.replace("cln_", "") not in names
    gen = open(os.path.join(ROOT, "include", "cln_amd.h")).read()
    assert not any(n + "(" in gen for n in NAMES)
    fast = open(os.path.join(CSRC, "pyext", "cln_fastcall.c")).read()
    assert "kv_append" not in fast


# k_new, v_new, k_pages, v_pages, block_table, seqlens, q, q_out, rope_table: never dereferenced, every call below fails its checks first
PTR = [0x10000 * (i + 1) for i in range(9)]
DIMS = (2, 3, 8, 2, 40, 6, 16, 128, 4096)  # B, T, Hq, Hkv, P, max_pages, page, D, max_pos
BAD_D = (2, 3, 8, 2, 40, 6, 16, 96, 4096)  # the same with an unsupported D: what a call that passed every -1 check ends on


def _no_rope(p):
    return p[:6] + [None, None, None]


def test_append_checks_arguments_before_any_device_access(built):
    f = _append()
    p = list(PTR)
    # every call that is complete but for an unsupported D ends on -2: the -1 checks below are what fails, not something else
    assert f(*p, *BAD_D, 1, None) == -2 and f(*p, *BAD_D, 2, None) == -2 and f(*_no_rope(p), *BAD_D, 0, None) == -2
    assert f(*p[:6], None, None, p[8], *BAD_D, 1, None) == -2  # a rotation of K alone
    for mode in (0, 1, 2):
        base = _no_rope(p) if mode == 0 else list(p)
        for i in range(6):  # a null required pointer
            a = list(base)
            a[i] = None
            assert f(*a, *DIMS, mode, None) == -1, (mode, i)
        for i in (0, 1, 2, 3) + ((6, 7) if mode else ()):  # 16-byte alignment
            a = list(base)
            a[i] = base[i] + 8
            assert f(*a, *DIMS, mode, None) == -1, (mode, i)
        for i in (4, 5) + ((8,) if mode else ()):  # block_table, seqlens, rope_table: 4-byte alignment, and no more than that
            a = list(base)
            a[i] = base[i] + 2
            assert f(*a, *DIMS, mode, None) == -1, (mode, i)
            a[i] = base[i] + 4
            assert f(*a, *BAD_D, mode, None) == -2, (mode, i)
        for i in range(8):  # each dimension non-positive
            for bad in (0, -2):
                d = list(DIMS)
                d[i] = bad
                assert f(*base, *d, mode, None) == -1, (mode, d)
        assert f(*base, 2, 3, 8, 3, 40, 6, 16, 128, 4096, mode, None) == -1  # Hq % Hkv
    # the pointer rules of rope_mode
    for i in (6, 7, 8):  # mode 0 takes none of q, q_out, rope_table
        a = _no_rope(p)
        a[i] = p[i]
        assert f(*a, *DIMS, 0, None) == -1, i
    for mode in (1, 2):
        assert f(*p[:8], None, *DIMS, mode, None) == -1  # no table
        assert f(*p[:6], p[6], None, p[8], *DIMS, mode, None) == -1  # q without q_out
        assert f(*p[:6], None, p[7], p[8], *DIMS, mode, None) == -1  # q_out without q
        for max_pos in (0, -1):
            assert f(*p, *DIMS[:8], max_pos, mode, None) == -1, max_pos
    assert f(*_no_rope(p), *BAD_D[:8], 0, 0, None) == -2  # max_pos is of no concern without a rotation
    # aliasing: q_out == q passes the alias check (the call then ends on the unsupported D), every other equality is -1
    a = list(p)
    a[7] = p[6]
    assert f(*a, *BAD_D, 1, None) == -2 and f(*a, *BAD_D, 2, None) == -2
    assert f(*a, *DIMS[:7], 0, 4096, 1, None) == -1  # ... and a bad dimension behind it is still found
    for out in (2, 3, 7):
        for src in range(9):
            if src != out and (out, src) != (7, 6):
                a = list(p)
                a[out] = p[src]
                assert f(*a, *DIMS, 1, None) == -1, (out, src)
                a = list(p)
                a[src] = p[out]
                if (src, out) != (7, 6) and (src, out) != (6, 7):
                    assert f(*a, *DIMS, 1, None) == -1, (out, src)
    a = _no_rope(p)
    for (out, src) in ((2, 3), (2, 0), (3, 1), (2, 4), (3, 5)):
        a = _no_rope(p)
        a[out] = p[src]
        assert f(*a, *DIMS, 0, None) == -1, (out, src)
    # -2: the unsupported shapes
    for mode in (-1, 3, 7):
        assert f(*p, *DIMS, mode, None) == -2, mode
    for D in (32, 96, 256, 512):
        assert f(*p, *DIMS[:7], D, 4096, 1, None) == -2, D
    for page in (1, 8, 48, 100, 512):
        assert f(*p, *DIMS[:6], page, 128, 4096, 1, None) == -2, page
    assert f(*p, 2, 3, 8, 2, 40, 1 << 23, 256, 128, 4096, 1, None) == -2  # max_pages page = 2^31
    assert f(*p, 1 << 12, 1 << 12, 8, 2, 40, 6, 16, 128, 4096, 1, None) == -2  # B T = 2^24 workgroups of 256 threads: one past a grid dimension
    assert f(*p, 2, 3, 1 << 21, 1 << 20, 40, 6, 16, 128, 4096, 1, None) == -2  # 2^22 rows of 8 threads: 2^17 workgroups per token in y


def test_describe_names_the_instantiation_and_matches_the_python_mirror(built):
    m = built.manifest
    for D in (64, 128):
        for mode in (0, 1, 2):
            for page in PAGES:
                for (B, T, Hq, Hkv, mp) in ((1, 1, 1, 1, 1), (3, 19, 6, 3, 3), (4, 512, 32, 8, 64), (256, 1, 16, 2, 7)):
                    rc, text = _describe(B, T, Hq, Hkv, mp, page, D, mode)
                    assert rc == len(text) > 0, (rc, text)
                    assert text == m.describe_kv_append_paged(B, T, Hq, Hkv, mp, page, D, mode)
                    assert text == m.describe_kv_append_paged(B, T, Hq, Hkv, mp, page, D, ("none", "half", "interleaved")[mode])
                    assert text.startswith("kv_append_paged<D=%d,ROPE=%d> T=%d page=%d: one launch, no workspace" % (D, mode, T, page)), text
                    assert text.endswith("deterministic"), text
                    rows = 2 * Hkv + (Hq if mode else 0)
                    y = -(-rows * (D // 16 if mode == 1 else D // 8) // 256)
                    assert "%d x %d workgroups of 256 threads" % (B * T, y) in text, text
    rc, text = _describe(1, 1, 8, 2, 4, 16, 64, 1)
    fn = _lib().cln_kv_append_paged_describe
    fn.argtypes, fn.restype = [ctypes.c_int] * 8 + [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    small = ctypes.create_string_buffer(b"\xff" * 24, 24)
    assert fn(1, 1, 8, 2, 4, 16, 64, 1, small, 16) == 15 and small.raw[:16] == text[:15].encode() + b"\0" and small.raw[16:] == b"\xff" * 8
    assert fn(1, 1, 8, 2, 4, 16, 64, 1, None, 16) == -1 and fn(1, 1, 8, 2, 4, 16, 64, 1, small, 0) == -1
    for dims in ((1, 1, 8, 8, 4, 16, 96, 1), (1, 1, 8, 8, 4, 48, 64, 1), (1, 1, 8, 3, 4, 16, 64, 1), (0, 1, 8, 8, 4, 16, 64, 1),
                 (1, 0, 8, 8, 4, 16, 64, 1), (1, 1, 8, 8, 4, 16, 64, 3), (1, 1, 8, 8, 1 << 23, 256, 64, 0), (1, 1, 8, 8, 4, 16, 64, "neox")):
        with pytest.raises(ValueError):
            m.describe_kv_append_paged(*dims)


class _Fake:
    """What the Python entry looks at before it asks for a pointer: enough of a tensor to reach the checks under test without a GPU."""
    is_cuda = True

    def __init__(self, dtype, *shape):
        self.dtype, self.shape, self.device = dtype, torch.Size(shape), "cuda:0"

    def dim(self):
        return len(self.shape)


def test_error_messages_of_the_python_entry(built, monkeypatch):
    f = built.kv_append_paged
    h, i32 = torch.float16, torch.int32
    t = lambda *s: torch.zeros(*s, dtype=h)  # noqa: E731
    args = (t(2, 3, 2, 64), t(2, 3, 2, 64), t(9, 2, 16, 64), t(9, 2, 16, 64), torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32))
    with pytest.raises(RuntimeError, match="kv_append_paged: rope 'neox' not supported"):
        f(*args, rope="neox")
    with pytest.raises(RuntimeError, match="takes no q, q_out or rope_table"):
        f(*args, rope_table=torch.zeros(8, 64))
    with pytest.raises(RuntimeError, match="needs a rope_table"):
        f(*args, rope="half")
    with pytest.raises(RuntimeError, match="given together"):
        f(*args, q=t(2, 3, 4, 64), rope_table=torch.zeros(8, 64), rope="half")
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(*args)
    with pytest.raises(RuntimeError, match="values must be"):
        f(args[0].float(), *args[1:])
    # the shape messages come behind the device check: tensors that only claim to be on the GPU, and are refused before any pointer is taken
    from cuda_learn_notes_amd import host
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)

    def call(D=64, page=16, Hq=4, Hkv=2):
        a = (_Fake(h, 2, 3, Hkv, D), _Fake(h, 2, 3, Hkv, D), _Fake(h, 9, Hkv, page, D), _Fake(h, 9, Hkv, page, D), _Fake(i32, 2, 4), _Fake(i32, 2))
        f(*a, q=_Fake(h, 2, 3, Hq, D), q_out=_Fake(h, 2, 3, Hq, D), rope_table=_Fake(torch.float32, 8, D), rope="interleaved")
    with pytest.raises(RuntimeError, match="kv_append_paged: headdim 96 not supported"):
        call(D=96)
    with pytest.raises(RuntimeError, match="kv_append_paged: page size 48 not supported"):
        call(page=48)
    with pytest.raises(RuntimeError, match="kv_append_paged: 4 query heads are no multiple of 3 KV heads"):
        call(Hkv=3)
    with pytest.raises(AttributeError, match="data_ptr"):  # a supported shape gets as far as the pointers
        call()


def test_rope_table_is_float64_cos_and_sin_rounded_once(built):
    for (max_pos, D, theta) in ((1, 64, 10000.0), (700, 64, 10000.0), (257, 128, 500000.0)):
        tab = built.kv_append_rope_table(max_pos, D, theta)
        assert tab.dtype == torch.float32 and tab.shape == (max_pos, D) and tab.device.type == "cpu" and tab.is_contiguous()
        for p in sorted({0, min(1, max_pos - 1), min(2, max_pos - 1), max_pos // 2, max_pos - 1}):
            for i in range(D // 2):
                ang = p * theta ** (-2.0 * i / D)
                for got, want in ((tab[p, i].item(), math.cos(ang)), (tab[p, D // 2 + i].item(), math.sin(ang))):
                    # one rounding of a value in [-1, 1] to fp32, and the last bits of pow / cos / sin in float64 at angles below 2^10
                    assert abs(got - want) <= 2.0 ** -24 * abs(want) + 2.0 ** -40, (p, i, got, want)
        assert tab[0, :D // 2].tolist() == [1.0] * (D // 2) and tab[0, D // 2:].tolist() == [0.0] * (D // 2)
    with pytest.raises(RuntimeError):
        built.kv_append_rope_table(0, 64)
    with pytest.raises(RuntimeError):
        built.kv_append_rope_table(8, 63)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_reference_is_the_brute_force_scatter_and_rotation_on_a_tiny_case(mode):
    """B = 4, T = 3, page 16, two pages per sequence: a run that crosses the page boundary (len 17: positions 14, 15, 16), len 2 < T (the first
    token is not live), len 40 > 32 (no token is live), and len 34 (only the first token, at position 31, is live)."""
    g = torch.Generator().manual_seed(3)
    B, T, Hkv, Hq, page, mp, D, P = 4, 3, 2, 4, 16, 2, 64, 10
    k_new, v_new, q = (torch.randn(B, T, H, D, generator=g).half() for H in (Hkv, Hkv, Hq))
    kp, vp = torch.randn(P, Hkv, page, D, generator=g).half(), torch.randn(P, Hkv, page, D, generator=g).half()
    bt = torch.tensor([[5, 1], [3, 6], [0, 9], [8, 2]], dtype=torch.int32)
    lens = [17, 2, 40, 34]
    table = (torch.rand(32, D, generator=g) * 2 - 1) if mode else None
    r = kr.ref_append(k_new, v_new, kp, vp, bt, lens, q if mode else None, table, mode)
    assert r.live == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (3, 0)]
    want_k, want_v = kp.clone(), vp.clone()
    written = set()
    for (b, t, pos) in ((0, 0, 14), (0, 1, 15), (0, 2, 16), (1, 1, 0), (1, 2, 1), (3, 0, 31)):
        pg, row = int(bt[b, pos // 16]), pos % 16
        written.add((pg, row))
        for h in range(Hkv):
            want_v[pg, h, row] = v_new[b, t, h]
            for d in range(D):
                x = float(k_new[b, t, h, d])
                if mode:
                    i, first = (d % 32, d < 32) if mode == 1 else (d // 2, d % 2 == 0)
                    mate = float(k_new[b, t, h, (d + 32) % 64 if mode == 1 else d ^ 1])
                    c, s = float(table[pos, i]), float(table[pos, 32 + i])
                    x = x * c - mate * s if first else mate * s + x * c
                    assert abs(float(r.k_rot[b, t, h, d]) - x) <= 1e-15 * (1 + abs(x)), (b, t, h, d)
                want_k[pg, h, row, d] = x
        for h in range(Hq if mode else 0):
            for d in range(D):
                i, first = (d % 32, d < 32) if mode == 1 else (d // 2, d % 2 == 0)
                x, mate = float(q[b, t, h, d]), float(q[b, t, h, (d + 32) % 64 if mode == 1 else d ^ 1])
                c, s = float(table[pos, i]), float(table[pos, 32 + i])
                val = x * c - mate * s if first else mate * s + x * c
                assert abs(float(r.q_rot[b, t, h, d]) - val) <= 1e-15 * (1 + abs(val)), (b, t, h, d)
                m = abs(x * c) + abs(mate * s) if first else abs(mate * s) + abs(x * c)
                assert abs(float(r.q_mag[b, t, h, d]) - m) <= 1e-15 * (1 + m)
    assert torch.equal(r.k_pages, want_k) and torch.equal(r.v_pages, want_v)
    assert {(int(a), int(b)) for a, b in r.k_live.nonzero()} == written
    dead = [(b, t) for b in range(B) for t in range(T) if (b, t) not in r.live]
    assert all(bool((r.k_rot[b, t] == 0).all()) for (b, t) in dead)
    if mode:
        assert all(bool((r.q_rot[b, t] == 0).all()) for (b, t) in dead)
        # max_pos below the capacity: position 31 is live no more
        r2 = kr.ref_append(k_new, v_new, kp, vp, bt, lens, q, table[:31], mode)
        assert r2.live == r.live[:-1] and torch.equal(r2.k_pages[8], kp[8]) and torch.equal(r2.k_pages[2], kp[2])
    else:
        alive = torch.tensor([[(b, t) in r.live for t in range(T)] for b in range(B)])
        assert r.q_rot is None and torch.equal(r.k_rot, k_new.double() * alive[:, :, None, None])
    assert torch.equal(kp, kr.ref_append(k_new, v_new, kp, vp, bt, [0, -5, 1 << 31, -(1 << 31)], None, table, mode).k_pages)  # nothing live
    # the bound: exact for r = 0, and at a normal fp16 value it is the half ulp plus the fp32 cover
    assert kr.bound(torch.tensor(0.0), torch.tensor(0.0)).item() == 2.0 ** -25
    assert kr.bound(torch.tensor(-2.0), torch.tensor(3.0)).item() == 2.0 ** -10 + 2.0 ** -25 + 3 * 2.0 ** -22


def test_kernels_keep_registers_and_move_sixteen_bytes(tmp_path):
    import kernel_resources as kres
    kernels, s = kres.report(os.path.join(CSRC, "kv_append_paged.hip"), keep=str(tmp_path))
    assert len(kernels) == 6 and all("kva::kv_append_paged_kernel<" in k["demangled"] for k in kernels), [k["demangled"] for k in kernels]  # D x mode
    text = open(s).read()
    for k in kernels:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, k
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "atomic" not in body, k["demangled"]
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, k["demangled"]
        assert "global_store_short" not in body and "global_store_dword " not in body and " nt" not in body, k["demangled"]  # whole pieces, plain stores
