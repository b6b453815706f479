"""CPU: the FP8 paged KV-cache append entries (include/cln_amd_ext.h: cln_kv_append_paged_fp8, cln_kv_append_paged_fp8_describe;
csrc/kv_append_paged_fp8.hip) -- header, exports, every status code before any device access (the scale pointers among them), the describe text,
the Python entry's messages, the quantiser of tests/fp8_kv_reference.py proved code by code, the reference against brute force, and the kernels'
code (no spill, no scratch, no LDS, no atomics, 16-byte loads, 8-byte pool stores, the packed e4m3 conversion and an IEEE division). No GPU
needed: hipcc cross-compiles."""
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

NAMES = ("cln_kv_append_paged_fp8", "cln_kv_append_paged_fp8_describe")
PAGES = (16, 32, 64, 128, 256)


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_both_prototypes(tmp_path, lang, cc):
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*a1)(const void*, const void*, void*, void*, const int*, const int*, const float*, const float*, const void*, void*,"
                   " const float*, int, int, int, int, int, int, int, int, int, int, void*) = cln_kv_append_paged_fp8;\n"
                   "int (*t1)(int, int, int, int, int, int, int, int, char*, int) = cln_kv_append_paged_fp8_describe;\n"
                   "int main(void) { return a1 && t1 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _append():
    fn = _lib().cln_kv_append_paged_fp8
    fn.argtypes = [ctypes.c_void_p] * 11 + [ctypes.c_int] * 10 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def _describe(*dims):
    fn = _lib().cln_kv_append_paged_fp8_describe
    fn.argtypes = [ctypes.c_int] * 8 + [ctypes.c_char_p, ctypes.c_int]
    fn.restype = ctypes.c_int
    buf = ctypes.create_string_buffer(1024)
    rc = fn(*dims, buf, 1024)
    return rc, buf.value.decode()


def test_product_library_and_package_export_the_entries(built):
    lib = _lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    from cuda_learn_notes_amd import host
    assert hasattr(built, "kv_append_paged_fp8") and hasattr(host, "kv_append_paged_fp8")
    assert hasattr(built.manifest, "describe_kv_append_paged_fp8")


def test_names_stay_off_the_manifest_surface(built):
    m = built.manifest
    names = {e.name for e in m.ENTRIES}
    for n in NAMES:
        assert n not in names and n.replace("cln_", "") not in names
    gen = open(os.path.join(ROOT, "include", "cln_amd.h")).read()
    assert not any(n + "(" in gen for n in NAMES)


# k_new, v_new, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, q, q_out, rope_table: never dereferenced, every call below fails its
# checks first
PTR = [0x10000 * (i + 1) for i in range(11)]
DIMS = (2, 3, 8, 2, 40, 6, 16, 128, 4096)  # B, T, Hq, Hkv, P, max_pages, page, D, max_pos
BAD_D = (2, 3, 8, 2, 40, 6, 16, 96, 4096)  # the same with an unsupported D: what a call that passed every -1 check ends on


def _no_rope(p):
    return p[:8] + [None, None, None]


def test_append_checks_arguments_before_any_device_access(built):
    f = _append()
    p = list(PTR)
    # every call that is complete but for an unsupported D ends on -2: the -1 checks below are what fails, not something else
    assert f(*p, *BAD_D, 1, None) == -2 and f(*p, *BAD_D, 2, None) == -2 and f(*_no_rope(p), *BAD_D, 0, None) == -2
    assert f(*p[:8], None, None, p[10], *BAD_D, 1, None) == -2  # a rotation of K alone
    for mode in (0, 1, 2):
        base = _no_rope(p) if mode == 0 else list(p)
        for i in range(8):  # a null required pointer, the scales among them
            a = list(base)
            a[i] = None
            assert f(*a, *DIMS, mode, None) == -1, (mode, i)
        for i in (0, 1, 2, 3) + ((8, 9) if mode else ()):  # 16-byte alignment
            a = list(base)
            a[i] = base[i] + 8
            assert f(*a, *DIMS, mode, None) == -1, (mode, i)
        for i in (4, 5, 6, 7) + ((10,) if mode else ()):  # block_table, seqlens, k_scale, v_scale, rope_table: 4-byte alignment, and no more
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
    for i in (8, 9, 10):  # mode 0 takes none of q, q_out, rope_table
        a = _no_rope(p)
        a[i] = p[i]
        assert f(*a, *DIMS, 0, None) == -1, i
    for mode in (1, 2):
        assert f(*p[:10], None, *DIMS, mode, None) == -1  # no table
        assert f(*p[:8], p[8], None, p[10], *DIMS, mode, None) == -1  # q without q_out
        assert f(*p[:8], None, p[9], p[10], *DIMS, mode, None) == -1  # q_out without q
        for max_pos in (0, -1):
            assert f(*p, *DIMS[:8], max_pos, mode, None) == -1, max_pos
    assert f(*_no_rope(p), *BAD_D[:8], 0, 0, None) == -2  # max_pos is of no concern without a rotation
    # aliasing: q_out == q passes the alias check (the call then ends on the unsupported D), every other equality is -1
    a = list(p)
    a[9] = p[8]
    assert f(*a, *BAD_D, 1, None) == -2 and f(*a, *BAD_D, 2, None) == -2
    for out in (2, 3, 9):  # an output equal to an input (the scales among them) or to another output
        for src in range(11):
            if src != out and (out, src) != (9, 8) and (out, src) != (8, 9):
                a = list(p)
                a[out] = p[src]
                assert f(*a, *DIMS, 1, None) == -1, (out, src)
    for (out, src) in ((2, 3), (2, 0), (3, 1), (2, 4), (3, 5), (2, 6), (3, 7), (3, 6)):
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
                    assert text == m.describe_kv_append_paged_fp8(B, T, Hq, Hkv, mp, page, D, mode)
                    assert text == m.describe_kv_append_paged_fp8(B, T, Hq, Hkv, mp, page, D, ("none", "half", "interleaved")[mode])
                    assert text.startswith("kv_append_paged_fp8<D=%d,ROPE=%d> T=%d page=%d: one launch, no workspace" % (D, mode, T, page)), text
                    assert text.endswith("deterministic") and "e4m3" in text and "8-byte plain stores" in text, text
                    rows = 2 * Hkv + (Hq if mode else 0)
                    y = -(-rows * (D // 16 if mode == 1 else D // 8) // 256)
                    assert "%d x %d workgroups of 256 threads" % (B * T, y) in text, text
    rc, text = _describe(1, 1, 8, 2, 4, 16, 64, 1)
    fn = _lib().cln_kv_append_paged_fp8_describe
    fn.argtypes, fn.restype = [ctypes.c_int] * 8 + [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    small = ctypes.create_string_buffer(b"\xff" * 24, 24)
    assert fn(1, 1, 8, 2, 4, 16, 64, 1, small, 16) == 15 and small.raw[:16] == text[:15].encode() + b"\0" and small.raw[16:] == b"\xff" * 8
    assert fn(1, 1, 8, 2, 4, 16, 64, 1, None, 16) == -1 and fn(1, 1, 8, 2, 4, 16, 64, 1, small, 0) == -1
    for dims in ((1, 1, 8, 8, 4, 16, 96, 1), (1, 1, 8, 8, 4, 48, 64, 1), (1, 1, 8, 3, 4, 16, 64, 1), (0, 1, 8, 8, 4, 16, 64, 1),
                 (1, 0, 8, 8, 4, 16, 64, 1), (1, 1, 8, 8, 4, 16, 64, 3), (1, 1, 8, 8, 1 << 23, 256, 64, 0), (1, 1, 8, 8, 4, 16, 64, "neox")):
        with pytest.raises(ValueError):
            m.describe_kv_append_paged_fp8(*dims)


class _Fake:
    """What the Python entry looks at before it asks for a pointer: enough of a tensor to reach the checks under test without a GPU."""
    is_cuda = True

    def __init__(self, dtype, *shape):
        self.dtype, self.shape, self.device = dtype, torch.Size(shape), "cuda:0"

    def dim(self):
        return len(self.shape)


def test_error_messages_of_the_python_entry(built, monkeypatch):
    f = built.kv_append_paged_fp8
    h, i32, f32 = torch.float16, torch.int32, torch.float32
    t = lambda *s: torch.zeros(*s, dtype=h)  # noqa: E731
    p8 = lambda *s: torch.zeros(*s, dtype=torch.uint8).view(f8.F8)  # noqa: E731
    args = (t(2, 3, 2, 64), t(2, 3, 2, 64), p8(9, 2, 16, 64), p8(9, 2, 16, 64), torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32),
            torch.ones(2), torch.ones(2))
    with pytest.raises(RuntimeError, match="kv_append_paged_fp8: rope 'neox' not supported"):
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

    def call(D=64, page=16, Hq=4, Hkv=2, pool=f8.F8, sdt=f32, ns=None):
        ns = Hkv if ns is None else ns
        a = (_Fake(h, 2, 3, Hkv, D), _Fake(h, 2, 3, Hkv, D), _Fake(pool, 9, Hkv, page, D), _Fake(pool, 9, Hkv, page, D), _Fake(i32, 2, 4),
             _Fake(i32, 2), _Fake(sdt, ns), _Fake(sdt, ns))
        f(*a, q=_Fake(h, 2, 3, Hq, D), q_out=_Fake(h, 2, 3, Hq, D), rope_table=_Fake(f32, 8, D), rope="interleaved")
    with pytest.raises(RuntimeError, match="values must be"):  # fp16 pools are the other entry's
        call(pool=h)
    with pytest.raises(RuntimeError, match="values must be"):
        call(pool=torch.float8_e5m2)
    with pytest.raises(RuntimeError, match="values must be"):
        call(sdt=h)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):  # a per-tensor scale is given as the same value Hkv times
        call(ns=1)
    with pytest.raises(RuntimeError, match="kv_append_paged_fp8: headdim 96 not supported"):
        call(D=96)
    with pytest.raises(RuntimeError, match="kv_append_paged_fp8: page size 48 not supported"):
        call(page=48)
    with pytest.raises(RuntimeError, match="kv_append_paged_fp8: 4 query heads are no multiple of 3 KV heads"):
        call(Hkv=3)
    with pytest.raises(AttributeError, match="data_ptr"):  # a supported shape gets as far as the pointers
        call()


# ---------------------------------------------------------------- the quantiser, code by code

def _codes():
    c = torch.arange(256, dtype=torch.uint8)
    return c[(c & 0x7F) != 0x7F]  # without the two NaN codes


def test_every_code_round_trips_through_quantize_at_several_scales():
    c = _codes()
    for s in (1.0, 0.25, 8.0, 2.0 ** -7):  # powers of two: dequantize in fp32 is exact, and so is the product with the reciprocal
        scale = torch.tensor(s)
        x = f8.dequantize(c.view(f8.F8), scale)
        assert bool(torch.isfinite(x).all()) and x.abs().max().item() == 448.0 * s
        assert torch.equal(f8.bits(f8.quantize(x, scale)), c), s
    # ... and an fp16 input of the kernel: every e4m3 value is an fp16 value
    x = c.view(f8.F8).to(torch.float16)
    assert torch.equal(f8.bits(f8.quantize(x, torch.tensor(1.0))), c)
    assert torch.equal(f8.dequantize(c.view(f8.F8), torch.tensor(3.0), torch.float64), c.view(f8.F8).double() * 3.0)


def test_ties_go_to_even_subnormals_and_saturation():
    one = torch.tensor(1.0)
    q = lambda *v: f8.quantize(torch.tensor(v), one).float().tolist()  # noqa: E731
    # normal range, spacing 2 at 16 .. 32: 17 and 19 are ties
    assert q(17.0, 19.0, 21.0, 23.0, 17.0001, 18.9999) == [16.0, 20.0, 20.0, 24.0, 18.0, 18.0]
    assert q(-17.0, -19.0) == [-16.0, -20.0]
    # subnormals: spacing 2^-9 below 2^-6; ties at odd multiples of 2^-10
    u = 2.0 ** -9
    assert q(u, 0.5 * u, 1.5 * u, 2.5 * u, 0.5001 * u, 0.4999 * u, 7 * u, 7.5 * u, 8 * u) == [u, 0.0, 2 * u, 2 * u, u, 0.0, 7 * u, 8 * u, 8 * u]
    assert f8.bits(f8.quantize(torch.tensor([0.0, -0.0, -0.5 * u]), one)).tolist() == [0x00, 0x80, 0x80]
    # beyond the largest finite value: 448, never the NaN code
    big = f8.quantize(torch.tensor([449.0, 463.0, 464.0, 1e9, 3e38, -449.0, -1e9]), one)
    assert f8.bits(big).tolist() == [0x7E] * 5 + [0xFE] * 2 and big.float().abs().tolist() == [448.0] * 7
    # the clamp is on x / scale: 448 scale is the largest value kept
    s = torch.tensor(0.37)
    assert f8.quantize(torch.tensor([1e4, 448 * 0.37, -1e4]), s).float().tolist() == [448.0, 448.0, -448.0]
    # a scale per row broadcasts: the same input under four scales
    x = torch.full((4, 3), 5.0)
    assert f8.quantize(x, torch.tensor([[0.25], [0.5], [1.0], [2.0]])).float()[:, 0].tolist() == [20.0, 10.0, 5.0, 2.5]


def test_quantize_is_the_three_fp32_operations_of_the_kernel():
    """x * (1 / s) with the correctly rounded fp32 reciprocal: the reference's reciprocal is that one, whichever way it is formed."""
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(1 << 16, generator=g) * 3).half()
    s = torch.rand(1 << 16, generator=g) + 0.05
    a = f8.quantize(x, s)
    inv = (1.0 / s.double()).float()  # the correctly rounded reciprocal, formed another way
    b = (x.float() * inv).clamp(-448, 448).to(f8.F8)
    assert torch.equal(f8.bits(a), f8.bits(b))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_reference_is_the_brute_force_scatter_on_a_tiny_case(mode):
    """kv_append_reference's tiny case: B = 4, T = 3, page 16, two pages per sequence, lengths 17, 2, 40, 34."""
    import kv_append_reference as kr
    g = torch.Generator().manual_seed(3)
    B, T, Hkv, Hq, page, mp, D, P = 4, 3, 2, 4, 16, 2, 64, 10
    k_new, v_new, q = (torch.randn(B, T, H, D, generator=g).half() for H in (Hkv, Hkv, Hq))
    kp = torch.randint(0, 256, (P, Hkv, page, D), generator=g, dtype=torch.uint8).view(f8.F8)
    vp = torch.randint(0, 256, (P, Hkv, page, D), generator=g, dtype=torch.uint8).view(f8.F8)
    bt = torch.tensor([[5, 1], [3, 6], [0, 9], [8, 2]], dtype=torch.int32)
    lens = [17, 2, 40, 34]
    ks, vs = torch.tensor([0.01, 0.02]), torch.tensor([0.04, 0.005])
    table = (torch.rand(32, D, generator=g) * 2 - 1) if mode else None
    r = f8.ref_append_fp8(k_new, v_new, kp, vp, bt, lens, ks, vs, q if mode else None, table, mode)
    assert r.live == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (3, 0)]
    want_k, want_v = f8.bits(kp).clone(), f8.bits(vp).clone()
    for (b, t, pos) in ((0, 0, 14), (0, 1, 15), (0, 2, 16), (1, 1, 0), (1, 2, 1), (3, 0, 31)):
        pg, row = int(bt[b, pos // 16]), pos % 16
        for h in range(Hkv):
            y = kr.rotate(k_new[b, t, h], table[pos] if mode else None, mode)[0]
            for d in range(D):
                zk = torch.tensor(float(y[d]), dtype=torch.float32) * (torch.tensor(1.0) / ks[h])
                zv = v_new[b, t, h, d].float() * (torch.tensor(1.0) / vs[h])
                want_k[pg, h, row, d] = f8.bits(zk.clamp(-448, 448).to(f8.F8))
                want_v[pg, h, row, d] = f8.bits(zv.clamp(-448, 448).to(f8.F8))
    assert torch.equal(f8.bits(r.k_pages), want_k) and torch.equal(f8.bits(r.v_pages), want_v)
    assert not torch.equal(want_k, f8.bits(kp)) and (mode == 0) == (r.q_rot is None)
    # nothing live: the pools come back byte for byte
    none = f8.ref_append_fp8(k_new, v_new, kp, vp, bt, [0, -5, 1 << 31, -(1 << 31)], ks, vs, None, table, mode)
    assert torch.equal(f8.bits(none.k_pages), f8.bits(kp)) and torch.equal(f8.bits(none.v_pages), f8.bits(vp))
    # the bound: at y = 0 it is the subnormal floor, at a normal value the half ulp plus the cover
    assert f8.bound(torch.tensor(0.0), 0.5, torch.tensor(0.0)).item() == 2.0 ** -11
    assert f8.bound(torch.tensor(-2.0), 1.0, torch.tensor(3.0)).item() == 2.0 ** -3 + 2.0 ** -10 + 3 * 2.0 ** -21


def test_make_pool_poisons_with_the_nan_byte_and_the_decode_reference_dequantises():
    import paged_decode_reference as pr
    g = torch.Generator().manual_seed(4)
    B, Hkv, G, page, mp, D = 2, 2, 2, 16, 4, 64
    ks, vs = torch.tensor([0.5, 0.02]), torch.tensor([0.03, 2.0])
    k, v = torch.randn(B, Hkv, mp * page, D, generator=g), torch.randn(B, Hkv, mp * page, D, generator=g)
    k8, v8 = f8.quantize(k, f8.per_head(ks)), f8.quantize(v, f8.per_head(vs))
    lens = [17, 64]
    kp, vp, bt = f8.make_pool(k8, v8, page, lens, seed=5)
    P = kp.shape[0]
    live = {int(bt[b, i]) for b in range(B) for i in range(-(-lens[b] // page))}
    assert kp.dtype == f8.F8 and len(live) == 6 and P - 1 not in live
    assert all(bool((f8.bits(kp[s]) == 0x7F).all()) and bool((f8.bits(vp[s]) == 0x7F).all()) for s in range(P) if s not in live)
    assert bool(torch.isnan(kp[P - 1].float()).all())
    q = torch.randn(B, Hkv * G, D, generator=g).half()
    O, L = f8.ref_decode_paged_fp8(q, kp, vp, ks, vs, bt, lens)
    # by hand: the fp32 dequantised dense caches through the dense fp64 reference
    import decode_reference as dr
    kd = (k8.float() * ks.view(1, -1, 1, 1)).repeat_interleave(G, dim=1)
    vd = (v8.float() * vs.view(1, -1, 1, 1)).repeat_interleave(G, dim=1)
    O2, L2 = dr.ref_decode(q, kd, vd, lens)
    assert bool(torch.isfinite(O).all()) and torch.equal(O, O2) and torch.equal(L, L2)
    # the scales matter: swapping them is another answer
    O3, _ = f8.ref_decode_paged_fp8(q, kp, vp, ks.flip(0), vs, bt, lens)
    assert not torch.equal(O, O3)
    assert pr.plan(1, 8, 1, 4096, 16, 64)[0] == f8.plan(1, 8, 1, 4096, 16, 64)[0] == dr.MAX_SPLITS


def test_kernels_keep_registers_and_store_eight_bytes(tmp_path):
    import kernel_resources as kres
    kernels, s = kres.report(os.path.join(CSRC, "kv_append_paged_fp8.hip"), keep=str(tmp_path))
    assert len(kernels) == 6 and all("kva::kv_append_paged_fp8_kernel<" in k["demangled"] for k in kernels), [k["demangled"] for k in kernels]  # D x mode
    text = open(s).read()
    for k in kernels:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, k
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "atomic" not in body and "v_mfma" not in body, k["demangled"]
        assert "global_load_dwordx4" in body and "global_store_dwordx2" in body and "v_cvt_pk_fp8_f32" in body, k["demangled"]
        assert "v_div_fixup_f32" in body, k["demangled"]  # 1 / scale is the IEEE division, not the bare reciprocal approximation
        # the pools get whole 8-byte pieces, plain stores; nothing narrower anywhere
        assert "global_store_byte" not in body and "global_store_short" not in body and "global_store_dword " not in body and " nt" not in body, k["demangled"]
