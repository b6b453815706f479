"""CPU: the packed variable-length paged entries (include/cln_amd_ext.h: cln_fa2_prefill_paged_varlen, cln_kv_append_paged_varlen and their
describe entries; csrc/flash_attn_prefill_paged_varlen.hip, csrc/kv_append_paged_varlen.hip) -- header, exports, every status code before any
device access, the describe texts against their Python mirrors (tests/prefill_varlen_reference.py), the slot mapping against a brute-force
enumeration of (sequence, tile) pairs, the Python entries' messages, and the kernels' code (MFMA on both products, the transposing LDS read, no
spill, no scratch, the registers of the fixed-T kernels; the append's 16-byte pieces and no atomics). No GPU needed: hipcc cross-compiles."""
import ctypes
import os
import random
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
import paged_decode_reference as pr  # noqa: E402
import prefill_varlen_reference as vr  # noqa: E402

NAMES = ("cln_fa2_prefill_paged_varlen", "cln_fa2_prefill_paged_varlen_describe", "cln_kv_append_paged_varlen",
         "cln_kv_append_paged_varlen_describe")
LDS_PER_CU = 160 * 1024


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_prototypes(tmp_path, lang, cc):
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*a1)(const void*, const void*, const void*, const int*, const int*, const int*, void*, float*, int, int, int, int, int,"
                   " int, int, int, void*) = cln_fa2_prefill_paged_varlen;\n"
                   "int (*t1)(int, int, int, int, int, int, int, char*, int) = cln_fa2_prefill_paged_varlen_describe;\n"
                   "int (*a2)(const void*, const void*, void*, void*, const int*, const int*, const int*, const void*, void*, const float*, int,"
                   " int, int, int, int, int, int, int, int, int, void*) = cln_kv_append_paged_varlen;\n"
                   "int (*t2)(int, int, int, int, int, int, int, int, char*, int) = cln_kv_append_paged_varlen_describe;\n"
                   "int main(void) { return a1 && t1 && a2 && t2 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _prefill():
    fn = _lib().cln_fa2_prefill_paged_varlen
    fn.argtypes, fn.restype = [ctypes.c_void_p] * 8 + [ctypes.c_int] * 8 + [ctypes.c_void_p], ctypes.c_int
    return fn


def _append():
    fn = _lib().cln_kv_append_paged_varlen
    fn.argtypes, fn.restype = [ctypes.c_void_p] * 10 + [ctypes.c_int] * 10 + [ctypes.c_void_p], ctypes.c_int
    return fn


def _describe(name, n_int, *dims):
    fn = getattr(_lib(), name)
    fn.argtypes, fn.restype = [ctypes.c_int] * n_int + [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    buf = ctypes.create_string_buffer(1280)
    rc = fn(*dims, buf, 1280)
    return rc, buf.value.decode()


def test_product_library_and_package_export_the_entries(built):
    lib = _lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    from cuda_learn_notes_amd import host
    for n in ("fa2_prefill_paged_varlen", "kv_append_paged_varlen"):
        assert hasattr(built, n) and hasattr(host, n), n
    assert hasattr(built.manifest, "describe_prefill_paged_varlen") and hasattr(built.manifest, "describe_kv_append_paged_varlen")
    names = {e.name for e in built.manifest.ENTRIES}
    for n in NAMES:
        assert n not in names and n.replace("cln_", "") not in names


# q, k_pages, v_pages, block_table, seqlens, cu_q, o, lse: never dereferenced, every call below fails its checks first
PTR = [0x10000 * (i + 1) for i in range(8)]
DIMS = (3, 170, 8, 2, 40, 6, 16, 128)  # B, total_q, Hq, Hkv, P, max_pages, page, D
BAD_D = DIMS[:7] + (96,)               # the same with an unsupported D: what a call that passed every -1 check ends on


def test_prefill_checks_arguments_before_any_device_access(built):
    f = _prefill()
    p = list(PTR)
    assert f(*p, *BAD_D, None) == -2 and f(*p[:7], None, *BAD_D, None) == -2  # with and without lse
    for i in range(7):  # a null required pointer, cu_q among them
        a = list(p)
        a[i] = None
        assert f(*a, *DIMS, None) == -1, i
    for i in (0, 1, 2, 6):  # 16-byte alignment
        a = list(p)
        a[i] = p[i] + 8
        assert f(*a, *DIMS, None) == -1, i
    for i in (3, 4, 5, 7):  # block_table, seqlens, cu_q, lse: 4-byte alignment, and no more than that
        a = list(p)
        a[i] = p[i] + 2
        assert f(*a, *DIMS, None) == -1, i
        a[i] = p[i] + 4
        assert f(*a, *BAD_D, None) == -2, i
    for out in (6, 7):  # an output equal to an input (cu_q among them) or to the other output
        for src in range(8):
            if src != out:
                a = list(p)
                a[out] = p[src]
                assert f(*a, *DIMS, None) == -1, (out, src)
    for i in range(8):  # each dimension non-positive: B and total_q among them
        for bad in (0, -2):
            d = list(DIMS)
            d[i] = bad
            assert f(*p, *d, None) == -1, d
    assert f(*p, 3, 170, 8, 3, 40, 6, 16, 128, None) == -1  # Hq % Hkv
    for D in (32, 96, 256, 512):
        assert f(*p, *DIMS[:7], D, None) == -2, D
    for (Hq, Hkv) in ((3, 1), (6, 2), (16, 1), (5, 1)):  # G = 3, 3, 16, 5
        assert f(*p, 3, 170, Hq, Hkv, 40, 6, 16, 128, None) == -2, (Hq, Hkv)
    for page in (1, 8, 48, 100, 512):
        assert f(*p, 3, 170, 8, 2, 40, 6, page, 128, None) == -2, page
    assert f(*p, 3, 170, 8, 2, 40, 1 << 23, 256, 128, None) == -2  # max_pages page = 2^31
    assert f(*p, 1, 1 << 28, 8, 1, 40, 6, 16, 128, None) == -2     # total_q G = 2^31
    assert f(*p, 1, 1 << 27, 64, 8, 40, 6, 16, 64, None) == -2     # 8 KV heads x 2^23 slots: 2^26 workgroups of 256 threads
    assert f(*p, 1 << 24, 1, 8, 8, 40, 6, 16, 64, None) == -2      # the B empty slots count too: 8 x 2^24
    assert _describe(NAMES[1], 7, 2, 1 << 20, 8, 2, 6, 16, 128)[0] > 0  # any total_q that fits


APTR = [0x10000 * (i + 1) for i in range(10)]  # k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, q, q_out, rope_table
ADIMS = (3, 23, 8, 2, 40, 6, 16, 128, 4096)    # B, total_q, Hq, Hkv, P, max_pages, page, D, max_pos
ABAD_D = ADIMS[:7] + (96, 4096)


def _no_rope(p):
    return p[:7] + [None, None, None]


def test_append_checks_arguments_before_any_device_access(built):
    f = _append()
    p = list(APTR)
    assert f(*p, *ABAD_D, 1, None) == -2 and f(*p, *ABAD_D, 2, None) == -2 and f(*_no_rope(p), *ABAD_D, 0, None) == -2
    assert f(*p[:7], None, None, p[9], *ABAD_D, 1, None) == -2  # a rotation of K alone
    for mode in (0, 1, 2):
        base = _no_rope(p) if mode == 0 else list(p)
        for i in range(7):  # a null required pointer, cu_q among them
            a = list(base)
            a[i] = None
            assert f(*a, *ADIMS, mode, None) == -1, (mode, i)
        for i in (0, 1, 2, 3) + ((7, 8) if mode else ()):  # 16-byte alignment
            a = list(base)
            a[i] = base[i] + 8
            assert f(*a, *ADIMS, mode, None) == -1, (mode, i)
        for i in (4, 5, 6) + ((9,) if mode else ()):  # block_table, seqlens, cu_q, rope_table: 4-byte alignment, and no more than that
            a = list(base)
            a[i] = base[i] + 2
            assert f(*a, *ADIMS, mode, None) == -1, (mode, i)
            a[i] = base[i] + 4
            assert f(*a, *ABAD_D, mode, None) == -2, (mode, i)
        for i in range(8):  # each dimension non-positive
            for bad in (0, -2):
                d = list(ADIMS)
                d[i] = bad
                assert f(*base, *d, mode, None) == -1, (mode, d)
        assert f(*base, 3, 23, 8, 3, 40, 6, 16, 128, 4096, mode, None) == -1  # Hq % Hkv
    for i in (7, 8, 9):  # mode 0 takes none of q, q_out, rope_table
        a = _no_rope(p)
        a[i] = p[i]
        assert f(*a, *ADIMS, 0, None) == -1, i
    for mode in (1, 2):
        assert f(*p[:9], None, *ADIMS, mode, None) == -1  # no table
        assert f(*p[:7], p[7], None, p[9], *ADIMS, mode, None) == -1  # q without q_out
        assert f(*p[:7], None, p[8], p[9], *ADIMS, mode, None) == -1  # q_out without q
        for max_pos in (0, -1):
            assert f(*p, *ADIMS[:8], max_pos, mode, None) == -1, max_pos
    # aliasing: q_out == q passes the alias check (the call then ends on the unsupported D), every other equality is -1
    a = list(p)
    a[8] = p[7]
    assert f(*a, *ABAD_D, 1, None) == -2 and f(*a, *ABAD_D, 2, None) == -2
    for out in (2, 3, 8):
        for src in range(10):
            if src != out and (out, src) != (8, 7):
                a = list(p)
                a[out] = p[src]
                assert f(*a, *ADIMS, 1, None) == -1, (out, src)
    for mode in (-1, 3, 7):
        assert f(*p, *ADIMS, mode, None) == -2, mode
    for D in (32, 96, 256, 512):
        assert f(*p, *ADIMS[:7], D, 4096, 1, None) == -2, D
    for page in (1, 8, 48, 100, 512):
        assert f(*p, *ADIMS[:6], page, 128, 4096, 1, None) == -2, page
    assert f(*p, 3, 23, 24, 2, 40, 6, 16, 96, 4096, 1, None) == -2  # G = 12 passes the -1 checks: the append serves any multiple
    assert f(*p, 3, 23, 8, 2, 40, 1 << 23, 256, 128, 4096, 1, None) == -2  # max_pages page = 2^31
    assert f(*p, 3, 1 << 24, 8, 2, 40, 6, 16, 128, 4096, 1, None) == -2     # 2^24 packed rows: one past a grid dimension of 256-thread workgroups
    assert f(*p, 3, 23, 1 << 21, 1 << 20, 40, 6, 16, 128, 4096, 1, None) == -2  # 2^17 workgroups per row in y


def test_describe_texts_match_the_python_mirrors(built):
    m = built.manifest
    for D in (64, 128):
        for G in pr.GROUPS:
            for page in pr.PAGES:
                for (B, tq, Hkv, mp) in ((1, 1, 1, 1), (5, 204, 1, 32), (3, 258, 2, 40), (65, 2112, 8, 300)):
                    Hq = Hkv * G
                    rc, text = _describe(NAMES[1], 7, B, tq, Hq, Hkv, mp, page, D)
                    assert rc == len(text) > 0, (rc, text)
                    assert text == m.describe_prefill_paged_varlen(B, tq, Hq, Hkv, mp, page, D) == vr.describe_prefill_text(B, tq, Hq, Hkv, mp, page, D)
                    S = tq * G // vr.ROW_TILE + B
                    assert text.startswith("fa2_prefill_paged_varlen_mfma<D=%d,G=%d> B=%d total_q=%d page=%d rows=128 keys=64: one launch, no workspace"
                                           % (D, G, B, tq, page)), text
                    assert "%d workgroups of 256 threads (%d KV heads x %d slots" % (Hkv * S, Hkv, S) in text and text.endswith("deterministic")
                    for mode in (0, 1, 2):
                        rc, text = _describe(NAMES[3], 8, B, tq, Hq, Hkv, mp, page, D, mode)
                        assert rc == len(text) > 0, (rc, text)
                        assert text == m.describe_kv_append_paged_varlen(B, tq, Hq, Hkv, mp, page, D, ("none", "half", "interleaved")[mode])
                        assert text == vr.describe_append_text(B, tq, Hq, Hkv, mp, page, D, mode)
                        assert "one launch, no workspace" in text and text.endswith("deterministic")
    # the 64 x T = 1 plus 1 x T = 2048 batch at G = 4: 131 slots for 128 tiles
    assert "(8 KV heads x 131 slots" in m.describe_prefill_paged_varlen(65, 2112, 32, 8, 300, 16, 128)
    for fn, n, dims in ((NAMES[1], 7, (1, 1, 8, 2, 4, 16, 64)), (NAMES[3], 8, (1, 1, 8, 2, 4, 16, 64, 1))):
        rc, text = _describe(fn, n, *dims)
        f = getattr(_lib(), fn)
        small = ctypes.create_string_buffer(b"\xff" * 24, 24)
        assert f(*dims, small, 16) == 15 and small.raw[:16] == text[:15].encode() + b"\0" and small.raw[16:] == b"\xff" * 8
        assert f(*dims, None, 16) == -1 and f(*dims, small, 0) == -1
    for dims in ((1, 2, 8, 8, 4, 16, 96), (1, 2, 3, 1, 4, 16, 64), (1, 2, 8, 8, 4, 48, 64), (1, 2, 8, 3, 4, 16, 64), (0, 2, 8, 8, 4, 16, 64),
                 (1, 0, 8, 8, 4, 16, 64), (1, 2, 8, 8, 1 << 23, 256, 64), (1, 1 << 28, 8, 1, 4, 16, 64)):
        with pytest.raises(ValueError):
            m.describe_prefill_paged_varlen(*dims)
    for dims in ((1, 1, 8, 8, 4, 16, 96, 1), (1, 1, 8, 8, 4, 48, 64, 1), (1, 1, 8, 3, 4, 16, 64, 1), (0, 1, 8, 8, 4, 16, 64, 1),
                 (1, 0, 8, 8, 4, 16, 64, 1), (1, 1, 8, 8, 4, 16, 64, 3), (1, 1, 8, 8, 4, 16, 64, "neox")):
        with pytest.raises(ValueError):
            m.describe_kv_append_paged_varlen(*dims)


def _check_slots(cu, G, total_q):
    """Every (sequence, tile) pair has exactly one slot below S, found by the kernel's rule; at most B slots are empty."""
    B = len(cu) - 1
    S, first, tiles = vr.slots(cu, G, total_q)
    want = [(b, t) for b in range(B) for t in range(-(-(cu[b + 1] - cu[b]) * G // vr.ROW_TILE))]
    got = [vr.slot_owner(cu, G, x) for x in range(S)]
    assert [g for g in got if g is not None] == want, (cu, G)  # in order, none twice, none missing
    assert all(first[b + 1] > first[b] for b in range(B - 1)), (cu, G)  # strictly increasing, also across empty sequences
    # S <= total_q G / 128 + B and the tiles cover (cu[B] - cu[0]) G rows: at most B empty slots, plus those of the rows outside the sequences
    assert got.count(None) <= B + (total_q - (cu[B] - cu[0])) * G // vr.ROW_TILE, (cu, G)
    if cu[0] == 0 and total_q == cu[B]:
        assert S - len(want) <= B
    return S, len(want)


def test_slots_equal_a_brute_force_enumeration_of_sequence_tile_pairs():
    for (_, G, _, _), T in vr.CASES:
        for first, spare in ((0, 5), (3, 5), (0, 0)):
            cu = vr.cu_of(T, first)
            _check_slots(cu, G, cu[-1] + spare)
    assert _check_slots(vr.cu_of([1] * 64 + [2048]), 4, 2112) == (131, 128)
    assert _check_slots(vr.cu_of([2048, 512, 64, 17]), 4, 2641)[0] == 2641 * 4 // 128 + 4
    rng = random.Random(5)
    for _ in range(3000):
        G = rng.choice(pr.GROUPS)
        B = rng.randint(1, 12)
        T = [rng.choice((0, 0, 1, 1, 2, 15, 16, 17, 31, 32, 33, 64, 127, 128, 129, rng.randint(0, 700))) for _ in range(B)]
        cu = vr.cu_of(T, rng.choice((0, 0, 0, 1, 7, 200)))
        _check_slots(cu, G, cu[-1] + rng.choice((0, 0, 1, 5, 130)))


class _Fake:
    """What the Python entry looks at before it asks for a pointer: enough of a tensor to reach the checks under test without a GPU."""
    is_cuda = True

    def __init__(self, dtype, *shape):
        self.dtype, self.shape, self.device = dtype, torch.Size(shape), "cuda:0"

    def dim(self):
        return len(self.shape)


def test_error_messages_of_the_python_entries(built, monkeypatch):
    f, fa = built.fa2_prefill_paged_varlen, built.kv_append_paged_varlen
    h, i32, f32 = torch.float16, torch.int32, torch.float32
    t = lambda *s: torch.zeros(*s, dtype=h)  # noqa: E731
    ints = (torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), torch.zeros(3, dtype=i32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(t(40, 8, 64), t(9, 2, 16, 64), t(9, 2, 16, 64), *ints, t(40, 8, 64))
    with pytest.raises(RuntimeError, match="values must be"):
        f(t(40, 8, 64).float(), t(9, 2, 16, 64), t(9, 2, 16, 64), *ints, t(40, 8, 64))
    args = (t(40, 2, 64), t(40, 2, 64), t(9, 2, 16, 64), t(9, 2, 16, 64)) + ints
    with pytest.raises(RuntimeError, match="kv_append_paged_varlen: rope 'neox' not supported"):
        fa(*args, rope="neox")
    with pytest.raises(RuntimeError, match="kv_append_paged_varlen: rope 'none' takes no q, q_out or rope_table"):
        fa(*args, rope_table=torch.zeros(8, 64))
    with pytest.raises(RuntimeError, match="kv_append_paged_varlen: rope 'half' needs a rope_table"):
        fa(*args, rope="half")
    with pytest.raises(RuntimeError, match="kv_append_paged_varlen: q and q_out are given together"):
        fa(*args, q=t(40, 4, 64), rope_table=torch.zeros(8, 64), rope="half")
    with pytest.raises(RuntimeError, match="no CPU path"):
        fa(*args)
    from cuda_learn_notes_amd import host
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)

    def call(D=64, page=16, Hq=8, Hkv=2, tq=40, **bad):
        a = dict(q=_Fake(h, tq, Hq, D), k=_Fake(h, 9, Hkv, page, D), v=_Fake(h, 9, Hkv, page, D), bt=_Fake(i32, 2, 4), sl=_Fake(i32, 2),
                 cu=_Fake(i32, 3), o=_Fake(h, tq, Hq, D))
        a.update(bad)
        f(a["q"], a["k"], a["v"], a["bt"], a["sl"], a["cu"], a["o"], a.get("lse"))
    for kw in (dict(cu=_Fake(torch.int64, 3)), dict(lse=_Fake(h, 40, 8)), dict(k=_Fake(torch.bfloat16, 9, 2, 16, 64))):
        with pytest.raises(RuntimeError, match="values must be"):
            call(**kw)
    for kw in (dict(cu=_Fake(i32, 2)), dict(cu=_Fake(i32, 4)), dict(cu=_Fake(i32, 3, 1)), dict(v=_Fake(h, 8, 2, 16, 64)), dict(o=_Fake(h, 39, 8, 64)),
               dict(sl=_Fake(i32, 3)), dict(lse=_Fake(f32, 8)), dict(lse=_Fake(f32, 1, 40, 8)), dict(q=_Fake(h, 1, 40, 8, 64))):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            call(**kw)
    with pytest.raises(RuntimeError, match="fa2_prefill_paged_varlen: headdim 96 not supported"):
        call(D=96)
    with pytest.raises(RuntimeError, match=r"fa2_prefill_paged_varlen: group size 3 \(= Hq 6 / Hkv 2\) not supported"):
        call(Hq=6)
    with pytest.raises(RuntimeError, match="fa2_prefill_paged_varlen: page size 48 not supported"):
        call(page=48)
    with pytest.raises(RuntimeError, match="fa2_prefill_paged_varlen: 8 query heads are no multiple of 3 KV heads"):
        call(Hkv=3)
    for tq in (1, 9, 4096):  # a supported shape, whatever total_q is, gets as far as the pointers
        with pytest.raises(AttributeError, match="data_ptr"):
            call(tq=tq)

    def acall(D=64, page=16, Hq=4, Hkv=2, cu=3):
        a = (_Fake(h, 7, Hkv, D), _Fake(h, 7, Hkv, D), _Fake(h, 9, Hkv, page, D), _Fake(h, 9, Hkv, page, D), _Fake(i32, 2, 4), _Fake(i32, 2),
             _Fake(i32, cu))
        fa(*a, q=_Fake(h, 7, Hq, D), q_out=_Fake(h, 7, Hq, D), rope_table=_Fake(f32, 8, D), rope="interleaved")
    with pytest.raises(RuntimeError, match="kv_append_paged_varlen: headdim 96 not supported"):
        acall(D=96)
    with pytest.raises(RuntimeError, match="kv_append_paged_varlen: page size 48 not supported"):
        acall(page=48)
    with pytest.raises(RuntimeError, match="kv_append_paged_varlen: 4 query heads are no multiple of 3 KV heads"):
        acall(Hkv=3)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):
        acall(cu=2)
    with pytest.raises(AttributeError, match="data_ptr"):
        acall()


def test_attention_kernels_run_both_products_on_the_matrix_pipe_and_keep_the_parents_registers(tmp_path):
    import kernel_resources as kres
    kernels, s = kres.report(os.path.join(CSRC, "flash_attn_prefill_paged_varlen.hip"), keep=str(tmp_path))
    assert len(kernels) == 2 and all("fa2pp::fa2_prefill_paged_varlen_mfma<" in k["demangled"] for k in kernels), [k["demangled"] for k in kernels]
    text = open(s).read()
    for k in kernels:
        print(k["demangled"][:60], {x: k[x] for x in ("vgpr", "sgpr", "lds")})
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        assert 0 < 2 * k["lds"] <= LDS_PER_CU, k  # two workgroups resident per CU ...
        assert k["vgpr"] <= 256, k                # ... whose 8 waves, two per SIMD, share the 512 registers of a lane
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "v_mfma_f32_16x16x32_f16" in body and "ds_read_b64_tr_b16" in body and "global_load_dwordx4" in body, k["demangled"]
        assert "atomic" not in body, k["demangled"]


def test_append_kernels_keep_registers_and_move_sixteen_bytes(tmp_path):
    import kernel_resources as kres
    kernels, s = kres.report(os.path.join(CSRC, "kv_append_paged_varlen.hip"), keep=str(tmp_path))
    assert len(kernels) == 6 and all("kva::kv_append_paged_varlen_rows<" in k["demangled"] for k in kernels), [k["demangled"] for k in kernels]
    text = open(s).read()
    for k in kernels:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0 and k["lds"] == 0, k
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "atomic" not in body, k["demangled"]
        assert "global_load_dwordx4" in body and "global_store_dwordx4" in body, k["demangled"]
        assert "global_store_short" not in body and "global_store_dword " not in body and " nt" not in body, k["demangled"]  # whole pieces, plain stores
