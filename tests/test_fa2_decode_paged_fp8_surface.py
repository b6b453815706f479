"""CPU: the FP8 paged decode attention entries (include/cln_amd_ext.h: cln_fa2_decode_paged_fp8_plan, cln_fa2_decode_paged_fp8,
cln_fa2_decode_paged_fp8_describe; csrc/flash_attn_decode_paged_fp8.hip) -- header, exports, argument checks before any device access (the scale
pointers among them), the plan against its Python mirror (tests/fp8_kv_reference.py) and the describe text, the Python entry's messages, the
kernels linked into the library, and their code (no spill, no scratch, no MFMA, no atomics, 8-byte loads, the packed e4m3 conversion). No GPU
needed: hipcc cross-compiles."""
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
import decode_reference as dr  # noqa: E402
import fp8_kv_reference as f8  # noqa: E402
import paged_decode_reference as pr  # noqa: E402

NAMES = ("cln_fa2_decode_paged_fp8_plan", "cln_fa2_decode_paged_fp8", "cln_fa2_decode_paged_fp8_describe")
# the plan grid of the fp16 entry: (B, Hkv) with B Hkv = 1, 8, 15, 256, 2048; every G; max_pages and pages that give Nmax from 16 to 65536
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
                   "int (*p1)(int, int, int, int, int, int, int*, int*, long long*) = cln_fa2_decode_paged_fp8_plan;\n"
                   "int (*d1)(const void*, const void*, const void*, const int*, const int*, const float*, const float*, void*, float*, void*,"
                   " long long, int, int, int, int, int, int, int, void*) = cln_fa2_decode_paged_fp8;\n"
                   "int (*t1)(int, int, int, int, int, int, char*, int) = cln_fa2_decode_paged_fp8_describe;\n"
                   "int main(void) { return p1 && d1 && t1 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _decode():
    fn = _lib().cln_fa2_decode_paged_fp8
    fn.argtypes = [ctypes.c_void_p] * 10 + [ctypes.c_longlong] + [ctypes.c_int] * 7 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def _plan(B, Hq, Hkv, max_pages, page, D):
    fn = _lib().cln_fa2_decode_paged_fp8_plan
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
    for n in ("fa2_decode_paged_fp8", "fa2_decode_paged_fp8_plan"):
        assert hasattr(built, n) and hasattr(host, n), n
    assert hasattr(built.manifest, "describe_decode_paged_fp8")


def test_names_stay_off_the_manifest_surface(built):
    m = built.manifest
    names = {e.name for e in m.ENTRIES}
    for n in NAMES:
        assert n not in names and n.replace("cln_", "") not in names
    gen = open(os.path.join(ROOT, "include", "cln_amd.h")).read()
    assert not any(n + "(" in gen for n in NAMES)
    fast = open(os.path.join(CSRC, "pyext", "cln_fastcall.c")).read()
    assert "fp8" not in fast


def test_decode_checks_arguments_before_any_device_access(built):
    f = _decode()
    # q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, o, lse, workspace: never dereferenced, every call below fails its checks first
    p = [0x10000 * (i + 1) for i in range(10)]
    big = 1 << 40
    split = (1, 8, 2, 400, 256, 16, 128)  # B, Hq, Hkv, P, max_pages, page, D: a shape whose plan splits the keys
    rc, S, C, need = _plan(1, 8, 2, 256, 16, 128)
    assert rc == 0 and S > 1 and need > 0
    assert f(*p, big, 1, 8, 2, 400, 256, 16, 96, None) == -2  # complete but for D: the -1 checks below are what fails, not something else
    for i in (0, 1, 2, 3, 4, 5, 6, 7):  # a null required pointer, the scales among them
        a = list(p)
        a[i] = None
        assert f(*a, big, *split, None) == -1, i
    a = list(p)
    a[8] = None  # lse may be null
    assert f(*a, big, 1, 8, 2, 400, 256, 16, 96, None) == -2
    for i in (0, 1, 2, 7, 8, 9):  # 16-byte alignment
        a = list(p)
        a[i] = p[i] + 8
        assert f(*a, big, *split, None) == -1, i
    for i in (3, 4, 5, 6):  # block_table, seqlens, k_scale, v_scale: 4-byte alignment, and no more than that
        a = list(p)
        a[i] = p[i] + 2
        assert f(*a, big, *split, None) == -1, i
        a[i] = p[i] + 4
        assert f(*a, big, 1, 8, 2, 400, 256, 16, 96, None) == -2, i
    for out in (7, 8, 9):  # an output equal to an input (the scales among them) or to another output
        for src in range(10):
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
    a[9] = None
    assert f(*a, 0, *split, None) == -1
    assert f(*p, need - 1, *split, None) == -1
    assert f(*p, 0, *split, None) == -1
    assert f(*p, -1, *split, None) == -1


def test_plan_grid_and_describe(built):
    m = built.manifest
    seen, differs = set(), 0
    for (B, Hq, Hkv, mp, page, D) in grid():
        G, Nmax, step = Hq // Hkv, mp * page, f8.key_step(D)
        rc, S, C, need = _plan(B, Hq, Hkv, mp, page, D)
        assert rc == 0, (B, Hq, Hkv, mp, page, D)
        assert (S, C, need) == f8.plan(B, Hq, Hkv, mp, page, D), (B, Hq, Hkv, mp, page, D, S, C, need)
        assert built.fa2_decode_paged_fp8_plan(B, Hq, Hkv, mp, page, D) == (S, C, need)
        assert S >= 1 and S * C >= Nmax > (S - 1) * C and C % max(page, step) == 0, (B, Hq, Hkv, mp, page, D, S, C)
        assert need == (B * Hq * S * (D + 2) * 4 if S > 1 else 0)
        differs += (S, C) != pr.plan(B, Hq, Hkv, mp, page, D)[:2]
        t = m.describe_decode_paged_fp8(B, Hq, Hkv, mp, page, D)
        assert t.startswith("fa2_decode_paged_fp8<D=%d,G=%d> S=%d C=%d page=%d: 4 waves stream %d-key steps of e4m3" % (D, G, S, C, page, step)), t
        assert ("; then fa2_decode_combine<D=%d>" % D in t) == (S > 1), t
        assert t.endswith("deterministic") and "k_scale" in t and "v_scale" in t, t
        if S > 1:
            assert "workspace %d bytes" % need in t, t
        seen.add((D, 1 if S == 1 else 3 if S >= 3 else 2))
    assert differs > 0  # the key step is twice the fp16 one: this entry needs its own plan
    for D in (64, 128):
        assert f8.key_step(D) == 2 * dr.key_step(D)
        assert (D, 1) in seen and (D, 3) in seen, sorted(seen)
    for dims in ((1, 8, 8, 4, 16, 96), (1, 3, 1, 4, 16, 64), (1, 8, 8, 4, 48, 64), (1, 8, 3, 4, 16, 64), (0, 8, 8, 4, 16, 64)):
        with pytest.raises(ValueError):
            m.describe_decode_paged_fp8(*dims)
    fn = _lib().cln_fa2_decode_paged_fp8_describe
    fn.argtypes, fn.restype = [ctypes.c_int] * 6 + [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    text = m.describe_decode_paged_fp8(1, 8, 2, 256, 16, 128)
    small = ctypes.create_string_buffer(b"\xff" * 24, 24)
    assert fn(1, 8, 2, 256, 16, 128, small, 16) == 15 and small.raw[:16] == text[:15].encode() + b"\0" and small.raw[16:] == b"\xff" * 8
    assert fn(1, 8, 2, 256, 16, 128, None, 16) == -1 and fn(1, 8, 2, 256, 16, 128, small, 0) == -1
    assert fn(1, 8, 2, 256, 16, 128, ctypes.create_string_buffer(1024), 1024) == len(text)


def test_plan_keeps_the_three_constants_and_never_reads_the_lengths(built):
    for D in (64, 128):
        assert len({_plan(2, 4 * G, 4, 256, 16, D)[1:3] for G in pr.GROUPS}) == 1
        assert _plan(64, 32, 32, 4096, 16, D)[1] == 1 and _plan(64, 256, 32, 4096, 16, D)[1] == 1
        assert _plan(1, 8, 1, 16, 16, D)[1] == 1
        assert _plan(1, 8, 1, 4096, 16, D)[1] == dr.MAX_SPLITS
        assert _plan(1, 8, 1, 4096, 16, D)[2] == 65536 // dr.MAX_SPLITS  # chunk 1024 >= MIN_CHUNK, a multiple of the step
    with pytest.raises(RuntimeError, match="fa2_decode_paged_fp8: headdim 96"):
        built.fa2_decode_paged_fp8_plan(1, 8, 8, 4, 16, 96)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_fp8: group size 3"):
        built.fa2_decode_paged_fp8_plan(1, 3, 1, 4, 16, 64)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_fp8: page size 48"):
        built.fa2_decode_paged_fp8_plan(1, 8, 8, 4, 48, 64)
    with pytest.raises(RuntimeError, match="no multiple"):
        built.fa2_decode_paged_fp8_plan(1, 8, 3, 4, 16, 64)


class _Fake:
    """What the Python entry looks at before it asks for a pointer: enough of a tensor to reach the checks under test without a GPU."""
    is_cuda = True

    def __init__(self, dtype, *shape):
        self.dtype, self.shape, self.device = dtype, torch.Size(shape), "cuda:0"

    def dim(self):
        return len(self.shape)


def test_error_messages_of_the_python_entry(built, monkeypatch):
    f = built.fa2_decode_paged_fp8
    h, i32, f32 = torch.float16, torch.int32, torch.float32
    p8 = lambda *s: torch.zeros(*s, dtype=torch.uint8).view(f8.F8)  # noqa: E731
    q = torch.zeros(2, 8, 64, dtype=h)
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(q, p8(9, 2, 16, 64), p8(9, 2, 16, 64), torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), torch.ones(2), torch.ones(2), q.clone())
    with pytest.raises(RuntimeError, match="values must be"):
        f(q.float(), p8(9, 2, 16, 64), p8(9, 2, 16, 64), torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), torch.ones(2), torch.ones(2), q)
    from cuda_learn_notes_amd import host
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)

    def call(D=64, page=16, Hq=8, Hkv=2, pool=f8.F8, sdt=f32, ns=None):
        ns = Hkv if ns is None else ns
        f(_Fake(h, 2, Hq, D), _Fake(pool, 9, Hkv, page, D), _Fake(pool, 9, Hkv, page, D), _Fake(i32, 2, 4), _Fake(i32, 2), _Fake(sdt, ns),
          _Fake(sdt, ns), _Fake(h, 2, Hq, D))
    with pytest.raises(RuntimeError, match="values must be"):  # fp16 pools are the other entry's
        call(pool=h)
    with pytest.raises(RuntimeError, match="values must be"):
        call(pool=torch.float8_e4m3fnuz)
    with pytest.raises(RuntimeError, match="values must be"):
        call(sdt=torch.float64)
    with pytest.raises(RuntimeError, match="Tensor size mismatch"):  # a per-tensor scale is given as the same value Hkv times
        call(ns=1)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_fp8: headdim 96"):
        call(D=96)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_fp8: page size 48"):
        call(page=48)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_fp8: group size 3"):
        call(Hq=6)
    with pytest.raises(RuntimeError, match="no multiple"):
        call(Hkv=3)
    with pytest.raises(AttributeError, match="data_ptr"):  # a supported shape gets as far as the pointers
        call()


def _fp8_stream_symbols(so):
    nm, filt = shutil.which("nm"), shutil.which("c++filt")
    if not nm or not filt:
        pytest.skip("binutils nm / c++filt not available")
    out = subprocess.run([nm, so], capture_output=True, text=True, check=True).stdout
    names = [ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and "fa2_decode_fp8_stream" in ln and "__device_stub__" not in ln]
    dem = subprocess.run([filt], input="\n".join(n.replace("DF16_", "Dh") for n in names), capture_output=True, text=True, check=True).stdout
    return {(int(a), int(b)) for a, b in re.findall(r"fa2d::fa2_decode_fp8_stream<(\d+), (\d+)>", dem)}


def test_fp8_kernels_in_the_product_library_are_exactly_the_plannable_ones(built):
    from cuda_learn_notes_amd import _loader
    linked = _fp8_stream_symbols(_loader.so_path("libcln_amd.so"))
    plannable = set()
    for (B, Hq, Hkv, mp, page, D) in grid():
        mm = re.match(r"fa2_decode_paged_fp8<D=(\d+),G=(\d+)>", built.manifest.describe_decode_paged_fp8(B, Hq, Hkv, mp, page, D))
        plannable.add((int(mm.group(1)), int(mm.group(2))))
    assert len(plannable) == 2 * len(pr.GROUPS), sorted(plannable)
    assert linked == plannable, sorted(linked ^ plannable)


def test_fp8_kernels_keep_registers_and_load_8_bytes(tmp_path):
    import kernel_resources as kr
    kernels, s = kr.report(os.path.join(CSRC, "flash_attn_decode_paged_fp8.hip"), keep=str(tmp_path))
    ks = [k for k in kernels if "fa2d::" in k["demangled"]]
    assert len(ks) == 2 * len(pr.GROUPS) + 2 and len(kernels) == len(ks), [k["demangled"] for k in kernels]
    text = open(s).read()
    streams = 0
    for k in ks:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "v_mfma" not in body and "atomic" not in body, k["demangled"]
        if "fa2_decode_fp8_stream" in k["demangled"]:
            streams += 1
            assert "global_load_dwordx2" in body and "v_cvt_pk_f32_fp8" in body, k
            assert "global_load_ubyte" not in body and "global_load_ushort" not in body, k  # no pool byte is loaded on its own
            assert k["vgpr"] + k["agpr"] <= 512, k
            if re.search(r"<\d+, [12]>", k["demangled"]):
                assert k["vgpr"] <= 256 and k["agpr"] == 0, k  # G <= 2: at least two waves per SIMD
    assert streams == 2 * len(pr.GROUPS)
