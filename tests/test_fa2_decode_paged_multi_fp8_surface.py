"""CPU: the FP8 multi-token paged decode attention entries (include/cln_amd_ext.h: cln_fa2_decode_paged_multi_fp8_plan,
cln_fa2_decode_paged_multi_fp8, cln_fa2_decode_paged_multi_fp8_describe; csrc/flash_attn_decode_paged_multi_fp8.hip) -- header, exports, every
status code before any device access (the scale pointers among them), the plan and the describe text against their Python mirrors
(tests/fp8_paged_attn_reference.py), the Python entry's messages, the reference against brute force on pools with a NaN-byte page, the kernels
linked into the library, and their code (MFMA on both products, the transposing LDS read, 16-byte loads, no spill, no scratch). No GPU needed:
hipcc cross-compiles."""
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
import fp8_paged_attn_reference as fr  # noqa: E402
import multi_decode_reference as mr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402

NAMES = ("cln_fa2_decode_paged_multi_fp8_plan", "cln_fa2_decode_paged_multi_fp8", "cln_fa2_decode_paged_multi_fp8_describe")
BHKV = ((1, 1), (1, 8), (3, 5), (8, 32), (64, 32))  # B Hkv = 1, 8, 15, 256, 2048
MAXPAGES = (1, 3, 63, 256)


def grid():
    for D in (64, 128):
        for (B, Hkv) in BHKV:
            for G in pr.GROUPS:
                for page in pr.PAGES:
                    for mp in MAXPAGES:
                        yield B, 1 + (B + Hkv + G + mp) % mr.MAX_T, Hkv * G, Hkv, mp, page, D


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_three_prototypes(tmp_path, lang, cc):
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*p1)(int, int, int, int, int, int, int, int*, int*, long long*) = cln_fa2_decode_paged_multi_fp8_plan;\n"
                   "int (*d1)(const void*, const void*, const void*, const int*, const int*, const float*, const float*, void*, float*, void*,"
                   " long long, int, int, int, int, int, int, int, int, void*) = cln_fa2_decode_paged_multi_fp8;\n"
                   "int (*t1)(int, int, int, int, int, int, int, char*, int) = cln_fa2_decode_paged_multi_fp8_describe;\n"
                   "int main(void) { return p1 && d1 && t1 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _decode():
    fn = _lib().cln_fa2_decode_paged_multi_fp8
    fn.argtypes = [ctypes.c_void_p] * 10 + [ctypes.c_longlong] + [ctypes.c_int] * 8 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def _plan(B, T, Hq, Hkv, max_pages, page, D):
    fn = _lib().cln_fa2_decode_paged_multi_fp8_plan
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
    for n in ("fa2_decode_paged_multi_fp8", "fa2_decode_paged_multi_fp8_plan"):
        assert hasattr(built, n) and hasattr(host, n), n
    assert hasattr(built.manifest, "describe_decode_paged_multi_fp8")
    names = {e.name for e in built.manifest.ENTRIES}
    for n in NAMES:
        assert n not in names and n.replace("cln_", "") not in names


def test_decode_checks_arguments_before_any_device_access(built):
    f = _decode()
    # q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, o, lse, workspace: never dereferenced, every call below fails its checks first
    p = [0x10000 * (i + 1) for i in range(10)]
    big = 1 << 40
    split = (1, 3, 8, 2, 400, 256, 16, 128)  # B, T, Hq, Hkv, P, max_pages, page, D: a shape whose plan splits the keys
    bad_d = split[:7] + (96,)
    rc, S, C, need = _plan(1, 3, 8, 2, 256, 16, 128)
    assert rc == 0 and S > 1 and need > 0
    assert f(*p, big, *bad_d, None) == -2  # complete but for D: the -1 checks below are what fails, not something else
    for i in range(8):  # a null required pointer, the scales among them
        a = list(p)
        a[i] = None
        assert f(*a, big, *split, None) == -1, i
    a = list(p)
    a[8] = None  # lse may be null
    assert f(*a, big, *bad_d, None) == -2
    for i in (0, 1, 2, 7, 8, 9):  # 16-byte alignment
        a = list(p)
        a[i] = p[i] + 8
        assert f(*a, big, *split, None) == -1, i
    for i in (3, 4, 5, 6):  # block_table, seqlens, k_scale, v_scale: 4-byte alignment, and no more than that
        a = list(p)
        a[i] = p[i] + 2
        assert f(*a, big, *split, None) == -1, i
        a[i] = p[i] + 4
        assert f(*a, big, *bad_d, None) == -2, i
    for out in (7, 8, 9):  # an output equal to an input (the scales among them) or to another output
        for src in range(10):
            if src != out:
                a = list(p)
                a[out] = p[src]
                assert f(*a, big, *split, None) == -1, (out, src)
    for i in range(8):  # each dim non-positive
        for bad in (0, -2):
            d = list(split)
            d[i] = bad
            assert f(*p, big, *d, None) == -1, d
    assert f(*p, big, 1, 3, 8, 3, 400, 256, 16, 128, None) == -1  # Hq % Hkv
    for D in (32, 96, 256, 512):
        assert f(*p, big, 1, 3, 8, 2, 400, 256, 16, D, None) == -2, D
    for T in (9, 16, 1 << 20):
        assert f(*p, big, 1, T, 8, 2, 400, 256, 16, 128, None) == -2, T
    for (Hq, Hkv) in ((3, 1), (6, 2), (16, 1), (5, 1)):  # G = 3, 3, 16, 5
        assert f(*p, big, 1, 3, Hq, Hkv, 400, 256, 16, 128, None) == -2, (Hq, Hkv)
    for page in (1, 8, 48, 100, 512):
        assert f(*p, big, 1, 3, 8, 2, 400, 256, page, 128, None) == -2, page
    assert f(*p, big, 65536, 1, 256, 256, 4, 1, 16, 64, None) == -2  # 2^24 workgroups of 256 threads: one past what a grid dimension takes
    assert f(*p, big, 1, 3, 8, 2, 400, 1 << 24, 256, 64, None) == -2  # max_pages page = 2^32
    # S > 1: a null workspace, and one too small by a single byte
    a = list(p)
    a[9] = None
    assert f(*a, 0, *split, None) == -1
    assert f(*p, need - 1, *split, None) == -1
    assert f(*p, 0, *split, None) == -1
    assert f(*p, -1, *split, None) == -1


def test_plan_grid_and_describe(built):
    m = built.manifest
    seen = set()
    for (B, T, Hq, Hkv, mp, page, D) in grid():
        G, Nmax = Hq // Hkv, mp * page
        rc, S, C, need = _plan(B, T, Hq, Hkv, mp, page, D)
        assert rc == 0, (B, T, Hq, Hkv, mp, page, D)
        assert (S, C, need) == fr.plan(B, T, Hq, Hkv, mp, page, D), (B, T, Hq, Hkv, mp, page, D, S, C, need)
        assert (S, C, need) == mr.plan(B, T, Hq, Hkv, mp, page, D)  # the key step is the fp16 kernel's: the two entries plan alike
        assert built.fa2_decode_paged_multi_fp8_plan(B, T, Hq, Hkv, mp, page, D) == (S, C, need)
        assert S >= 1 and S * C >= Nmax > (S - 1) * C and C % max(page, fr.KEY_STEP) == 0, (B, T, Hq, Hkv, mp, page, D, S, C)
        assert need == (B * T * Hq * S * (D + 2) * 4 if S > 1 else 0)
        t = m.describe_decode_paged_multi_fp8(B, T, Hq, Hkv, mp, page, D)
        assert t == fr.describe_multi_text(B, T, Hq, Hkv, mp, page, D), t
        assert t.startswith("fa2_decode_paged_multi_fp8<D=%d,MT=%d> T=%d G=%d S=%d C=%d page=%d: 4 waves split the %d-key steps, e4m3"
                            % (D, -(-T * G // 16), T, G, S, C, page, fr.KEY_STEP)), t
        assert ("; then fa2_decode_combine<D=%d>" % D in t) == (S > 1), t
        assert t.endswith("deterministic") and "k_scale" in t and "v_scale" in t, t
        assert "v_mfma_f32_16x16x32_f16" in t
        seen.add((D, 1 if S == 1 else 3 if S >= 3 else 2))
    for D in (64, 128):
        assert (D, 1) in seen and (D, 3) in seen, sorted(seen)
        # the plan never reads T, the lengths or the group size: the three constants of the decode plans
        assert len({_plan(2, T, 4 * G, 4, 256, 16, D)[1:3] for G in pr.GROUPS for T in (1, 3, 8)}) == 1
        assert _plan(64, 2, 32, 32, 4096, 16, D)[1] == 1 and _plan(1, 2, 8, 1, 16, 16, D)[1] == 1
        assert _plan(1, 2, 8, 1, 4096, 16, D)[1:3] == (dr.MAX_SPLITS, 65536 // dr.MAX_SPLITS)
    for dims in ((1, 2, 8, 8, 4, 16, 96), (1, 2, 3, 1, 4, 16, 64), (1, 2, 8, 8, 4, 48, 64), (1, 2, 8, 3, 4, 16, 64), (0, 2, 8, 8, 4, 16, 64),
                 (1, 9, 8, 8, 4, 16, 64), (1, 0, 8, 8, 4, 16, 64)):
        with pytest.raises(ValueError):
            m.describe_decode_paged_multi_fp8(*dims)
    fn = _lib().cln_fa2_decode_paged_multi_fp8_describe
    fn.argtypes, fn.restype = [ctypes.c_int] * 7 + [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    text = m.describe_decode_paged_multi_fp8(1, 3, 8, 2, 256, 16, 128)
    small = ctypes.create_string_buffer(b"\xff" * 24, 24)
    assert fn(1, 3, 8, 2, 256, 16, 128, small, 16) == 15 and small.raw[:16] == text[:15].encode() + b"\0" and small.raw[16:] == b"\xff" * 8
    assert fn(1, 3, 8, 2, 256, 16, 128, None, 16) == -1 and fn(1, 3, 8, 2, 256, 16, 128, small, 0) == -1
    assert fn(1, 3, 8, 2, 256, 16, 128, ctypes.create_string_buffer(1280), 1280) == len(text)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi_fp8: headdim 96"):
        built.fa2_decode_paged_multi_fp8_plan(1, 2, 8, 8, 4, 16, 96)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi_fp8: group size 3"):
        built.fa2_decode_paged_multi_fp8_plan(1, 2, 3, 1, 4, 16, 64)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi_fp8: page size 48"):
        built.fa2_decode_paged_multi_fp8_plan(1, 2, 8, 8, 4, 48, 64)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi_fp8: T 9 not supported"):
        built.fa2_decode_paged_multi_fp8_plan(1, 9, 8, 8, 4, 16, 64)
    with pytest.raises(RuntimeError, match="no multiple"):
        built.fa2_decode_paged_multi_fp8_plan(1, 2, 8, 3, 4, 16, 64)


class _Fake:
    """What the Python entry looks at before it asks for a pointer: enough of a tensor to reach the checks under test without a GPU."""
    is_cuda = True

    def __init__(self, dtype, *shape):
        self.dtype, self.shape, self.device = dtype, torch.Size(shape), "cuda:0"

    def dim(self):
        return len(self.shape)


def test_error_messages_of_the_python_entry(built, monkeypatch):
    f = built.fa2_decode_paged_multi_fp8
    h, i32, f32 = torch.float16, torch.int32, torch.float32
    p8 = lambda *s: torch.zeros(*s, dtype=torch.uint8).view(f8.F8)  # noqa: E731
    q = torch.zeros(2, 3, 8, 64, dtype=h)
    rest = (torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), torch.ones(2), torch.ones(2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(q, p8(9, 2, 16, 64), p8(9, 2, 16, 64), *rest, q.clone())
    with pytest.raises(RuntimeError, match="values must be"):
        f(q.float(), p8(9, 2, 16, 64), p8(9, 2, 16, 64), *rest, q)
    from cuda_learn_notes_amd import host
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)

    def call(D=64, page=16, Hq=8, Hkv=2, T=3, pool=f8.F8, sdt=f32, ns=None, **bad):
        ns = Hkv if ns is None else ns
        a = dict(q=_Fake(h, 2, T, Hq, D), k=_Fake(pool, 9, Hkv, page, D), v=_Fake(pool, 9, Hkv, page, D), bt=_Fake(i32, 2, 4), sl=_Fake(i32, 2),
                 ks=_Fake(sdt, ns), vs=_Fake(sdt, ns), o=_Fake(h, 2, T, Hq, D))
        a.update(bad)
        f(a["q"], a["k"], a["v"], a["bt"], a["sl"], a["ks"], a["vs"], a["o"], a.get("lse"))
    for kw in (dict(pool=h), dict(pool=torch.float8_e4m3fnuz), dict(pool=torch.uint8), dict(sdt=torch.float64),
               dict(lse=_Fake(h, 2, 3, 8))):  # fp16 pools are the other entry's
        with pytest.raises(RuntimeError, match="values must be"):
            call(**kw)
    for kw in (dict(ns=1), dict(v=_Fake(f8.F8, 8, 2, 16, 64)), dict(o=_Fake(h, 2, 2, 8, 64)), dict(sl=_Fake(i32, 3)), dict(bt=_Fake(i32, 3, 4)),
               dict(lse=_Fake(f32, 2, 8)), dict(q=_Fake(h, 2, 8, 64)), dict(vs=_Fake(f32, 2, 1))):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            call(**kw)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi_fp8: headdim 96"):
        call(D=96)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi_fp8: page size 48"):
        call(page=48)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi_fp8: group size 3"):
        call(Hq=6)
    with pytest.raises(RuntimeError, match="fa2_decode_paged_multi_fp8: T 9 not supported"):
        call(T=9)
    with pytest.raises(RuntimeError, match="no multiple"):
        call(Hkv=3)
    with pytest.raises(RuntimeError, match="values must be"):  # FP8 pools to the fp16 entry
        built.fa2_decode_paged_multi(_Fake(h, 2, 3, 8, 64), _Fake(f8.F8, 9, 2, 16, 64), _Fake(f8.F8, 9, 2, 16, 64), _Fake(i32, 2, 4),
                                     _Fake(i32, 2), _Fake(h, 2, 3, 8, 64))
    with pytest.raises(AttributeError, match="data_ptr"):  # a supported shape gets as far as the pointers
        call()


def test_reference_is_the_brute_force_masked_softmax_on_a_tiny_case_with_a_nan_page():
    g = torch.Generator().manual_seed(12)
    B, T, Hkv, G, page, mp, D = 3, 5, 2, 2, 16, 2, 64
    P = 7
    q = torch.randn(B, T, Hkv * G, D, generator=g).half()
    ks, vs = torch.tensor([0.011, 0.023]), torch.tensor([0.5, 0.017])
    kp, vp = (f8.quantize(torch.randn(P, Hkv, page, D, generator=g), f8.per_head(torch.full((Hkv,), 0.01))) for _ in range(2))
    kp, vp = f8.bits(kp).clone(), f8.bits(vp).clone()
    kp[0], vp[0] = f8.NAN_BYTE, f8.NAN_BYTE  # a page no entry names
    kp, vp = kp.view(f8.F8), vp.view(f8.F8)
    bt = torch.tensor([[5, 1], [3, 6], [2, 4]], dtype=torch.int32)
    lens = [2, 21, 99]  # fewer than T (right-aligned), a page and a bit, past the capacity (clamped to 32)
    O, L = fr.ref_decode_paged_multi_fp8(q, kp, vp, ks, vs, bt, lens)
    assert bool(torch.isfinite(O).all())
    for b in range(B):
        n_b = min(lens[b], mp * page)
        for t in range(T):
            n = n_b - (T - 1 - t)
            for h in range(Hkv * G):
                if n <= 0:
                    assert bool((O[b, t, h] == 0).all()) and L[b, t, h].item() == float("-inf")
                    continue
                kv = h // G
                rows_k = torch.stack([kp[int(bt[b, j // page]), kv, j % page].float() for j in range(n)]).mul(ks[kv]).double()
                rows_v = torch.stack([vp[int(bt[b, j // page]), kv, j % page].float() for j in range(n)]).mul(vs[kv]).double()
                s = (rows_k @ q[b, t, h].double()) / D ** 0.5
                o1 = torch.softmax(s, dim=0) @ rows_v
                # the rows dequantised in fp32 as fp8_kv_reference.dequantize does; |O| reaches 0.5 x 448
                assert (O[b, t, h] - o1).abs().max().item() <= 1e-10 and abs(L[b, t, h].item() - torch.logsumexp(s, dim=0).item()) <= 1e-10


def _fp8_multi_symbols(so):
    nm, filt = shutil.which("nm"), shutil.which("c++filt")
    if not nm or not filt:
        pytest.skip("binutils nm / c++filt not available")
    out = subprocess.run([nm, so], capture_output=True, text=True, check=True).stdout
    names = [ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and "fa2_decode_paged_multi_fp8_mfma" in ln and "__device_stub__" not in ln]
    dem = subprocess.run([filt], input="\n".join(n.replace("DF16_", "Dh") for n in names), capture_output=True, text=True, check=True).stdout
    return {(int(a), int(b)) for a, b in re.findall(r"fa2pm::fa2_decode_paged_multi_fp8_mfma<(\d+), (\d+)>", dem)}


def test_fp8_kernels_in_the_product_library_are_exactly_the_plannable_ones(built):
    from cuda_learn_notes_amd import _loader
    linked = _fp8_multi_symbols(_loader.so_path("libcln_amd.so"))
    plannable = set()
    for D in (64, 128):
        for G in pr.GROUPS:
            for T in range(1, mr.MAX_T + 1):
                mm = re.match(r"fa2_decode_paged_multi_fp8<D=(\d+),MT=(\d+)>", built.manifest.describe_decode_paged_multi_fp8(1, T, G, 1, 4, 16, D))
                plannable.add((int(mm.group(1)), int(mm.group(2))))
    assert len(plannable) == 8, sorted(plannable)
    assert linked == plannable, sorted(linked ^ plannable)


def test_kernels_run_both_products_on_the_matrix_pipe_and_load_16_bytes(tmp_path):
    import kernel_resources as kr
    kernels, s = kr.report(os.path.join(CSRC, "flash_attn_decode_paged_multi_fp8.hip"), keep=str(tmp_path))
    assert len(kernels) == 10, [k["demangled"] for k in kernels]  # 2 head dims x 4 row-tile counts, and the combine kernel of each head dim
    text = open(s).read()
    multis = 0
    for k in kernels:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "atomic" not in body, k["demangled"]
        if "fa2_decode_paged_multi_fp8_mfma" in k["demangled"]:
            multis += 1
            assert "v_mfma_f32_16x16x32_f16" in body and "ds_read_b64_tr_b16" in body and "global_load_dwordx4" in body, k["demangled"]
            assert "global_load_ubyte" not in body and "global_load_ushort" not in body, k  # no pool byte is loaded on its own
            assert k["vgpr"] <= 512 and k["lds"] <= 64 * 1024, k  # vgpr counts the accumulation registers too
        else:
            assert "fa2d::fa2_decode_combine_kernel<" in k["demangled"], k["demangled"]
    assert multis == 8
