"""CPU: the paged prefill attention entries (include/cln_amd_ext.h: cln_fa2_prefill_paged, cln_fa2_prefill_paged_describe;
csrc/flash_attn_prefill_paged.hip) -- header, exports, every status code before any device access, the describe text against its Python mirror,
the Python entry's messages, the reference of tests/prefill_reference.py against the multi-token reference and against brute force, and the
kernels' code (MFMA on both products, the transposing LDS read, no spill, no scratch, LDS for two workgroups per CU). No GPU needed: hipcc
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
import multi_decode_reference as mr  # noqa: E402
import paged_decode_reference as pr  # noqa: E402
import prefill_reference as pf  # noqa: E402

NAMES = ("cln_fa2_prefill_paged", "cln_fa2_prefill_paged_describe")
LDS_PER_CU = 160 * 1024


@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_both_prototypes(tmp_path, lang, cc):
    if not shutil.which(cc):
        pytest.skip(cc + " not available")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n'
                   "int (*a1)(const void*, const void*, const void*, const int*, const int*, void*, float*, int, int, int, int, int, int, int, int,"
                   " void*) = cln_fa2_prefill_paged;\n"
                   "int (*t1)(int, int, int, int, int, int, int, char*, int) = cln_fa2_prefill_paged_describe;\n"
                   "int main(void) { return a1 && t1 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _lib():
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


def _prefill():
    fn = _lib().cln_fa2_prefill_paged
    fn.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_int] * 8 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def _describe_fn():
    fn = _lib().cln_fa2_prefill_paged_describe
    fn.argtypes, fn.restype = [ctypes.c_int] * 7 + [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
    return fn


def _describe(*dims):
    buf = ctypes.create_string_buffer(1024)
    rc = _describe_fn()(*dims, buf, 1024)
    return rc, buf.value.decode()


def test_product_library_and_package_export_the_entries(built):
    lib = _lib()
    for n in NAMES:
        assert hasattr(lib, n), n
    from cuda_learn_notes_amd import host
    assert hasattr(built, "fa2_prefill_paged") and hasattr(host, "fa2_prefill_paged")
    assert hasattr(built.manifest, "describe_prefill_paged")


def test_names_stay_off_the_manifest_surface(built):
    names = {e.name for e in built.manifest.ENTRIES}
    for n in NAMES:
        assert n not in names and n.replace("cln_", "") not in names
    gen = open(os.path.join(ROOT, "include", "cln_amd.h")).read()
    assert not any(n + "(" in gen for n in NAMES)
    fast = open(os.path.join(CSRC, "pyext", "cln_fastcall.c")).read()
    assert "prefill" not in fast


# q, k_pages, v_pages, block_table, seqlens, o, lse: never dereferenced, every call below fails its checks first
PTR = [0x10000 * (i + 1) for i in range(7)]
DIMS = (2, 40, 8, 2, 40, 6, 16, 128)  # B, T, Hq, Hkv, P, max_pages, page, D
BAD_D = DIMS[:7] + (96,)              # the same with an unsupported D: what a call that passed every -1 check ends on


def test_prefill_checks_arguments_before_any_device_access(built):
    f = _prefill()
    p = list(PTR)
    # a call that is complete but for an unsupported D ends on -2, with and without lse: the -1 checks below are what fails, not something else
    assert f(*p, *BAD_D, None) == -2 and f(*p[:6], None, *BAD_D, None) == -2
    for i in range(6):  # a null required pointer
        a = list(p)
        a[i] = None
        assert f(*a, *DIMS, None) == -1, i
    for i in (0, 1, 2, 5):  # 16-byte alignment
        a = list(p)
        a[i] = p[i] + 8
        assert f(*a, *DIMS, None) == -1, i
    for i in (3, 4, 6):  # block_table, seqlens, lse: 4-byte alignment, and no more than that
        a = list(p)
        a[i] = p[i] + 2
        assert f(*a, *DIMS, None) == -1, i
        a[i] = p[i] + 4
        assert f(*a, *BAD_D, None) == -2, i
    for out in (5, 6):  # an output equal to an input or to the other output
        for src in range(7):
            if src != out:
                a = list(p)
                a[out] = p[src]
                assert f(*a, *DIMS, None) == -1, (out, src)
    for i in range(8):  # each dimension non-positive
        for bad in (0, -2):
            d = list(DIMS)
            d[i] = bad
            assert f(*p, *d, None) == -1, d
    assert f(*p, 2, 40, 8, 3, 40, 6, 16, 128, None) == -1  # Hq % Hkv
    # -2: the unsupported shapes
    for D in (32, 96, 256, 512):
        assert f(*p, *DIMS[:7], D, None) == -2, D
    for (Hq, Hkv) in ((3, 1), (6, 2), (16, 1), (5, 1)):  # G = 3, 3, 16, 5
        assert f(*p, 2, 40, Hq, Hkv, 40, 6, 16, 128, None) == -2, (Hq, Hkv)
    for page in (1, 8, 48, 100, 512):
        assert f(*p, 2, 40, 8, 2, 40, 6, page, 128, None) == -2, page
    assert f(*p, 2, 40, 8, 2, 40, 1 << 23, 256, 128, None) == -2  # max_pages page = 2^31
    assert f(*p, 1, 1 << 28, 8, 1, 40, 6, 16, 128, None) == -2  # T G = 2^31 rows of a KV head
    assert f(*p, 1 << 12, 1 << 19, 8, 8, 40, 6, 16, 64, None) == -2  # 2^15 pairs x 2^12 tiles: 2^27 workgroups of 256 threads
    # T far past what cln_fa2_decode_paged_multi takes is no error here: the call gets as far as the unsupported D
    assert f(*p, 2, 1 << 20, 8, 2, 40, 6, 16, 96, None) == -2 and _describe(2, 1 << 20, 8, 2, 6, 16, 128)[0] > 0


def test_describe_names_the_instantiation_and_matches_the_python_mirror(built):
    m = built.manifest
    for D in (64, 128):
        for G in pr.GROUPS:
            for page in pr.PAGES:
                for (B, T, Hkv, mp) in ((1, 1, 1, 1), (3, 19, 3, 3), (4, 512, 8, 64), (2, 4096, 2, 300), (256, 129, 2, 7)):
                    Hq = Hkv * G
                    rc, text = _describe(B, T, Hq, Hkv, mp, page, D)
                    assert rc == len(text) > 0, (rc, text)
                    assert text == m.describe_prefill_paged(B, T, Hq, Hkv, mp, page, D)
                    assert text == pf.describe_text(B, T, Hq, Hkv, mp, page, D)
                    assert text.startswith("fa2_prefill_paged<D=%d,G=%d> T=%d page=%d rows=%d keys=%d: one launch, no workspace"
                                           % (D, G, T, page, pf.ROW_TILE, pf.KEY_STEP)), text
                    assert text.endswith("deterministic"), text
                    assert "%d workgroups of 256 threads" % (B * Hkv * -(-T * G // pf.ROW_TILE)) in text, text
                    assert "v_mfma_f32_16x16x32_f16" in text and "ds_read_b64_tr_b16" in text
    rc, text = _describe(1, 1, 8, 2, 4, 16, 64)
    fn = _describe_fn()
    small = ctypes.create_string_buffer(b"\xff" * 24, 24)
    assert fn(1, 1, 8, 2, 4, 16, 64, small, 16) == 15 and small.raw[:16] == text[:15].encode() + b"\0" and small.raw[16:] == b"\xff" * 8
    assert fn(1, 1, 8, 2, 4, 16, 64, None, 16) == -1 and fn(1, 1, 8, 2, 4, 16, 64, small, 0) == -1
    for dims in ((1, 2, 8, 8, 4, 16, 96), (1, 2, 3, 1, 4, 16, 64), (1, 2, 8, 8, 4, 48, 64), (1, 2, 8, 3, 4, 16, 64), (0, 2, 8, 8, 4, 16, 64),
                 (1, 0, 8, 8, 4, 16, 64), (1, 2, 8, 8, 1 << 23, 256, 64), (1, 1 << 28, 8, 1, 4, 16, 64)):
        with pytest.raises(ValueError):
            m.describe_prefill_paged(*dims)


class _Fake:
    """What the Python entry looks at before it asks for a pointer: enough of a tensor to reach the checks under test without a GPU."""
    is_cuda = True

    def __init__(self, dtype, *shape):
        self.dtype, self.shape, self.device = dtype, torch.Size(shape), "cuda:0"

    def dim(self):
        return len(self.shape)


def test_error_messages_of_the_python_entry(built, monkeypatch):
    f = built.fa2_prefill_paged
    h, i32 = torch.float16, torch.int32
    t = lambda *s: torch.zeros(*s, dtype=h)  # noqa: E731
    args = (t(2, 40, 4, 64), t(9, 2, 16, 64), t(9, 2, 16, 64), torch.zeros(2, 4, dtype=i32), torch.zeros(2, dtype=i32), t(2, 40, 4, 64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        f(*args)
    with pytest.raises(RuntimeError, match="values must be"):
        f(args[0].float(), *args[1:])
    with pytest.raises(RuntimeError, match="values must be"):
        f(*args[:3], args[3].long(), *args[4:])
    # the shape messages come behind the device check: tensors that only claim to be on the GPU, and are refused before any pointer is taken
    from cuda_learn_notes_amd import host
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)

    def call(D=64, page=16, Hq=4, Hkv=2, T=40, **bad):
        a = dict(q=_Fake(h, 2, T, Hq, D), k=_Fake(h, 9, Hkv, page, D), v=_Fake(h, 9, Hkv, page, D), bt=_Fake(i32, 2, 4), sl=_Fake(i32, 2),
                 o=_Fake(h, 2, T, Hq, D), lse=_Fake(torch.float32, 2, T, Hq))
        a.update(bad)
        f(a["q"], a["k"], a["v"], a["bt"], a["sl"], a["o"], a["lse"])
    with pytest.raises(RuntimeError, match="fa2_prefill_paged: headdim 96 not supported"):
        call(D=96)
    with pytest.raises(RuntimeError, match=r"fa2_prefill_paged: group size 3 \(= Hq 6 / Hkv 2\) not supported"):
        call(Hq=6)
    with pytest.raises(RuntimeError, match="fa2_prefill_paged: page size 48 not supported"):
        call(page=48)
    with pytest.raises(RuntimeError, match="fa2_prefill_paged: 4 query heads are no multiple of 3 KV heads"):
        call(Hkv=3)
    for bad in (dict(v=_Fake(h, 8, 2, 16, 64)), dict(o=_Fake(h, 2, 39, 4, 64)), dict(sl=_Fake(i32, 3)), dict(bt=_Fake(i32, 3, 4)),
                dict(lse=_Fake(torch.float32, 2, 4)), dict(q=_Fake(h, 2, 4, 64)), dict(bt=_Fake(i32, 8))):
        with pytest.raises(RuntimeError, match="Tensor size mismatch"):
            call(**bad)
    with pytest.raises(RuntimeError, match="values must be"):
        call(lse=_Fake(h, 2, 40, 4))
    for T in (1, 9, 4096):  # a supported shape, whatever T is, gets as far as the pointers
        with pytest.raises(AttributeError, match="data_ptr"):
            call(T=T)


@pytest.mark.parametrize("T", [1, 3, 8])
def test_reference_agrees_with_the_multi_token_reference(T):
    """The two fp64 references form the same sums in different orders (one matrix product per head here, one einsum per query token there):
    equal to 1e-12, and the -inf / zero rows exactly."""
    g = torch.Generator().manual_seed(5 + T)
    B, Hkv, G, page, mp, D = 3, 2, 2, 16, 4, 64
    q = torch.randn(B, T, Hkv * G, D, generator=g).half()
    k, v = torch.randn(B, Hkv, mp * page, D, generator=g).half(), torch.randn(B, Hkv, mp * page, D, generator=g).half()
    lens = [2, 33, 64]
    kp, vp, bt = pr.make_pool(k, v, page, lens, seed=T)
    O, L = pf.ref_prefill_paged(q, kp, vp, bt, lens)
    O1, L1 = mr.ref_decode_paged_multi(q, kp, vp, bt, lens)
    fin = torch.isfinite(L1)
    assert torch.equal(torch.isfinite(L), fin) and bool((L[~fin] == float("-inf")).all()) and bool((O[~fin] == 0).all())
    assert bool(torch.isfinite(O).all())  # the NaN pages of the pool are never touched
    assert (O - O1).abs().max().item() <= 1e-12 and (L[fin] - L1[fin]).abs().max().item() <= 1e-12
    assert pf.visible(lens, T, mp * page).flatten().tolist() == mr.visible(lens, T, mp * page)
    assert (T < 3) == bool(fin.all())  # T >= 3: sequence 0 (length 2) has queries with no key


def test_reference_is_the_brute_force_masked_softmax_on_a_tiny_case():
    g = torch.Generator().manual_seed(11)
    B, T, Hkv, G, page, mp, D = 3, 20, 1, 2, 16, 2, 64
    P = 7
    q = torch.randn(B, T, Hkv * G, D, generator=g).half()
    kp, vp = torch.randn(P, Hkv, page, D, generator=g).half(), torch.randn(P, Hkv, page, D, generator=g).half()
    kp[0], vp[0] = float("nan"), float("nan")  # a page no entry names
    bt = torch.tensor([[5, 1], [3, 6], [2, 4]], dtype=torch.int32)
    lens = [2, 21, 99]  # fewer than T (right-aligned), a page and a bit, past the capacity (clamped to 32)
    O, L = pf.ref_prefill_paged(q, kp, vp, bt, lens)
    for b in range(B):
        n_b = min(lens[b], mp * page)
        for t in range(T):
            n = n_b - (T - 1 - t)
            for h in range(Hkv * G):
                if n <= 0:
                    assert bool((O[b, t, h] == 0).all()) and L[b, t, h].item() == float("-inf")
                    continue
                rows_k = torch.stack([kp[int(bt[b, j // page]), h // G, j % page] for j in range(n)]).double()
                rows_v = torch.stack([vp[int(bt[b, j // page]), h // G, j % page] for j in range(n)]).double()
                s = (rows_k @ q[b, t, h].double()) / D ** 0.5
                o1 = torch.softmax(s, dim=0) @ rows_v
                assert (O[b, t, h] - o1).abs().max().item() <= 1e-12 and abs(L[b, t, h].item() - torch.logsumexp(s, dim=0).item()) <= 1e-12
    assert pf.visible([2, 21, -4, 99], 3, 32).tolist() == [[0, 1, 2], [19, 20, 21], [0, 0, 0], [30, 31, 32]]
    assert (pf.tiles(1, 1), pf.tiles(16, 8), pf.tiles(129, 1), pf.tiles(33, 4)) == (1, 1, 2, 2)


def test_kernels_run_both_products_on_the_matrix_pipe_and_keep_registers(tmp_path):
    import kernel_resources as kr
    kernels, s = kr.report(os.path.join(CSRC, "flash_attn_prefill_paged.hip"), keep=str(tmp_path))
    assert len(kernels) == 2 and all("fa2pp::fa2_prefill_paged_kernel<" in k["demangled"] for k in kernels), [k["demangled"] for k in kernels]
    text = open(s).read()
    for k in kernels:
        assert k["spill"] == 0 and k["sgpr_spill"] == 0 and k["scratch"] == 0, k
        assert 0 < 2 * k["lds"] <= LDS_PER_CU, k  # two workgroups resident per CU ...
        assert k["vgpr"] <= 256, k                # ... whose 8 waves, two per SIMD, share the 512 registers of a lane
        body = text[text.index("\n" + k["name"] + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "v_mfma_f32_16x16x32_f16" in body and "ds_read_b64_tr_b16" in body and "global_load_dwordx4" in body, k["demangled"]
