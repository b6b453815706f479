"""Host-side mirror of the reference's per-kernel PyTorch-extension API.

Every reference `lib.<name>(tensors..., knobs...)` exists here with the same name, argument order
and error behaviour, implemented as: dtype/shape checks -> `extern "C" int <name>(ptrs, dims, knobs,
stream)` through ctypes -> status code mapped back to RuntimeError. PyTorch is only plumbing
(device memory + current HIP stream). Tensors must live on the GPU: there is no CPU path.

Reference bindings mirrored (checks and messages):
  CHECK_TORCH_TENSOR_DTYPE -> RuntimeError("values must be torch::kHalf")   kernels/hgemm/naive/hgemm.cu:772-777
  CHECK_TORCH_TENSOR_SHAPE -> RuntimeError("Tensor size mismatch!")          kernels/hgemm/naive/hgemm.cu:778-782
  head-dim switch default  -> RuntimeError("headdim not support!")           flash_attn_mma_share_qkv.cu:860,:882
"""
import ctypes
import math
import os
import threading
import types

import torch

from . import _loader, manifest

_TH_NAME = {
    torch.float16: "torch::kHalf", torch.float32: "torch::kFloat32", torch.bfloat16: "torch::kBFloat16",
    torch.int8: "torch::kInt8", torch.int32: "torch::kInt32",
}
if hasattr(torch, "float8_e4m3fn"):
    _TH_NAME[torch.float8_e4m3fn] = "torch::kFloat8_e4m3fn"
    _TH_NAME[torch.float8_e5m2] = "torch::kFloat8_e5m2"

_STATUS_TEXT = {
    -1: "bad argument (null/misaligned pointer or non-positive size)",
    -2: "unsupported shape",
    -3: "HIP launch failed (hipGetLastError)",
    -4: "rocBLAS row failed (call init_cublas_handle() first?)",
}


def _check_dtype(t, dtype):
    if t.dtype != dtype:
        print("Tensor Info:", t.dtype, t.device, tuple(t.shape))
        raise RuntimeError("values must be %s" % _TH_NAME.get(dtype, str(dtype)))


# The wrappers below run once per launch: for a 4-10 us kernel their cost IS the launch rate (profiles/r04_bw_rows_probe.log: 8.0 us per call
# through torch.cuda.current_stream() and per-tensor device objects, 4 us for torch's own dispatcher). The raw getters of torch._C do the same
# lookups without building Stream / device objects; they exist in every torch 2.x build (Triton's launcher uses them) -- the public API is
# the fallback.
_raw_device = getattr(torch._C, "_cuda_getDevice", None)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _current_device():
    return _raw_device() if _raw_device is not None else torch.cuda.current_device()


def _check_dev(*ts):
    """Every tensor must be a contiguous HIP tensor on the CURRENT device: the launch goes to
    torch.cuda.current_stream() of the current device with raw data_ptr()s, so a tensor living on another GPU
    would be dereferenced from the wrong device (fault or silent peer access)."""
    for t in ts:
        if not t.is_cuda:
            raise RuntimeError("expected a GPU (HIP) tensor, got device=%s: the kernel library has no CPU path"
                               % t.device)
    cur = _current_device() if ts else -1
    for t in ts:
        if t.get_device() != cur:
            raise RuntimeError("tensor on %s but the current device is cuda:%d: wrap the call in "
                               "`with torch.cuda.device(tensor.device):`" % (t.device, cur))
        if not t.is_contiguous():
            raise RuntimeError("tensor must be contiguous (the kernels take raw data_ptr())")


def _check_shape(t, *shape):
    if t.shape != shape:  # torch.Size is a tuple
        raise RuntimeError("Tensor size mismatch!")


def _stream():
    """The raw hipStream_t of torch's current stream on the current device."""
    if _raw_stream is not None:
        return _raw_stream(_current_device())
    return torch.cuda.current_stream().cuda_stream


# ---- the CPython entry in front of the C-ABI (csrc/pyext/cln_fastcall.c, round 5): argument checks, data_ptr()s, the raw stream and the C call
# in one vectorcall, falling back to the pure-Python wrapper below on ANY failed check or non-zero status (so the error texts stay those of
# this file). Absent module, CPU-only torch build or $CLN_AMD_NO_FASTCALL=1: the wrappers call through ctypes as before.
def _load_fastcall():
    if os.environ.get("CLN_AMD_NO_FASTCALL", "0") == "1" or _raw_device is None or _raw_stream is None:
        return None
    import glob
    import importlib.util
    for path in glob.glob(os.path.join(_loader.LIBDIR, "_cln_fastcall*.so")):
        try:
            spec = importlib.util.spec_from_file_location("_cln_fastcall", path)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            mod.setup(_raw_device, _raw_stream)
            return mod
        except Exception:  # noqa: BLE001 -- an optional accelerator: any trouble means ctypes
            continue
    return None


_fastcall = _load_fastcall()


def _fast(kind, name, fn, slow, dtype, vt=False, out_dtype=None):
    """`slow` wrapped by the vectorcall entry of kind `kind` (a key of _cln_fastcall.KINDS) when the extension is there."""
    if _fastcall is None:
        return slow
    import ctypes
    addr = ctypes.cast(fn, ctypes.c_void_p).value
    return _fastcall.bind(addr, _fastcall.KINDS[kind], dtype, slow, name, int(bool(vt)), out_dtype)


def _raise(name, rc, unsupported_msg=None):
    if rc == 0:
        return
    if rc == -2 and unsupported_msg:
        raise RuntimeError(unsupported_msg)
    raise RuntimeError("%s: %s (status %d)" % (name, _STATUS_TEXT.get(rc, "error"), rc))


# ------------------------------------------------------------------------------------------------
def _make_g3(name, dtype=torch.float16):
    fn = _loader.symbol(name)

    def f(a, b, c):
        for t in (a, b, c):
            _check_dtype(t, dtype)
        _check_dev(a, b, c)
        M, K = a.size(0), a.size(1)
        N = b.size(1)  # TN operands keep the [K,N] shape (reference as_col_major)
        _check_shape(a, M, K)
        _check_shape(b, K, N)
        _check_shape(c, M, N)
        _raise(name, fn(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, _stream()),
               "%s: M/N/K must be multiples of the block tile" % name)
    f.__name__ = name
    return _fast("G3", name, fn, f, dtype)


def _make_g6(name, dtype=torch.float16):
    fn = _loader.symbol(name)

    def f(a, b, c, stages, swizzle=False, swizzle_stride=1):
        for t in (a, b, c):
            _check_dtype(t, dtype)
        _check_dev(a, b, c)
        M, K = a.size(0), a.size(1)
        N = b.size(1)
        _check_shape(a, M, K)
        _check_shape(b, K, N)
        _check_shape(c, M, N)
        _raise(name, fn(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, int(stages), int(bool(swizzle)),
                        int(swizzle_stride), _stream()),
               "%s: M/N/K must be multiples of the block tile" % name)
    f.__name__ = name
    call = _fast("G6", name, fn, f, dtype)
    if not manifest.BY_NAME[name].impl.startswith("best<"):
        return call

    # the run-time dispatched names may split K: the stream's workspace is a tensor of torch's caching allocator, handed to the library before
    # the launch (the library itself never allocates: include/cln_amd.h, workspace block)
    def g(a, b, c, stages, swizzle=False, swizzle_stride=1):
        try:
            need = _ws_need[(a.shape[0], b.shape[1], a.shape[1])]
        except KeyError:
            need = _ws_need_of(a.shape[0], b.shape[1], a.shape[1])
        except Exception:  # noqa: BLE001 -- not tensors / wrong rank: the wrapper below raises the reference's error
            need = 0
        if need:
            _ensure_workspace(need)
        return call(a, b, c, stages, swizzle, swizzle_stride)
    g.__name__ = name
    return g


def _make_h0(name):
    fn = _loader.symbol(name)

    def f():
        _raise(name, fn())
    f.__name__ = name
    return f


def _make_fa(name):
    fn = _loader.symbol(name)
    vt = name in manifest.FA_V_TRANSPOSED

    def f(Q, K, V, O, stages):
        for t in (Q, K, V, O):
            _check_dtype(t, torch.float16)
        _check_dev(Q, K, V, O)
        B, H, N, D = Q.shape
        _check_shape(K, B, H, N, D)
        _check_shape(O, B, H, N, D)
        if vt:
            _check_shape(V, B, H, D, N)
        else:
            _check_shape(V, B, H, N, D)
        rc = fn(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), B, H, N, D, int(stages), _stream())
        if rc == -2:
            if N % 64 != 0 or (D == 256 and N % 128 != 0) or (D > 256 and N % 128 != 0):
                raise RuntimeError("%s: seqlen must be a multiple of 64 (128 for headdim >= 256)" % name)
            raise RuntimeError("headdim not support!")
        _raise(name, rc)
    f.__name__ = name
    return _fast("FA", name, fn, f, torch.float16, vt=vt)


def _make_p3(name):
    fn = _loader.symbol(name)
    dtype = torch.float32 if "_f32" in name else torch.float16

    def f(a, b, c):
        for t in (a, b, c):
            _check_dtype(t, dtype)
        _check_dev(a, b, c)
        _check_shape(b, *a.shape)
        _check_shape(c, *a.shape)
        _raise(name, fn(a.data_ptr(), b.data_ptr(), c.data_ptr(), a.numel(), _stream()))
    f.__name__ = name
    return _fast("P3", name, fn, f, dtype)


def _make_r1(name):
    fn = _loader.symbol(name)
    in_dt, out_dt = (getattr(torch, n) for n in manifest.REDUCE_DTYPES[name])

    def f(x):
        _check_dtype(x, in_dt)
        _check_dev(x)
        # the reference binding allocates a ZEROED result (block_all_reduce.cu:737-738) and its blocks add into it: two dispatches per call. Here the
        # launch overwrites y (csrc/stream_scratch.h: the last block moves the total out of a self-resetting per-stream scratch word): no fill kernel
        y = torch.empty(1, dtype=out_dt, device=x.device)
        _raise(name, fn(x.data_ptr(), y.data_ptr(), x.numel(), _stream()))
        return y
    f.__name__ = name
    return _fast("R1", name, fn, f, in_dt, out_dtype=out_dt)


_SOFTMAX_ONE_BLOCK_MAX = 65536  # == SOFTMAX_ONE_BLOCK_MAX in csrc/softmax.hip (tests/test_host_logic.py holds them equal)


def _make_sg(name):
    fn = _loader.symbol(name)

    def f(x, y):
        _check_dtype(x, torch.float32)
        _check_dtype(y, torch.float32)
        _check_dev(x, y)
        _check_shape(y, *x.shape)
        # reference softmax.cu:419 allocates the zeroed accumulator in the binding; up to _SOFTMAX_ONE_BLOCK_MAX elements ONE workgroup
        # does both passes and overwrites it (csrc/softmax.hip SOFTMAX_ONE_BLOCK_MAX), so no fill kernel is launched for it
        n = x.numel()
        total = (torch.empty if n <= _SOFTMAX_ONE_BLOCK_MAX else torch.zeros)(1, dtype=torch.float32, device=x.device)
        _raise(name, fn(x.data_ptr(), y.data_ptr(), total.data_ptr(), x.numel(), _stream()))
    f.__name__ = name
    return f


def _make_xy(name):
    fn = _loader.symbol(name)
    dtype = torch.float16 if "_f16" in name else torch.float32

    def f(x, y):
        _check_dtype(x, dtype)
        _check_dtype(y, dtype)
        _check_dev(x, y)
        _check_shape(y, *x.shape)
        S, H = x.size(0), x.size(1)
        _raise(name, fn(x.data_ptr(), y.data_ptr(), S, H, _stream()),
               "%s: unsupported H=%d (must be a multiple of the pack width and fit 8 packs x 1024 lanes)"
               % (name, H))
    f.__name__ = name
    return _fast("XY", name, fn, f, dtype)


def _make_ln(name):
    fn = _loader.symbol(name)
    dtype = torch.float32 if name.startswith("layer_norm_f32") else torch.float16

    def f(x, y, g, b):
        _check_dtype(x, dtype)
        _check_dtype(y, dtype)
        _check_dev(x, y)
        _check_shape(y, *x.shape)
        N, K = x.size(0), x.size(1)
        _raise(name, fn(x.data_ptr(), y.data_ptr(), float(g), float(b), N, K, _stream()),
               "%s: unsupported K=%d" % (name, K))
    f.__name__ = name
    return _fast("LN", name, fn, f, dtype)


def _make_rn(name):
    fn = _loader.symbol(name)
    dtype = torch.float32 if name.startswith("rms_norm_f32") else torch.float16

    def f(x, y, g):
        _check_dtype(x, dtype)
        _check_dtype(y, dtype)
        _check_dev(x, y)
        _check_shape(y, *x.shape)
        N, K = x.size(0), x.size(1)
        _raise(name, fn(x.data_ptr(), y.data_ptr(), float(g), N, K, _stream()), "%s: unsupported K=%d" % (name, K))
    f.__name__ = name
    return _fast("RN", name, fn, f, dtype)


def _make_rp(name):
    fn = _loader.symbol(name)

    def f(x, out, ref_quirk=None):
        """ref_quirk=False (default): the script's torch semantics, pair i of token t rotated by t * theta^(-2i/hidden)
        (rope.py:68-88). ref_quirk=True: the reference CUDA KERNELS' behaviour -- the exponent is an integer division
        that is always 0, so every pair is rotated by t radians (rope.cu:26,:41,:55). Keyword argument added to the
        reference signature `rope_*(x, out)`; $CLN_AMD_ROPE_REF_QUIRK=1 sets the default for callers that cannot
        pass it (read once at import)."""
        _check_dtype(x, torch.float32)
        _check_dtype(out, torch.float32)
        _check_dev(x, out)
        _check_shape(out, *x.shape)
        quirk = int(_ROPE_QUIRK_DEFAULT if ref_quirk is None else bool(ref_quirk))
        _raise(name, fn(x.data_ptr(), out.data_ptr(), x.size(0), x.size(1), quirk, _stream()),
               "%s: hidden size must be a multiple of the pack width" % name)
    f.__name__ = name
    return f


_ROPE_QUIRK_DEFAULT = os.environ.get("CLN_AMD_ROPE_REF_QUIRK", "0") == "1"


def _make_hi(name):
    fn = _loader.symbol(name)

    def f(a):
        _check_dtype(a, torch.int32)
        _check_dev(a)
        # reference binding: M = max(a) on the host, y = zeros(M + 1) (histogram.cu:60-66)
        nbins = int(a.max().item()) + 1 if a.numel() else 1
        y = torch.zeros(max(nbins, 1), dtype=torch.int32, device=a.device)
        _raise(name, fn(a.data_ptr(), y.data_ptr(), a.numel(), max(nbins, 1), _stream()))
        return y
    f.__name__ = name
    return f


def _make_em(name):
    fn = _loader.symbol(name)
    dtype = torch.float32 if "_f32" in name else torch.float16

    def f(a, weight, o):
        _check_dtype(a, torch.int32)
        _check_dtype(weight, dtype)
        _check_dtype(o, dtype)
        _check_dev(a, weight, o)
        n, emb = a.size(0), weight.size(1)
        _check_shape(o, n, emb)
        _raise(name, fn(a.data_ptr(), weight.data_ptr(), o.data_ptr(), n, emb, weight.size(0), _stream()),
               "%s: embedding size must be a multiple of the pack width" % name)
    f.__name__ = name
    return f


def _make_un(name):
    fn = _loader.symbol(name)
    dtype = torch.float32 if "_f32" in name else torch.float16

    def f(x, y):
        _check_dtype(x, dtype)
        _check_dtype(y, dtype)
        _check_dev(x, y)
        _check_shape(y, *x.shape)
        _raise(name, fn(x.data_ptr(), y.data_ptr(), x.numel(), _stream()))
    f.__name__ = name
    return _fast("UN", name, fn, f, dtype)


def _make_d2(name):
    fn = _loader.symbol(name)
    dtype = torch.float32 if name.startswith("dot_prod_f32") else torch.float16

    def f(a, b):
        _check_dtype(a, dtype)
        _check_dtype(b, dtype)
        _check_dev(a, b)
        _check_shape(b, *a.shape)
        prod = torch.empty(1, dtype=torch.float32, device=a.device)  # reference dot_product.cu:236-238 zeroes it; here the launch overwrites it (stream_scratch.h)
        _raise(name, fn(a.data_ptr(), b.data_ptr(), prod.data_ptr(), a.numel(), _stream()))
        return prod
    f.__name__ = name
    return _fast("D2", name, fn, f, dtype, out_dtype=torch.float32)


def _make_gv(name):
    fn = _loader.symbol(name)
    dtype = torch.float32 if name.startswith("sgemv") else torch.float16
    kmsg = {"k32": "K must be multiple of 32", "k128": "K must be multiple of 128", "k16": "K must be 16"}[name.split("_")[1]]

    def f(a, x, y):
        for t in (a, x, y):
            _check_dtype(t, dtype)
        _check_dev(a, x, y)
        M, K = a.size(0), a.size(1)
        _check_shape(x, K, 1)
        _check_shape(y, M, 1)
        _raise(name, fn(a.data_ptr(), x.data_ptr(), y.data_ptr(), M, K, _stream()), kmsg)  # sgemv.cu:134-137
    f.__name__ = name
    return f


def _make_tr(name):
    fn = _loader.symbol(name)

    def f(x, y):
        _check_dtype(x, torch.float32)
        _check_dtype(y, torch.float32)
        _check_dev(x, y)
        M, N = x.size(0), x.size(1)
        _check_shape(y, N, M)
        _raise(name, fn(x.data_ptr(), y.data_ptr(), M, N, _stream()),
               "%s: rows/cols must be multiples of 4 (x4 rungs) / 64 (shared rungs)" % name)
    f.__name__ = name
    return f


def _make_s3(name):
    return _make_g3(name, torch.float32)


def _make_s6(name):
    return _make_g6(name, torch.float32)


_MAKERS = {"S3": _make_s3, "S6": _make_s6, "D2": _make_d2, "GV": _make_gv, "TR": _make_tr, "UN": _make_un, "HI": _make_hi, "EM": _make_em, "G3": _make_g3, "G6": _make_g6, "H0": _make_h0, "FA": _make_fa, "P3": _make_p3, "R1": _make_r1,
           "SG": _make_sg, "XY": _make_xy, "LN": _make_ln, "RN": _make_rn, "RP": _make_rp}


def load_lib(*groups):
    """Return a module-like object whose attributes are the exported functions of the given lib
    groups ('hgemm' also pulls in the vendor row, as the reference's single hgemm module does)."""
    ns = types.SimpleNamespace()
    for e in manifest.ENTRIES:
        if e.lib in groups:
            if e.lib in manifest.OPTIONAL_LIBS and not _loader.has_symbol(e.name):
                continue  # optional comparison row absent from this build: the attribute is simply not there (callers test with hasattr / try)
            setattr(ns, e.name, _MAKERS[e.sig](e.name))
    return ns


# ---- split-K workspace of the best-dispatch HGEMM names (include/cln_amd.h; not part of the reference surface) -----------------------------
# Round 6 ("no hidden workspace"): the LIBRARY owns nothing. Every (device, stream) that runs a split-K shape through this module gets
# ONE uint8 tensor from torch's caching allocator (allocated on that stream, so its lifetime follows torch's stream semantics), registered with
# cln_hgemm_set_workspace and grown when a larger shape shows up. At most _WS_MAX of them are kept (least recently used withdrawn first); one that a
# stream capture has used is pinned -- the graph holds its address -- until release_workspaces(). A tensor the CALLER registered
# (hgemm_set_workspace) is never replaced or evicted.
_WS_MAX = 8
_ws_need = {}     # (M, N, K) -> bytes the plan of the shape uses (0: single-pass)
_workspaces = {}  # (device, raw stream) -> [tensor, bytes, user, pinned, clock]
_ws_clock = 0
_ws_lock = threading.Lock()  # two host threads on one stream: one of them registers the tensor, the other finds it


def hgemm_workspace_bytes(M, N, K):
    """Bytes of fp32 workspace the split-K / tail-split plan of (M, N, K) uses; 0 = the shape runs single-pass."""
    return int(_loader.load_so("libcln_amd.so").cln_hgemm_workspace_bytes(int(M), int(N), int(K)))


def _ws_need_of(M, N, K):
    need = _ws_need[(M, N, K)] = hgemm_workspace_bytes(M, N, K)
    if len(_ws_need) > 4096:
        _ws_need.clear()
    return need


def _ws_withdraw(key):
    lib = _loader.load_so("libcln_amd.so")
    with torch.cuda.device(key[0]):
        lib.cln_hgemm_set_workspace(None, 0, key[1])
    _workspaces.pop(key, None)


def _ensure_workspace(need):
    """The current stream's workspace holds at least `need` bytes after this call -- or the launch runs single-pass (growth is not allowed while
    the stream is being captured: an allocation made under capture belongs to the graph's private pool)."""
    global _ws_clock
    key = (_current_device(), _stream())
    ent = _workspaces.get(key)
    _ws_clock += 1
    if ent is not None and (ent[1] >= need or ent[2]):
        ent[4] = _ws_clock
        if not ent[3] and torch.cuda.is_current_stream_capturing():
            ent[3] = True
        return
    with _ws_lock:
        _grow_workspace(key, need)


def _grow_workspace(key, need):
    ent = _workspaces.get(key)
    if ent is not None and (ent[1] >= need or ent[2]):
        return
    if torch.cuda.is_current_stream_capturing() or (ent is not None and ent[3]):
        return
    if ent is None:
        free = [k for k, e in _workspaces.items() if not e[2] and not e[3]]
        while len(free) >= _WS_MAX:
            lru = min(free, key=lambda k: _workspaces[k][4])
            free.remove(lru)
            _ws_withdraw(lru)
    size = max(16 << 20, (need + (2 << 20) - 1) // (2 << 20) * (2 << 20))  # whole 2-MiB pages of the caching allocator, 16 MiB at least (few regrowths)
    buf = torch.empty(size, dtype=torch.uint8, device="cuda:%d" % key[0])
    lib = _loader.load_so("libcln_amd.so")
    _raise("cln_hgemm_set_workspace", lib.cln_hgemm_set_workspace(buf.data_ptr(), size, key[1]))
    _workspaces[key] = [buf, size, False, False, _ws_clock]  # the old tensor (if any) goes back to the allocator: launches queued on ITS stream run before any reuse


def hgemm_set_workspace(buf):
    """Give the launches on torch's CURRENT stream a caller-owned workspace: `buf` is a contiguous GPU tensor (any dtype; e.g.
    torch.empty(nbytes, dtype=torch.uint8, device="cuda")), or None to go back to the one this module keeps per stream. The library zeroes the
    first 4 KiB on the stream; shapes that need more than the buffer holds run single-pass."""
    lib = _loader.load_so("libcln_amd.so")
    key = (_current_device(), _stream())
    if buf is None:
        _raise("cln_hgemm_set_workspace", lib.cln_hgemm_set_workspace(None, 0, key[1]))
        _workspaces.pop(key, None)
        return
    _check_dev(buf)
    nbytes = buf.numel() * buf.element_size()
    _raise("cln_hgemm_set_workspace", lib.cln_hgemm_set_workspace(buf.data_ptr(), nbytes, key[1]))
    _workspaces[key] = [buf, nbytes, True, False, _ws_clock]


def release_workspaces():
    """Withdraw every workspace this module registered (their tensors go back to torch's allocator), and free what the library itself holds: the
    scalar-result kernels' ticket slabs and -- after cln_hgemm_library_workspace(1) only -- library-owned split-K buffers. Returns the bytes the
    LIBRARY freed. Call it only when no graph that captured a split-K launch will be replayed again."""
    _workspaces.clear()
    return int(_loader.load_so("libcln_amd.so").cln_release_workspaces())


def hgemm_workspace_held():
    """Bytes of LIBRARY-owned split-K workspace this process currently holds (0 unless cln_hgemm_library_workspace(1) was called)."""
    return int(_loader.load_so("libcln_amd.so").cln_hgemm_workspace_held())


def hgemm_workspace_tensors():
    """(device, raw stream) -> bytes of the workspace tensors this module currently keeps registered (torch-owned)."""
    return {k: e[1] for k, e in _workspaces.items()}


def hgemm_library_workspace(enable):
    """C callers' opt-in to library-owned (hipMalloc) workspaces; this module never needs it. Returns the previous setting."""
    return bool(_loader.load_so("libcln_amd.so").cln_hgemm_library_workspace(int(bool(enable))))


def hgemm_variant(kind, layout, tile, bk, stages, a, b, c, swizzle=0, swizzle_stride=1):
    """Tuning hook (not part of the reference surface; lives in the TEST-ONLY libcln_amd_probe.so): run an explicit
    tile/BK/stage variant."""
    _check_dev(a, b, c)
    M, K = a.size(0), a.size(1)
    N = b.size(1)
    fn = _loader.load_so("libcln_amd_probe.so").cln_hgemm_variant
    rc = fn(kind, layout, tile, bk, stages, a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, int(swizzle),
            int(swizzle_stride), _stream())
    _raise("cln_hgemm_variant", rc, "variant not available for this shape/LDS budget")


def fa2_variant(D_nw_vt_opt_abl, Q, K, V, O):
    """Tuning hook (not part of the reference surface; lives in the TEST-ONLY libcln_amd_probe.so): run an explicit
    FlashAttention kernel variant."""
    _check_dev(Q, K, V, O)
    nw, vt, opt, abl = D_nw_vt_opt_abl
    B, H, N, D = Q.shape
    fn = _loader.load_so("libcln_amd_probe.so").cln_fa2_variant
    rc = fn(D, nw, vt, opt, abl, Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), B, H, N, _stream())
    _raise("cln_fa2_variant", rc, "variant not instantiated / shape not supported")


def fa2_fwd_causal(Q, K, V, O, stages=2):
    """Causal FlashAttention-2 forward (mask key <= query, scale 1/sqrt(D)) into O: fp16 [B,H,N,D] tensors, D in {64, 128},
    N a multiple of 256. C entry cln_fa2_fwd_causal (include/cln_amd_ext.h); no CPU path."""
    fn = _ext_fn("cln_fa2_fwd_causal", [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_void_p])
    for t in (Q, K, V, O):
        _check_dtype(t, torch.float16)
    _check_dev(Q, K, V, O)
    if Q.dim() != 4:
        raise RuntimeError("Tensor size mismatch!")
    B, H, N, D = Q.shape
    for t in (K, V, O):
        _check_shape(t, B, H, N, D)
    rc = fn(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), B, H, N, D, int(stages), _stream())
    _check_bh("fa2_fwd_causal", B, H, N, D, rc)


_lse_fns = {}


def _ext_fn(name, argtypes):
    fn = _lse_fns.get(name)
    if fn is None:
        fn = getattr(_loader.load_so("libcln_amd.so"), name)
        fn.argtypes = argtypes
        fn.restype = ctypes.c_int
        _lse_fns[name] = fn
    return fn


def _check_bh(name, B, H, N, D, rc):
    if rc == -2:
        if D not in (64, 128):
            raise RuntimeError("%s: headdim %d not supported (64 or 128)" % (name, D))
        raise RuntimeError("%s: seqlen %d must be a multiple of 256" % (name, N))
    _raise(name, rc)


def fa2_fwd_lse(Q, K, V, O, LSE, causal=False, stages=2):
    """FlashAttention-2 forward (scale 1/sqrt(D); causal: mask key <= query) into O, and the row log-sum-exp into LSE (fp32 [B,H,N],
    natural log): fp16 [B,H,N,D] tensors, D in {64, 128}, N a multiple of 256. C entries cln_fa2_fwd_lse / cln_fa2_fwd_causal_lse
    (include/cln_amd_ext.h); no CPU path."""
    name = "cln_fa2_fwd_causal_lse" if causal else "cln_fa2_fwd_lse"
    fn = _ext_fn(name, [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_void_p])
    for t in (Q, K, V, O):
        _check_dtype(t, torch.float16)
    _check_dtype(LSE, torch.float32)
    _check_dev(Q, K, V, O, LSE)
    if Q.dim() != 4:
        raise RuntimeError("Tensor size mismatch!")
    B, H, N, D = Q.shape
    for t in (K, V, O):
        _check_shape(t, B, H, N, D)
    _check_shape(LSE, B, H, N)
    rc = fn(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), LSE.data_ptr(), B, H, N, D, int(stages), _stream())
    _check_bh("fa2_fwd_lse", B, H, N, D, rc)


def fa2_bwd(Q, K, V, O, dO, LSE, dQ, dK, dV, delta=None, causal=False):
    """FlashAttention-2 backward into dQ, dK, dV (fp16 [B,H,N,D]) from Q, K, V, O, dO (fp16 [B,H,N,D]) and the forward's LSE (fp32 [B,H,N],
    fa2_fwd_lse). delta: fp32 [B,H,N] scratch that receives rowsum(dO * O); allocated here on the current stream when None. Deterministic.
    C entries cln_fa2_bwd / cln_fa2_bwd_causal (include/cln_amd_ext.h); no CPU path."""
    name = "cln_fa2_bwd_causal" if causal else "cln_fa2_bwd"
    fn = _ext_fn(name, [ctypes.c_void_p] * 10 + [ctypes.c_int] * 4 + [ctypes.c_void_p])
    for t in (Q, K, V, O, dO, dQ, dK, dV):
        _check_dtype(t, torch.float16)
    _check_dtype(LSE, torch.float32)
    _check_dev(Q, K, V, O, dO, LSE, dQ, dK, dV)
    if Q.dim() != 4:
        raise RuntimeError("Tensor size mismatch!")
    B, H, N, D = Q.shape
    for t in (K, V, O, dO, dQ, dK, dV):
        _check_shape(t, B, H, N, D)
    _check_shape(LSE, B, H, N)
    if delta is None:
        delta = torch.empty((B, H, N), dtype=torch.float32, device=Q.device)
    _check_dtype(delta, torch.float32)
    _check_dev(delta)
    _check_shape(delta, B, H, N)
    rc = fn(Q.data_ptr(), K.data_ptr(), V.data_ptr(), O.data_ptr(), dO.data_ptr(), LSE.data_ptr(), delta.data_ptr(),
            dQ.data_ptr(), dK.data_ptr(), dV.data_ptr(), B, H, N, D, _stream())
    _check_bh("fa2_bwd", B, H, N, D, rc)


def _decode_plan(cname, dims):
    """(rc, (splits, chunk, workspace_bytes)) of a cln_fa2_decode*_plan entry for the int tuple dims."""
    fn = _ext_fn(cname, [ctypes.c_int] * len(dims) + [ctypes.c_void_p] * 3)
    s, c, w = ctypes.c_int(), ctypes.c_int(), ctypes.c_longlong()
    rc = fn(*dims, ctypes.addressof(s), ctypes.addressof(c), ctypes.addressof(w))
    return rc, (s.value, c.value, w.value)


def _decode_check(f16, i32, dtype=torch.float16):
    """The dtype and device checks the decode entries share: fp16 (or, for the *_bf16 entries, bf16) tensors, int32 tensors, all on the GPU."""
    for t in f16:
        _check_dtype(t, dtype)
    for t in i32:
        _check_dtype(t, torch.int32)
    _check_dev(*f16, *i32)


def _decode_lse(lse, *shape):
    """The pointer of the optional fp32 lse of that shape."""
    if lse is None:
        return None
    _check_dtype(lse, torch.float32)
    _check_dev(lse)
    _check_shape(lse, *shape)
    return lse.data_ptr()


def _decode_workspace(name, need, workspace, device):
    """(pointer, bytes) of the workspace of entry `name`, whose plan needs `need` bytes: allocated here when None and the plan splits the keys."""
    if workspace is None and need:
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
    if workspace is None:
        return None, 0
    _check_dev(workspace)
    ws_bytes = workspace.numel() * workspace.element_size()
    if ws_bytes < need:
        raise RuntimeError("%s: workspace of %d bytes, the plan needs %d (%s_plan)" % (name, ws_bytes, need, name))
    return workspace.data_ptr(), ws_bytes


def fa2_decode_plan(B, H, Nmax, D):
    """(splits, chunk, workspace_bytes) of fa2_decode for caches of fp16 [B,H,Nmax,D]: a function of these four numbers only
    (cln_fa2_decode_plan, include/cln_amd_ext.h). No GPU needed."""
    rc, plan = _decode_plan("cln_fa2_decode_plan", (int(B), int(H), int(Nmax), int(D)))
    if rc == -2 and D not in (64, 128):
        raise RuntimeError("fa2_decode: headdim %d not supported (64 or 128)" % D)
    _raise("fa2_decode", rc, "fa2_decode: B * H * splits = too many workgroups for one launch")
    return plan


def fa2_decode(q, k_cache, v_cache, seqlens, out, lse=None, workspace=None):
    """Single-query attention over a KV cache into out: q, out fp16 [B,H,D], k_cache, v_cache fp16 [B,H,Nmax,D], seqlens int32 [B] on the GPU
    (clamped to [0, Nmax] by the kernels, never read by the host), lse fp32 [B,H] (natural log) or None; D in {64, 128}. workspace: any
    contiguous GPU tensor of at least fa2_decode_plan(...)[2] bytes; allocated here on the current stream when None and the plan splits the
    keys. Deterministic. C entry cln_fa2_decode (include/cln_amd_ext.h); no CPU path."""
    fn = _ext_fn("cln_fa2_decode", [ctypes.c_void_p] * 7 + [ctypes.c_longlong] + [ctypes.c_int] * 4 + [ctypes.c_void_p])
    _decode_check((q, k_cache, v_cache, out), (seqlens,))
    if q.dim() != 3 or k_cache.dim() != 4:
        raise RuntimeError("Tensor size mismatch!")
    B, H, D = q.shape
    Nmax = k_cache.shape[2]
    _check_shape(k_cache, B, H, Nmax, D)
    _check_shape(v_cache, B, H, Nmax, D)
    _check_shape(out, B, H, D)
    _check_shape(seqlens, B)
    lse_ptr = _decode_lse(lse, B, H)
    ws_ptr, ws_bytes = _decode_workspace("fa2_decode", fa2_decode_plan(B, H, Nmax, D)[2], workspace, q.device)
    rc = fn(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), seqlens.data_ptr(), out.data_ptr(), lse_ptr, ws_ptr, ws_bytes, B, H, Nmax, D,
            _stream())
    _raise("fa2_decode", rc)


_PAGED_GROUPS, _PAGED_PAGES = (1, 2, 4, 8), (16, 32, 64, 128, 256)
_PAGED_GROUPS_ANYG, _PAGED_ROWS_ANYG = tuple(range(1, 17)), 64  # the *_anyg_* entries: any G = Hq / Hkv in 1 … 16; the decode: T * G <= 64
_ROPE_MODES = {"none": 0, "half": 1, "interleaved": 2}


_HEAD_DIMS = (64, 128)  # what every paged entry takes unless its wrapper says otherwise (the *_d256_* wrappers pass (256,): DESIGN 4.4.16)


def _paged_headdim_error(name, D, head_dims):
    if head_dims == _HEAD_DIMS:
        return RuntimeError("%s: headdim %d not supported (64 or 128)" % (name, D))
    return RuntimeError("%s: head dim %d not supported (%s)" % (name, D, " or ".join(map(str, head_dims))))


def _paged_page_error(name, page):
    return RuntimeError("%s: page size %d not supported (16, 32, 64, 128 or 256)" % (name, page))


def _paged_groups(name):
    """The group sizes Hq / Hkv the paged attention entry `name` takes."""
    return _PAGED_GROUPS_ANYG if "_anyg_" in name else _PAGED_GROUPS


def _paged_unsupported(name, B, Hq, Hkv, max_pages, page, D, head_dims=_HEAD_DIMS):
    """The RuntimeError for status -2 of the paged decode entry `name`."""
    if D not in head_dims:
        return _paged_headdim_error(name, D, head_dims)
    if Hkv > 0 and Hq % Hkv == 0 and Hq // Hkv not in _paged_groups(name):
        return RuntimeError("%s: group size %d (= Hq %d / Hkv %d) not supported (%s)"
                            % (name, Hq // Hkv, Hq, Hkv, "1 … 16" if "_anyg_" in name else "1, 2, 4 or 8"))
    if page not in _PAGED_PAGES:
        return _paged_page_error(name, page)
    return RuntimeError("%s: max_pages * page or B * Hkv * splits too large for one launch" % name)


def _fp8_check(k_pages, v_pages, k_scale, v_scale, Hkv):
    """What the FP8 cache entries ask of the pools and scales: torch.float8_e4m3fn pools, fp32 [Hkv] scales, all on the GPU."""
    for t in (k_pages, v_pages):
        _check_dtype(t, torch.float8_e4m3fn)
    for t in (k_scale, v_scale):
        _check_dtype(t, torch.float32)
    _check_dev(k_pages, v_pages, k_scale, v_scale)
    _check_shape(k_scale, Hkv)
    _check_shape(v_scale, Hkv)


def _paged_window(name, window):
    """() without a window, else the one more int of the *_window_* entries: W >= 1."""
    if window is None:
        return ()
    if int(window) < 1:
        raise RuntimeError("%s: window %d not supported (>= 1)" % (name, int(window)))
    return (int(window),)


def _paged_sinks(sinks, q):
    """What the *_sink_* entries ask of sinks before anything else is looked at: a contiguous torch.float32 [Hq], Hq = q's heads (its device is
    checked with the other tensors')."""
    _check_dtype(sinks, torch.float32)
    if sinks.dim() != 1 or q.dim() < 2 or sinks.shape[0] != q.shape[-2]:
        raise RuntimeError("Tensor size mismatch!")
    if not sinks.is_contiguous():
        raise RuntimeError("tensor must be contiguous (the kernels take raw data_ptr())")


def _paged_plan(name, *dims, window=None, head_dims=_HEAD_DIMS, max_rows=_PAGED_ROWS_ANYG):
    """The body of the paged *_plan wrappers: the C entry cln_<name>_plan for dims = (B, Hq, Hkv, max_pages, page, D), or with a T behind B
    for the multi-token entries, and its error texts; `window` goes behind D. head_dims and max_rows (the T * G an any-G entry takes at most)
    are what the entry takes: they choose the text of a -2, never the status."""
    args = tuple(map(int, dims))
    rc, plan = _decode_plan("cln_%s_plan" % name, args + _paged_window(name, window))
    Hq, Hkv, max_pages, page, D = args[-5:]
    if rc == -2:
        dims_ok = D in head_dims
        if len(args) == 7 and dims_ok and args[1] > 8:
            raise RuntimeError("%s: T %d not supported (1 … 8)" % (name, args[1]))
        if (len(args) == 7 and dims_ok and "_anyg_" in name and Hkv > 0 and Hq % Hkv == 0 and Hq // Hkv in _PAGED_GROUPS_ANYG
                and args[1] * (Hq // Hkv) > max_rows):
            raise RuntimeError("%s: T %d x group size %d = %d query rows per KV head not supported (at most %d)"
                               % (name, args[1], Hq // Hkv, args[1] * (Hq // Hkv), max_rows))
        raise _paged_unsupported(name, args[0], Hq, Hkv, max_pages, page, D, head_dims)
    if rc == -1 and Hkv > 0 and Hq % Hkv:
        raise RuntimeError("%s: %d query heads are no multiple of %d KV heads" % (name, Hq, Hkv))
    _raise(name, rc)
    return plan


def _paged_attention(name, dtype, q_dims, plan, q, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, out, lse, workspace,
                     window=None, sinks=None, sinks_optional=False, floats=(), head_dims=_HEAD_DIMS):
    """The body of every attention entry over a paged cache. q, out: dtype [B,Hq,D] (q_dims = 3) or [B,T,Hq,D] (4), or with cu_q the packed
    [total_q,Hq,D]; the pools hold dtype, or with k_scale / v_scale e4m3; plan = the *_plan of a decode entry, which splits the keys and takes
    a workspace, or None for a prefill entry: one launch, and what cannot be launched is told here, in the words of the plan. window = the W of
    a sliding-window entry: one more int behind D, for the entry and its plan. sinks = the fp32 [Hq] of a *_sink_* entry: the last input pointer;
    sinks_optional: the entry has that pointer and takes NULL for sinks = None. floats = the (softmax_scale, softcap) of a *_softcap_* entry
    (_paged_softcap): two floats behind the window, for the entry but not for its plan."""
    packed, fp8, sink = cu_q is not None, k_scale is not None, sinks is not None
    sink_ptr = sink or sinks_optional
    win = _paged_window(name, window)
    if sink:
        _paged_sinks(sinks, q)
    fn = _lse_fns.get("cln_" + name) or _ext_fn(  # the prototype is put together on the first call only
        "cln_" + name, [ctypes.c_void_p] * (7 + packed + 2 * fp8 + sink_ptr) + ([ctypes.c_void_p, ctypes.c_longlong] if plan else [])
        + [ctypes.c_int] * (q_dims + 4 + packed + len(win)) + [ctypes.c_float] * len(floats) + [ctypes.c_void_p])
    _decode_check((q, out) if fp8 else (q, k_pages, v_pages, out), (block_table, seqlens, cu_q) if packed else (block_table, seqlens), dtype)
    if sink:
        _check_dev(sinks)
    if q.dim() != q_dims or k_pages.dim() != 4 or block_table.dim() != 2:
        raise RuntimeError("Tensor size mismatch!")
    *lead, D = q.shape  # lead = [B, Hq], [B, T, Hq] or [total_q, Hq]
    P, Hkv, page, _ = k_pages.shape
    if fp8:
        _fp8_check(k_pages, v_pages, k_scale, v_scale, Hkv)
    B, max_pages = block_table.shape
    _check_shape(k_pages, P, Hkv, page, D)
    _check_shape(v_pages, P, Hkv, page, D)
    if not packed and B != lead[0]:
        raise RuntimeError("Tensor size mismatch!")
    _check_shape(out, *lead, D)
    _check_shape(seqlens, B)
    if packed:
        _check_shape(cu_q, B + 1)
    if lse is not None:
        _check_dtype(lse, torch.float32)
        _check_dev(lse)
        _check_shape(lse, *lead)
    if plan:
        ws, too_large = _decode_workspace(name, plan(*lead, Hkv, max_pages, page, D, *win)[2], workspace, q.device), None
    else:
        Hq = lead[-1]
        if Hq % Hkv:
            raise RuntimeError("%s: %d query heads are no multiple of %d KV heads" % (name, Hq, Hkv))
        if D not in head_dims or Hq // Hkv not in _paged_groups(name) or page not in _PAGED_PAGES:
            raise _paged_unsupported(name, B, Hq, Hkv, max_pages, page, D, head_dims)
        ws = ()
        too_large = ("%s: max_pages * page or Hkv * (total_q * Hq / Hkv / 128 + B) too large for one launch" if packed else
                     "%s: max_pages * page or B * Hkv * ceil(T * Hq / Hkv / 128) too large for one launch") % name
    more = ((cu_q.data_ptr(),) if packed else ()) + ((k_scale.data_ptr(), v_scale.data_ptr()) if fp8 else ())
    if sink_ptr:
        more += (sinks.data_ptr() if sink else None,)
    rc = fn(q.data_ptr(), k_pages.data_ptr(), v_pages.data_ptr(), block_table.data_ptr(), seqlens.data_ptr(), *more, out.data_ptr(),
            None if lse is None else lse.data_ptr(), *ws, *((B, *lead) if packed else lead), Hkv, P, max_pages, page, D, *win, *floats, _stream())
    _raise(name, rc, too_large)


def _rope_table_max_pos(rope_table, D):
    """The max_pos of the optional fp32 rope_table [max_pos, D] of an append entry; 0 without one."""
    if rope_table is None:
        return 0
    _check_dtype(rope_table, torch.float32)
    _check_dev(rope_table)
    if rope_table.dim() != 2:
        raise RuntimeError("Tensor size mismatch!")
    _check_shape(rope_table, rope_table.shape[0], D)
    return rope_table.shape[0]


def _kv_append_paged(name, dtype, k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, q, q_out, rope_table, rope,
                     head_dims=_HEAD_DIMS):
    """The body of every append entry. k_new, v_new: dtype [B,T,Hkv,D], or with cu_q the packed [total_q,Hkv,D]; q, q_out alike with Hq heads;
    the pools hold dtype, or with k_scale / v_scale e4m3."""
    packed, fp8 = cu_q is not None, k_scale is not None
    fn = _lse_fns.get("cln_" + name) or _ext_fn(  # the prototype is put together on the first call only
        "cln_" + name, [ctypes.c_void_p] * (9 + packed + 2 * fp8) + [ctypes.c_int] * 10 + [ctypes.c_void_p])
    if rope not in _ROPE_MODES:
        raise RuntimeError("%s: rope %r not supported ('none', 'half' or 'interleaved')" % (name, rope))
    mode = _ROPE_MODES[rope]
    if mode == 0 and not (q is None and q_out is None and rope_table is None):
        raise RuntimeError("%s: rope 'none' takes no q, q_out or rope_table" % name)
    if mode != 0 and rope_table is None:
        raise RuntimeError("%s: rope %r needs a rope_table (kv_append_rope_table)" % (name, rope))
    if (q is None) != (q_out is None):
        raise RuntimeError("%s: q and q_out are given together or not at all" % name)
    rows = ((k_new, v_new) if fp8 else (k_new, v_new, k_pages, v_pages)) + ((q, q_out) if q is not None else ())
    _decode_check(rows, (block_table, seqlens, cu_q) if packed else (block_table, seqlens), dtype)
    if k_new.dim() != (3 if packed else 4) or k_pages.dim() != 4 or block_table.dim() != 2:
        raise RuntimeError("Tensor size mismatch!")
    *lead, Hkv, D = k_new.shape  # lead = [B, T] or [total_q]
    P, _, page, _ = k_pages.shape
    if fp8:
        _fp8_check(k_pages, v_pages, k_scale, v_scale, Hkv)
    B, max_pages = block_table.shape
    _check_shape(v_new, *lead, Hkv, D)
    _check_shape(k_pages, P, Hkv, page, D)
    _check_shape(v_pages, P, Hkv, page, D)
    if not packed and B != lead[0]:
        raise RuntimeError("Tensor size mismatch!")
    _check_shape(seqlens, B)
    if packed:
        _check_shape(cu_q, B + 1)
    Hq = Hkv
    if q is not None:
        if q.dim() != k_new.dim():
            raise RuntimeError("Tensor size mismatch!")
        Hq = q.shape[-2]
        _check_shape(q, *lead, Hq, D)
        _check_shape(q_out, *lead, Hq, D)
    max_pos = _rope_table_max_pos(rope_table, D)
    if D not in head_dims:
        raise _paged_headdim_error(name, D, head_dims)
    if page not in _PAGED_PAGES:
        raise _paged_page_error(name, page)
    if Hq % Hkv:
        raise RuntimeError("%s: %d query heads are no multiple of %d KV heads" % (name, Hq, Hkv))
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    more = ((cu_q.data_ptr(),) if packed else ()) + ((k_scale.data_ptr(), v_scale.data_ptr()) if fp8 else ())
    rc = fn(k_new.data_ptr(), v_new.data_ptr(), k_pages.data_ptr(), v_pages.data_ptr(), block_table.data_ptr(), seqlens.data_ptr(), *more, ptr(q),
            ptr(q_out), ptr(rope_table), *((B, *lead) if packed else lead), Hq, Hkv, P, max_pages, page, D, max_pos, mode, _stream())
    _raise(name, rc, ("%s: max_pages * page or total_q too large for one launch" if packed else
                      "%s: max_pages * page or B * T too large for one launch") % name)


def fa2_decode_paged_plan(B, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged: a function of these six numbers only (cln_fa2_decode_paged_plan,
    include/cln_amd_ext.h). No GPU needed."""
    return _paged_plan("fa2_decode_paged", B, Hq, Hkv, max_pages, page, D)


def fa2_decode_paged(q, k_pages, v_pages, block_table, seqlens, out, lse=None, workspace=None):
    """Single-query attention over a paged KV cache with grouped query heads into out: q, out fp16 [B,Hq,D]; k_pages, v_pages fp16
    [P,Hkv,page,D]; block_table int32 [B,max_pages] and seqlens int32 [B] on the GPU (never read by the host; lengths clamped to
    [0, max_pages * page] by the kernels; the live table entries must lie in [0, P)); lse fp32 [B,Hq] (natural log) or None. D in {64, 128},
    Hq / Hkv in {1, 2, 4, 8}, page in {16, 32, 64, 128, 256}. workspace: any contiguous GPU tensor of at least fa2_decode_paged_plan(...)[2]
    bytes; allocated here on the current stream when None and the plan splits the keys. Deterministic. C entry cln_fa2_decode_paged
    (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_decode_paged", torch.float16, 3, fa2_decode_paged_plan, q, k_pages, v_pages, block_table, seqlens, None, None, None, out,
                     lse,
                     workspace)


def fa2_decode_paged_multi_plan(B, T, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi: a function of these seven numbers only (cln_fa2_decode_paged_multi_plan,
    include/cln_amd_ext.h). No GPU needed."""
    return _paged_plan("fa2_decode_paged_multi", B, T, Hq, Hkv, max_pages, page, D)


def fa2_decode_paged_multi(q, k_pages, v_pages, block_table, seqlens, out, lse=None, workspace=None):
    """Multi-token (speculative verify / short append) attention over a paged KV cache with grouped query heads into out: q, out fp16
    [B,T,Hq,D]; k_pages, v_pages fp16 [P,Hkv,page,D]; block_table int32 [B,max_pages] and seqlens int32 [B] on the GPU (never read by the host;
    lengths clamped to [0, max_pages * page] by the kernels; the live table entries must lie in [0, P)); lse fp32 [B,T,Hq] (natural log) or
    None. seqlens[b] counts the T newest tokens, whose K / V rows are already in the pool; query t sees the keys j < len_b - (T - 1 - t), and
    a query that sees none gets O = 0 and LSE = -inf. T in 1 … 8, D in {64, 128}, Hq / Hkv in {1, 2, 4, 8}, page in {16, 32, 64, 128, 256}.
    workspace: any contiguous GPU tensor of at least fa2_decode_paged_multi_plan(...)[2] bytes; allocated here on the current stream when None
    and the plan splits the keys. Deterministic. C entry cln_fa2_decode_paged_multi (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_decode_paged_multi", torch.float16, 4, fa2_decode_paged_multi_plan, q, k_pages, v_pages, block_table, seqlens, None, None,
                     None,
                     out, lse, workspace)


def kv_append_rope_table(max_pos, D, theta=10000.0, device=None):
    """The cos / sin table kv_append_paged rotates with: fp32 [max_pos, D], row p = cos(p f_i) for i < D/2, then sin(p f_i), with
    f_i = theta^(-2i/D). The angles are formed in float64 and cast once."""
    max_pos, D = int(max_pos), int(D)
    if max_pos <= 0 or D <= 0 or D % 2:
        raise RuntimeError("kv_append_rope_table: max_pos %d and an even D %d must be positive" % (max_pos, D))
    freq = torch.tensor(float(theta), dtype=torch.float64) ** (-2.0 * torch.arange(D // 2, dtype=torch.float64) / D)
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * freq[None, :]
    return torch.cat((torch.cos(ang), torch.sin(ang)), dim=1).to(torch.float32).to(device)


def kv_append_paged(k_new, v_new, k_pages, v_pages, block_table, seqlens, q=None, q_out=None, rope_table=None, rope="none"):
    """Write the K / V rows of T new tokens per sequence into a paged KV cache, with the rotary embedding of K and q fused in; one launch.
    k_new, v_new fp16 [B,T,Hkv,D]; k_pages, v_pages fp16 [P,Hkv,page,D], written in place; block_table int32 [B,max_pages] and seqlens int32 [B]
    on the GPU (never read by the host). seqlens[b] counts the T new tokens, as for fa2_decode_paged_multi: token t stands at
    pos = seqlens[b] - T + t and is live iff 0 <= pos < max_pages * page (and pos < max_pos with a rotation); a live token's rows go to row
    pos % page of page block_table[b, pos // page], a token that is not live writes nothing to the pools and zeros to its q_out rows.
    rope: "none" (rows copied bit for bit; q, q_out, rope_table must be None), "half" (pairs (i, i + D/2)) or "interleaved" (pairs (2i, 2i+1)),
    rotated in fp32 by rope_table fp32 [max_pos, D] (kv_append_rope_table) with one rounding; V is never rotated. q, q_out fp16 [B,T,Hq,D],
    given together or both None; q_out may be q. The live table entries must lie in [0, P) and name distinct pages. D in {64, 128}, page in
    {16, 32, 64, 128, 256}, Hq a multiple of Hkv, any T. Deterministic. C entry cln_kv_append_paged (include/cln_amd_ext.h); no CPU path."""
    _kv_append_paged("kv_append_paged", torch.float16, k_new, v_new, k_pages, v_pages, block_table, seqlens, None, None, None, q, q_out, rope_table,
                     rope)


def fa2_prefill_paged(q, k_pages, v_pages, block_table, seqlens, out, lse=None):
    """Prefill attention (a prompt or a chunk of one) over a paged KV cache with grouped query heads into out; one launch, no workspace. The
    tensors and the semantics of fa2_decode_paged_multi with any T >= 1: q, out fp16 [B,T,Hq,D]; k_pages, v_pages fp16 [P,Hkv,page,D];
    block_table int32 [B,max_pages] and seqlens int32 [B] on the GPU (never read by the host; lengths clamped to [0, max_pages * page] by the
    kernel; the live table entries must lie in [0, P)); lse fp32 [B,T,Hq] (natural log) or None. seqlens[b] counts the T newest tokens, whose
    K / V rows are already in the pool (kv_append_paged); query t sees the keys j < len_b - (T - 1 - t), and a query that sees none gets O = 0
    and LSE = -inf, so a sequence with len_b < T has its live tokens right-aligned: that is how a ragged prefill batch is expressed. D in
    {64, 128}, Hq / Hkv in {1, 2, 4, 8}, page in {16, 32, 64, 128, 256}. Deterministic. C entry cln_fa2_prefill_paged
    (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_prefill_paged", torch.float16, 4, None, q, k_pages, v_pages, block_table, seqlens, None, None, None, out, lse, None)


def fa2_prefill_paged_varlen(q, k_pages, v_pages, block_table, seqlens, cu_q, out, lse=None):
    """fa2_prefill_paged for a packed batch with a per-sequence number of new tokens; one launch, no workspace. q, out fp16 [total_q,Hq,D]; lse
    fp32 [total_q,Hq] (natural log) or None; cu_q int32 [B+1] on the GPU, non-decreasing with 0 <= cu_q[0] and cu_q[B] <= total_q (never read by
    the host: the grid comes from B and total_q): the tokens of sequence b are the packed rows cu_q[b] .. cu_q[b+1]-1, T_b of them (0 is
    allowed). k_pages, v_pages, block_table [B,max_pages] and seqlens [B] as for fa2_prefill_paged; seqlens[b] counts the T_b newest tokens,
    token i sees the keys j < len_b - (T_b - 1 - i), and a query that sees none gets O = 0 and LSE = -inf. Packed rows outside
    [cu_q[0], cu_q[B]) are neither read nor written. A sequence's bits are those of fa2_prefill_paged on that sequence alone. D in {64, 128},
    Hq / Hkv in {1, 2, 4, 8}, page in {16, 32, 64, 128, 256}. Deterministic. C entry cln_fa2_prefill_paged_varlen (include/cln_amd_ext.h); no
    CPU path."""
    _paged_attention("fa2_prefill_paged_varlen", torch.float16, 3, None, q, k_pages, v_pages, block_table, seqlens, cu_q, None, None, out, lse, None)


def kv_append_paged_varlen(k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, q=None, q_out=None, rope_table=None, rope="none"):
    """kv_append_paged for a packed batch with a per-sequence number of new tokens; one launch. k_new, v_new fp16 [total_q,Hkv,D]; q, q_out fp16
    [total_q,Hq,D], given together or both None (q_out may be q); cu_q int32 [B+1] on the GPU as for fa2_prefill_paged_varlen (never read by
    the host). Token i of sequence b is packed row cu_q[b] + i and stands at pos = seqlens[b] - T_b + i; liveness, rope, rope_table, the pools,
    the table and the caller's contract are those of kv_append_paged. Packed rows outside [cu_q[0], cu_q[B]) are neither read nor written.
    Deterministic. C entry cln_kv_append_paged_varlen (include/cln_amd_ext.h); no CPU path."""
    _kv_append_paged("kv_append_paged_varlen", torch.float16, k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, None, None, q, q_out,
                     rope_table,
                     rope)


def kv_append_paged_varlen_bf16(k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, q=None, q_out=None, rope_table=None, rope="none"):
    """kv_append_paged_varlen on bf16 tensors: k_new, v_new, q, q_out and the pools torch.bfloat16, rope_table fp32; everything else -- shapes,
    liveness, rope, the caller's contract, the errors -- as there. The rotation runs in fp32 from the bf16 inputs with one rounding to bf16 (round
    to nearest even); V rows and rope "none" rows are copied bit for bit. A fixed T is cu_q = T * arange(B + 1). Deterministic. C entry
    cln_kv_append_paged_varlen_bf16 (include/cln_amd_ext.h); no CPU path."""
    _kv_append_paged("kv_append_paged_varlen_bf16", torch.bfloat16, k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, None, None, q, q_out,
                     rope_table, rope)


def fa2_prefill_paged_varlen_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, out, lse=None):
    """fa2_prefill_paged_varlen on bf16 tensors: q, out and the pools torch.bfloat16, lse fp32; everything else as there. K, V and q are bf16
    operands of the matrix cores, scores and accumulators fp32, P rounded once to bf16, O rounded once to bf16 at the store; nothing passes
    through fp16. A fixed T is cu_q = T * arange(B + 1). Deterministic. C entry cln_fa2_prefill_paged_varlen_bf16 (include/cln_amd_ext.h); no
    CPU path."""
    _paged_attention("fa2_prefill_paged_varlen_bf16", torch.bfloat16, 3, None, q, k_pages, v_pages, block_table, seqlens, cu_q, None, None, out, lse,
                     None)


def fa2_decode_paged_multi_bf16_plan(B, T, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_bf16: what fa2_decode_paged_multi_plan returns for the same seven numbers (the
    workspace is fp32 either way), from cln_fa2_decode_paged_multi_bf16_plan (include/cln_amd_ext.h). No GPU needed."""
    return _paged_plan("fa2_decode_paged_multi_bf16", B, T, Hq, Hkv, max_pages, page, D)


def fa2_decode_paged_multi_bf16(q, k_pages, v_pages, block_table, seqlens, out, lse=None, workspace=None):
    """fa2_decode_paged_multi on bf16 tensors: q, out [B,T,Hq,D] and the pools torch.bfloat16, lse and the workspace fp32; T in 1 … 8 and
    everything else as there, with fa2_decode_paged_multi_bf16_plan(...)[2] workspace bytes. The numerics of fa2_prefill_paged_varlen_bf16; the
    split partials and their merge are fp32. Deterministic. C entry cln_fa2_decode_paged_multi_bf16 (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_decode_paged_multi_bf16", torch.bfloat16, 4, fa2_decode_paged_multi_bf16_plan, q, k_pages, v_pages, block_table, seqlens,
                     None, None,
                     None, out, lse, workspace)


def fa2_prefill_paged_varlen_window_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, out, lse=None):
    """fa2_prefill_paged_varlen_bf16 with a sliding window of `window` = W >= 1 keys: the query token at position p = len_b - T_b + t sees the
    keys max(0, p - W + 1) … p (HF sliding_window = W, FlashAttention window_size = (W - 1, 0)); everything else as there, and with
    W >= max_pages * page its bits. A tile walks about W + 128 / G + 128 keys whatever the length, and reads no table entry or pool row of a page
    that ends at or before align_down(max(0, len_b - T_b - W + 1), max(page, 64)). C entry cln_fa2_prefill_paged_varlen_window_bf16
    (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_prefill_paged_varlen_window_bf16", torch.bfloat16, 3, None, q, k_pages, v_pages, block_table, seqlens, cu_q, None, None,
                     out, lse, None, window)


def fa2_decode_paged_multi_window_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_bf16: the splits divide the span
    min(max_pages * page, round_up(window + T - 1, U) + U), U = max(page, 128), not max_pages * page; a function of these eight numbers only, and
    with window >= max_pages * page what fa2_decode_paged_multi_bf16_plan returns (cln_fa2_decode_paged_multi_window_bf16_plan,
    include/cln_amd_ext.h). No GPU needed."""
    return _paged_plan("fa2_decode_paged_multi_window_bf16", B, T, Hq, Hkv, max_pages, page, D, window=window)


def fa2_decode_paged_multi_window_bf16(q, k_pages, v_pages, block_table, seqlens, window, out, lse=None, workspace=None):
    """fa2_decode_paged_multi_bf16 with a sliding window of `window` = W >= 1 keys (the mask of fa2_prefill_paged_varlen_window_bf16); T in
    1 … 8 and everything else as there, with fa2_decode_paged_multi_window_bf16_plan(...)[2] workspace bytes, and with W >= max_pages * page its
    bits. Reads no table entry or pool row of a page that ends at or before align_down(max(0, len_b - T - W + 1), max(page, 128)). C entry
    cln_fa2_decode_paged_multi_window_bf16 (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_decode_paged_multi_window_bf16", torch.bfloat16, 4, fa2_decode_paged_multi_window_bf16_plan, q, k_pages, v_pages,
                     block_table, seqlens, None, None, None, out, lse, workspace, window)


_NO_WINDOW = 2 ** 31 - 1  # what window = None of the *_sink_* entries passes: a window past any cache


def fa2_prefill_paged_varlen_window_sink_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, sinks, out, lse=None):
    """fa2_prefill_paged_varlen_window_bf16 with attention sinks: sinks a contiguous torch.float32 [Hq] on q's device, one logit per query head in
    natural-log units as the model stores it (sinks.float(); NOT scaled by 1/sqrt(D)), which joins the softmax denominator of every row of its
    head and carries no value: O = sum_j exp(s_j) v_j / (sum_j exp(s_j) + exp(sinks[h])), lse = ln of that denominator, the sink included. A
    row that sees no key stays O = 0, LSE = -inf. window = None: no window (2**31 - 1), the full-attention layers of gpt-oss. sinks of -inf
    give the bits of fa2_prefill_paged_varlen_window_bf16; everything else as there. C entry cln_fa2_prefill_paged_varlen_window_sink_bf16
    (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_prefill_paged_varlen_window_sink_bf16", torch.bfloat16, 3, None, q, k_pages, v_pages, block_table, seqlens, cu_q, None,
                     None, out, lse, None, _NO_WINDOW if window is None else window, sinks)


def fa2_decode_paged_multi_window_sink_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_bf16: what fa2_decode_paged_multi_window_bf16_plan returns for the
    same numbers -- the sink changes neither the splits nor the workspace; window = None: no window (2**31 - 1)
    (cln_fa2_decode_paged_multi_window_sink_bf16_plan, include/cln_amd_ext.h). No GPU needed."""
    return _paged_plan("fa2_decode_paged_multi_window_sink_bf16", B, T, Hq, Hkv, max_pages, page, D, window=_NO_WINDOW if window is None else window)


def fa2_decode_paged_multi_window_sink_bf16(q, k_pages, v_pages, block_table, seqlens, window, sinks, out, lse=None, workspace=None):
    """fa2_decode_paged_multi_window_bf16 with attention sinks (sinks, lse and the rows that see no key as for
    fa2_prefill_paged_varlen_window_sink_bf16); T in 1 … 8, fa2_decode_paged_multi_window_sink_bf16_plan(...)[2] workspace bytes. The sink enters
    once per row whatever the number of splits: at the final store with one split, in the combine with more. window = None: no window. C entry
    cln_fa2_decode_paged_multi_window_sink_bf16 (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_decode_paged_multi_window_sink_bf16", torch.bfloat16, 4, fa2_decode_paged_multi_window_sink_bf16_plan, q, k_pages,
                     v_pages, block_table, seqlens, None, None, None, out, lse, workspace, _NO_WINDOW if window is None else window, sinks)


def fa2_decode_paged_fp8_plan(B, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_fp8: a function of these six numbers only (cln_fa2_decode_paged_fp8_plan,
    include/cln_amd_ext.h); the key step is that of the FP8 kernel, so it may differ from fa2_decode_paged_plan. No GPU needed."""
    return _paged_plan("fa2_decode_paged_fp8", B, Hq, Hkv, max_pages, page, D)


def fa2_decode_paged_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, out, lse=None, workspace=None):
    """Single-query attention over a paged KV cache held in FP8, with grouped query heads, into out: q, out fp16 [B,Hq,D]; k_pages, v_pages
    torch.float8_e4m3fn [P,Hkv,page,D]; k_scale, v_scale fp32 [Hkv], block_table int32 [B,max_pages] and seqlens int32 [B] on the GPU (never
    read by the host). A stored byte c of KV head h means e4m3(c) * scale[h]; the scales must be finite and > 0 and the live bytes no NaN code
    (the caller's contract, not checked). lse fp32 [B,Hq] (natural log) or None. Lengths, table entries, D, Hq / Hkv, page and workspace as for
    fa2_decode_paged, with fa2_decode_paged_fp8_plan(...)[2] bytes. Deterministic. C entry cln_fa2_decode_paged_fp8 (include/cln_amd_ext.h);
    no CPU path."""
    _paged_attention("fa2_decode_paged_fp8", torch.float16, 3, fa2_decode_paged_fp8_plan, q, k_pages, v_pages, block_table, seqlens, None, k_scale,
                     v_scale, out,
                     lse, workspace)


def fa2_decode_paged_multi_fp8_plan(B, T, Hq, Hkv, max_pages, page, D):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_fp8: a function of these seven numbers only
    (cln_fa2_decode_paged_multi_fp8_plan, include/cln_amd_ext.h); the key step is that of fa2_decode_paged_multi. No GPU needed."""
    return _paged_plan("fa2_decode_paged_multi_fp8", B, T, Hq, Hkv, max_pages, page, D)


def fa2_decode_paged_multi_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, out, lse=None, workspace=None):
    """fa2_decode_paged_multi over a paged KV cache held in FP8: q, out fp16 [B,T,Hq,D]; k_pages, v_pages torch.float8_e4m3fn [P,Hkv,page,D];
    k_scale, v_scale fp32 [Hkv], block_table int32 [B,max_pages] and seqlens int32 [B] on the GPU (never read by the host). A stored byte c of
    KV head h means e4m3(c) * scale[h]; the scales must be finite and > 0 and the live bytes no NaN code (the caller's contract, not checked).
    lse fp32 [B,T,Hq] (natural log) or None. T, lengths, table entries, D, Hq / Hkv, page and workspace as for fa2_decode_paged_multi, with
    fa2_decode_paged_multi_fp8_plan(...)[2] bytes. Deterministic. C entry cln_fa2_decode_paged_multi_fp8 (include/cln_amd_ext.h); no CPU
    path."""
    _paged_attention("fa2_decode_paged_multi_fp8", torch.float16, 4, fa2_decode_paged_multi_fp8_plan, q, k_pages, v_pages, block_table, seqlens,
                     None, k_scale,
                     v_scale, out, lse, workspace)


def fa2_prefill_paged_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, out, lse=None):
    """fa2_prefill_paged over a paged KV cache held in FP8; one launch, no workspace: q, out fp16 [B,T,Hq,D], any T >= 1; k_pages, v_pages
    torch.float8_e4m3fn [P,Hkv,page,D]; k_scale, v_scale fp32 [Hkv], block_table int32 [B,max_pages] and seqlens int32 [B] on the GPU (never
    read by the host). A stored byte c of KV head h means e4m3(c) * scale[h]; the scales must be finite and > 0 and the live bytes no NaN code
    (the caller's contract, not checked). lse fp32 [B,T,Hq] (natural log) or None. Lengths, the right-aligned ragged batch, table entries, D,
    Hq / Hkv and page as for fa2_prefill_paged. Deterministic. C entry cln_fa2_prefill_paged_fp8 (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_prefill_paged_fp8", torch.float16, 4, None, q, k_pages, v_pages, block_table, seqlens, None, k_scale, v_scale, out, lse,
                     None)


def kv_append_paged_fp8(k_new, v_new, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, q=None, q_out=None, rope_table=None, rope="none"):
    """kv_append_paged into a cache held in FP8; one launch. k_new, v_new fp16 [B,T,Hkv,D]; k_pages, v_pages torch.float8_e4m3fn
    [P,Hkv,page,D], written in place; k_scale, v_scale fp32 [Hkv], block_table int32 [B,max_pages] and seqlens int32 [B] on the GPU (never read
    by the host). Positions, liveness, rope, q, q_out and rope_table are those of kv_append_paged; q is rotated and written as fp16 without a
    scale. Every element of a live K or V row is stored as e4m3(clamp(y * (1 / scale[h]), -448, 448)), fp32 arithmetic, round to nearest even,
    y the fp16 input or the fp32 rotation result (not rounded to fp16 in between). The scales must be finite and > 0 and the inputs finite
    (the caller's contract, not checked). Deterministic. C entry cln_kv_append_paged_fp8 (include/cln_amd_ext.h); no CPU path."""
    _kv_append_paged("kv_append_paged_fp8", torch.float16, k_new, v_new, k_pages, v_pages, block_table, seqlens, None, k_scale, v_scale, q, q_out,
                     rope_table,
                     rope)


def kv_append_paged_varlen_bf16_fp8(k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, q=None, q_out=None,
                                    rope_table=None, rope="none"):
    """kv_append_paged_varlen_bf16 into a cache held in FP8; one launch. k_new, v_new torch.bfloat16 [total_q,Hkv,D]; k_pages, v_pages
    torch.float8_e4m3fn [P,Hkv,page,D], written in place; k_scale, v_scale fp32 [Hkv] on the GPU. The packed rows, cu_q, positions, liveness,
    rope, q, q_out and rope_table are those of kv_append_paged_varlen_bf16; q is rotated and written as bf16 without a scale. Every element of a
    live K or V row is stored as e4m3(clamp(y * (1 / scale[h]), -448, 448)), fp32 arithmetic, round to nearest even, y the bf16 input or the fp32
    rotation result (not rounded to bf16 in between). The scales must be finite and > 0 and the inputs finite (the caller's contract, not
    checked). Deterministic. C entry cln_kv_append_paged_varlen_bf16_fp8 (include/cln_amd_ext.h); no CPU path."""
    _kv_append_paged("kv_append_paged_varlen_bf16_fp8", torch.bfloat16, k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale,
                     q, q_out, rope_table, rope)


def fa2_prefill_paged_varlen_window_sink_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, window, sinks, out, lse=None):
    """fa2_prefill_paged_varlen_window_sink_bf16 over a paged KV cache held in FP8: q, out torch.bfloat16 [total_q,Hq,D]; k_pages, v_pages
    torch.float8_e4m3fn [P,Hkv,page,D]; k_scale, v_scale fp32 [Hkv] on the GPU. A stored byte c of KV head h means e4m3(c) * scale[h]; the scales
    must be finite and > 0 and the live bytes no NaN code (the caller's contract, not checked). The function is that of the bf16 entry on the
    dequantised pools: the codes become bf16 exactly, k_scale multiplies the fp32 score multiplier and v_scale the normalisation; nothing passes
    through fp16. window = None: no window (2**31 - 1). sinks = None: no sink, the bits of sinks that are all -inf. Everything else as there. C
    entry cln_fa2_prefill_paged_varlen_window_sink_bf16_fp8 (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_prefill_paged_varlen_window_sink_bf16_fp8", torch.bfloat16, 3, None, q, k_pages, v_pages, block_table, seqlens, cu_q,
                     k_scale, v_scale, out, lse, None, _NO_WINDOW if window is None else window, sinks, True)


def fa2_decode_paged_multi_window_sink_bf16_fp8_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_bf16_fp8: what fa2_decode_paged_multi_window_bf16_plan returns for
    the same numbers -- neither the FP8 pools nor the sink change the splits or the fp32 workspace; window = None: no window (2**31 - 1)
    (cln_fa2_decode_paged_multi_window_sink_bf16_fp8_plan, include/cln_amd_ext.h). No GPU needed."""
    return _paged_plan("fa2_decode_paged_multi_window_sink_bf16_fp8", B, T, Hq, Hkv, max_pages, page, D,
                       window=_NO_WINDOW if window is None else window)


def fa2_decode_paged_multi_window_sink_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, window, sinks, out, lse=None,
                                                workspace=None):
    """fa2_decode_paged_multi_window_sink_bf16 over a paged KV cache held in FP8 (pools, scales, numerics, window = None and sinks = None as for
    fa2_prefill_paged_varlen_window_sink_bf16_fp8; v_scale multiplies each split's fp32 partial); q, out torch.bfloat16 [B,T,Hq,D], T in 1 … 8,
    fa2_decode_paged_multi_window_sink_bf16_fp8_plan(...)[2] workspace bytes. C entry cln_fa2_decode_paged_multi_window_sink_bf16_fp8
    (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_decode_paged_multi_window_sink_bf16_fp8", torch.bfloat16, 4, fa2_decode_paged_multi_window_sink_bf16_fp8_plan, q, k_pages,
                     v_pages, block_table, seqlens, None, k_scale, v_scale, out, lse, workspace, _NO_WINDOW if window is None else window, sinks,
                     True)


def fa2_prefill_paged_varlen_window_sink_anyg_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, sinks, out, lse=None):
    """fa2_prefill_paged_varlen_window_sink_bf16 for any group size Hq / Hkv in 1 … 16 (3, 5, 6, 7, 12, 16 …), not a power of two only: tensors,
    lengths, window, sinks, lse and errors as there, and for Hq / Hkv in {1, 2, 4, 8} its bits. window = None: no window (2**31 - 1). sinks =
    None: no sink, the bits of sinks that are all -inf. C entry cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16 (include/cln_amd_ext.h); no
    CPU path."""
    _paged_attention("fa2_prefill_paged_varlen_window_sink_anyg_bf16", torch.bfloat16, 3, None, q, k_pages, v_pages, block_table, seqlens, cu_q,
                     None, None, out, lse, None, _NO_WINDOW if window is None else window, sinks, True)


def fa2_decode_paged_multi_window_sink_anyg_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_anyg_bf16: for Hq / Hkv in {1, 2, 4, 8} what
    fa2_decode_paged_multi_window_sink_bf16_plan returns, and the same function of (B * Hkv, B * T * Hq, span, unit, D) for every other Hq / Hkv
    in 1 … 16; T in 1 … 8 with T * Hq / Hkv <= 64; window = None: no window (2**31 - 1)
    (cln_fa2_decode_paged_multi_window_sink_anyg_bf16_plan, include/cln_amd_ext.h). No GPU needed."""
    return _paged_plan("fa2_decode_paged_multi_window_sink_anyg_bf16", B, T, Hq, Hkv, max_pages, page, D,
                       window=_NO_WINDOW if window is None else window)


def fa2_decode_paged_multi_window_sink_anyg_bf16(q, k_pages, v_pages, block_table, seqlens, window, sinks, out, lse=None, workspace=None):
    """fa2_decode_paged_multi_window_sink_bf16 for any group size Hq / Hkv in 1 … 16: q, out torch.bfloat16 [B,T,Hq,D], T in 1 … 8 with
    T * Hq / Hkv <= 64 (G = 16: T <= 4, G = 12: T <= 5), fa2_decode_paged_multi_window_sink_anyg_bf16_plan(...)[2] workspace bytes; for Hq / Hkv
    in {1, 2, 4, 8} the sibling's bits. window = None: no window. sinks = None: no sink. C entry cln_fa2_decode_paged_multi_window_sink_anyg_bf16
    (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_decode_paged_multi_window_sink_anyg_bf16", torch.bfloat16, 4, fa2_decode_paged_multi_window_sink_anyg_bf16_plan, q,
                     k_pages, v_pages, block_table, seqlens, None, None, None, out, lse, workspace, _NO_WINDOW if window is None else window, sinks,
                     True)


def fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, window, sinks, out,
                                                       lse=None):
    """fa2_prefill_paged_varlen_window_sink_bf16_fp8 for any group size Hq / Hkv in 1 … 16: pools, scales, numerics, window = None, sinks = None
    and errors as there, and for Hq / Hkv in {1, 2, 4, 8} its bits. C entry cln_fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8
    (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8", torch.bfloat16, 3, None, q, k_pages, v_pages, block_table, seqlens,
                     cu_q, k_scale, v_scale, out, lse, None, _NO_WINDOW if window is None else window, sinks, True)


def fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_anyg_bf16_fp8: what
    fa2_decode_paged_multi_window_sink_anyg_bf16_plan returns for the same numbers
    (cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan, include/cln_amd_ext.h). No GPU needed."""
    return _paged_plan("fa2_decode_paged_multi_window_sink_anyg_bf16_fp8", B, T, Hq, Hkv, max_pages, page, D,
                       window=_NO_WINDOW if window is None else window)


def fa2_decode_paged_multi_window_sink_anyg_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, window, sinks, out, lse=None,
                                                     workspace=None):
    """fa2_decode_paged_multi_window_sink_bf16_fp8 for any group size Hq / Hkv in 1 … 16: T in 1 … 8 with T * Hq / Hkv <= 64,
    fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan(...)[2] workspace bytes; everything else as there, and for Hq / Hkv in {1, 2, 4, 8}
    its bits. C entry cln_fa2_decode_paged_multi_window_sink_anyg_bf16_fp8 (include/cln_amd_ext.h); no CPU path."""
    _paged_attention("fa2_decode_paged_multi_window_sink_anyg_bf16_fp8", torch.bfloat16, 4, fa2_decode_paged_multi_window_sink_anyg_bf16_fp8_plan,
                     q, k_pages, v_pages, block_table, seqlens, None, k_scale, v_scale, out, lse, workspace,
                     _NO_WINDOW if window is None else window, sinks, True)


def _paged_softcap(name, softmax_scale, softcap):
    """The two floats of a *_softcap_* entry: None is the C entry's 0 -- softmax_scale: 1 / sqrt(D), softcap: no cap; a 0 given as
    a number means the same -- and any other value is finite and > 0."""
    out = []
    for what, v in (("softmax_scale", softmax_scale), ("softcap", softcap)):
        if v is None:
            out.append(0.0)
            continue
        v = float(v)
        if not (0.0 <= v < math.inf):
            raise RuntimeError("%s: %s %r not supported (finite and > 0, or None)" % (name, what, v))
        out.append(v)
    return tuple(out)


def fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, sinks, softmax_scale, softcap,
                                                           out, lse=None):
    """fa2_prefill_paged_varlen_window_sink_anyg_bf16 with a softmax scale and logit soft-capping: the score of a key is u = q.k * softmax_scale
    (None: 1 / sqrt(D)) and, with softcap = c, c * tanh(u / c) (None: no cap), capped before the window and causal mask; the sink is neither
    scaled nor capped. Both None: the bits of fa2_prefill_paged_varlen_window_sink_anyg_bf16. Everything else as there. C entry
    cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16 (include/cln_amd_ext.h); no CPU path."""
    name = "fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16"
    _paged_attention(name, torch.bfloat16, 3, None, q, k_pages, v_pages, block_table, seqlens, cu_q, None, None, out, lse, None,
                     _NO_WINDOW if window is None else window, sinks, True, _paged_softcap(name, softmax_scale, softcap))


def fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_softcap_anyg_bf16: what
    fa2_decode_paged_multi_window_sink_anyg_bf16_plan returns for the same numbers -- neither the scale nor the cap changes the splits or the
    workspace (cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan, include/cln_amd_ext.h). No GPU needed."""
    return _paged_plan("fa2_decode_paged_multi_window_sink_softcap_anyg_bf16", B, T, Hq, Hkv, max_pages, page, D,
                       window=_NO_WINDOW if window is None else window)


def fa2_decode_paged_multi_window_sink_softcap_anyg_bf16(q, k_pages, v_pages, block_table, seqlens, window, sinks, softmax_scale, softcap, out,
                                                         lse=None, workspace=None):
    """fa2_decode_paged_multi_window_sink_anyg_bf16 with a softmax scale and logit soft-capping (softmax_scale, softcap as for
    fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16; both None: the bits of fa2_decode_paged_multi_window_sink_anyg_bf16);
    fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan(...)[2] workspace bytes. C entry
    cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16 (include/cln_amd_ext.h); no CPU path."""
    name = "fa2_decode_paged_multi_window_sink_softcap_anyg_bf16"
    _paged_attention(name, torch.bfloat16, 4, fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_plan, q, k_pages, v_pages, block_table, seqlens,
                     None, None, None, out, lse, workspace, _NO_WINDOW if window is None else window, sinks, True,
                     _paged_softcap(name, softmax_scale, softcap))


def fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, window, sinks,
                                                               softmax_scale, softcap, out, lse=None):
    """fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8 with a softmax scale and logit soft-capping (softmax_scale, softcap as for
    fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16); k_scale is part of the dequantised score and stands inside the tanh. C entry
    cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8 (include/cln_amd_ext.h); no CPU path."""
    name = "fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8"
    _paged_attention(name, torch.bfloat16, 3, None, q, k_pages, v_pages, block_table, seqlens, cu_q, k_scale, v_scale, out, lse, None,
                     _NO_WINDOW if window is None else window, sinks, True, _paged_softcap(name, softmax_scale, softcap))


def fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8: what
    fa2_decode_paged_multi_window_sink_anyg_bf16_plan returns for the same numbers
    (cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan, include/cln_amd_ext.h). No GPU needed."""
    return _paged_plan("fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8", B, T, Hq, Hkv, max_pages, page, D,
                       window=_NO_WINDOW if window is None else window)


def fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8(q, k_pages, v_pages, block_table, seqlens, k_scale, v_scale, window, sinks,
                                                             softmax_scale, softcap, out, lse=None, workspace=None):
    """fa2_decode_paged_multi_window_sink_anyg_bf16_fp8 with a softmax scale and logit soft-capping (softmax_scale, softcap as for
    fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16; k_scale inside the tanh);
    fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan(...)[2] workspace bytes. C entry
    cln_fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8 (include/cln_amd_ext.h); no CPU path."""
    name = "fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8"
    _paged_attention(name, torch.bfloat16, 4, fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8_plan, q, k_pages, v_pages, block_table,
                     seqlens, None, k_scale, v_scale, out, lse, workspace, _NO_WINDOW if window is None else window, sinks, True,
                     _paged_softcap(name, softmax_scale, softcap))


def kv_append_paged_varlen_d256_bf16(k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, q=None, q_out=None, rope_table=None, rope="none"):
    """kv_append_paged_varlen_bf16 at head dim 256: k_new, v_new torch.bfloat16 [total_q,Hkv,256], q, q_out [total_q,Hq,256], the
    pools [P,Hkv,page,256], rope_table fp32 [max_pos,256]; rope "half" rotates the pairs (i, i + 128). Everything else -- liveness, the caller's
    contract, the errors -- as there; any other head dim is refused. Deterministic. C entry cln_kv_append_paged_varlen_d256_bf16
    (include/cln_amd_ext.h); no CPU path."""
    _kv_append_paged("kv_append_paged_varlen_d256_bf16", torch.bfloat16, k_new, v_new, k_pages, v_pages, block_table, seqlens, cu_q, None, None, q,
                     q_out, rope_table, rope, head_dims=(256,))


def fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16(q, k_pages, v_pages, block_table, seqlens, cu_q, window, sinks, softmax_scale,
                                                                softcap, out, lse=None):
    """fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16 at head dim 256: q, out torch.bfloat16 [total_q,Hq,256], the pools
    [P,Hkv,page,256]; window, sinks, softmax_scale (None: 1 / 16) and softcap as there, each None-able; any other head dim is refused. C entry
    cln_fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16 (include/cln_amd_ext.h); no CPU path."""
    name = "fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16"
    _paged_attention(name, torch.bfloat16, 3, None, q, k_pages, v_pages, block_table, seqlens, cu_q, None, None, out, lse, None,
                     _NO_WINDOW if window is None else window, sinks, True, _paged_softcap(name, softmax_scale, softcap), head_dims=(256,))


def fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan(B, T, Hq, Hkv, max_pages, page, D, window):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16: the entry's own plan -- fa2d::split_plan on
    the span of the window in units of max(page, 64), the 64-key step of its kernel, and D = 256; T in 1 … 8 with T * Hq / Hkv <= 32;
    window = None: no window (2**31 - 1) (cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan, include/cln_amd_ext.h). No GPU
    needed."""
    return _paged_plan("fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16", B, T, Hq, Hkv, max_pages, page, D,
                       window=_NO_WINDOW if window is None else window, head_dims=(256,), max_rows=32)


def fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16(q, k_pages, v_pages, block_table, seqlens, window, sinks, softmax_scale, softcap,
                                                              out, lse=None, workspace=None):
    """fa2_decode_paged_multi_window_sink_softcap_anyg_bf16 at head dim 256: q, out torch.bfloat16 [B,T,Hq,256], T in 1 … 8 with
    T * Hq / Hkv <= 32; fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan(...)[2] workspace bytes; everything else as there. C entry
    cln_fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16 (include/cln_amd_ext.h); no CPU path."""
    name = "fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16"
    _paged_attention(name, torch.bfloat16, 4, fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16_plan, q, k_pages, v_pages, block_table,
                     seqlens, None, None, None, out, lse, workspace, _NO_WINDOW if window is None else window, sinks, True,
                     _paged_softcap(name, softmax_scale, softcap), head_dims=(256,))


# ---- multi-head latent attention over a paged latent cache: one pool bf16 [P,page,576] of rows [c 512 | k_pe 64]
_MLA_DC, _MLA_DR, _MLA_DK, _MLA_MAX_HQ = 512, 64, 576, 128


def _softmax_scale(name, softmax_scale):
    """The float of the softmax scale of the MLA entries, which has no default."""
    scale = float(softmax_scale)
    if not (0.0 < scale < math.inf):
        raise RuntimeError("%s: softmax_scale %r not supported (finite and > 0; there is no default)" % (name, softmax_scale))
    return scale


def _mla_fp8_check(name, pool, kv_scale):
    """What the MLA FP8 entries ask of the pool and its scale: a torch.float8_e4m3fn pool of three dims and an fp32 [1] scale on the GPU."""
    _check_dtype(pool, torch.float8_e4m3fn)
    _check_dtype(kv_scale, torch.float32)
    _check_dev(pool, kv_scale)
    _check_shape(kv_scale, 1)
    if pool.dim() != 3:
        raise RuntimeError("Tensor size mismatch!")


def _mla_plan(name, dims, max_t, too_large):
    """The body of the MLA *_plan wrappers: the C entry cln_<name>_plan for dims = (B, T, Hq, …, max_pages, page) and its error texts. max_t
    (the T the entry takes at most, None for no cap) and too_large (what its last -2 says) are the entry's: they choose the text of a -2,
    never the status."""
    dims = tuple(map(int, dims))
    rc, plan = _decode_plan("cln_%s_plan" % name, dims)
    if rc == -2:
        T, Hq, page = dims[1], dims[2], dims[-1]
        if max_t is not None and T > max_t:
            raise RuntimeError("%s: T %d not supported (1 … %d)" % (name, T, max_t))
        if Hq > _MLA_MAX_HQ:
            raise RuntimeError("%s: %d query heads not supported (1 … %d)" % (name, Hq, _MLA_MAX_HQ))
        if page not in _PAGED_PAGES:
            raise _paged_page_error(name, page)
        raise RuntimeError(too_large % name)
    _raise(name, rc)
    return plan


def _mla_decode(name, plan, q, pool, block_table, seqlens, kv_scale, indices, softmax_scale, out, lse, workspace):
    """The body of every MLA decode entry over the paged latent cache. q: bf16 [B,T,Hq,576], out: bf16 [B,T,Hq,512]; the pool holds bf16, or
    for a *_fp8 entry e4m3 with kv_scale: one more input pointer behind seqlens; indices = the int32 [B,T,topk] of a *_sparse_* entry: one
    more input pointer there and topk behind Hq, for the entry and its plan. plan = the entry's *_plan. What an entry takes is read from its
    name, not from an argument being None: a forgotten tensor must not select another C prototype."""
    fp8, sparse = name.endswith("_fp8"), "_sparse_" in name
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * (7 + fp8 + sparse) + [ctypes.c_longlong] + [ctypes.c_int] * (6 + sparse)
                 + [ctypes.c_float, ctypes.c_void_p])
    scale = _softmax_scale(name, softmax_scale)
    _decode_check((q, out) if fp8 else (q, pool, out), (block_table, seqlens, indices) if sparse else (block_table, seqlens), torch.bfloat16)
    if fp8:
        _mla_fp8_check(name, pool, kv_scale)
    if q.dim() != 4 or pool.dim() != 3 or block_table.dim() != 2 or (sparse and indices.dim() != 3):
        raise RuntimeError("Tensor size mismatch!")
    B, T, Hq, Dk = q.shape
    P, page, _ = pool.shape
    if Dk != _MLA_DK:
        raise RuntimeError("%s: q of %d dims not supported (%d = 512 latent + 64 rotary)" % (name, Dk, _MLA_DK))
    _check_shape(pool, P, page, _MLA_DK)
    if block_table.shape[0] != B:
        raise RuntimeError("Tensor size mismatch!")
    max_pages = block_table.shape[1]
    _check_shape(out, B, T, Hq, _MLA_DC)
    _check_shape(seqlens, B)
    topk = ()
    if sparse:
        topk = (indices.shape[2],)
        _check_shape(indices, B, T, *topk)
        if not indices.is_contiguous():
            raise RuntimeError("%s: indices must be contiguous [B,T,topk]" % name)
    lse_ptr = _decode_lse(lse, B, T, Hq)
    ws_ptr, ws_bytes = _decode_workspace(name, plan(B, T, Hq, *topk, max_pages, page)[2], workspace, q.device)
    more = ((kv_scale.data_ptr(),) if fp8 else ()) + ((indices.data_ptr(),) if sparse else ())
    rc = fn(q.data_ptr(), pool.data_ptr(), block_table.data_ptr(), seqlens.data_ptr(), *more, out.data_ptr(), lse_ptr, ws_ptr, ws_bytes, B, T,
            Hq, *topk, P, max_pages, page, scale, _stream())
    _raise(name, rc)


def _mla_append(name, c_new, k_pe_new, pool, block_table, seqlens, cu_q, kv_scale, q, q_out, rope_table, rope):
    """The body of the two appends to the paged latent cache. c_new: bf16 [total_q,512], k_pe_new: bf16 [total_q,64], q, q_out: bf16
    [total_q,Hq,576]; the pool holds bf16, or for the *_fp8 entry e4m3 with kv_scale: one more input pointer behind cu_q. Unlike the GQA
    appends, rope "none" takes q and q_out."""
    fp8 = name.endswith("_fp8")
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * (9 + fp8) + [ctypes.c_int] * 8 + [ctypes.c_void_p])
    if rope not in _ROPE_MODES:
        raise RuntimeError("%s: rope %r not supported ('none', 'half' or 'interleaved')" % (name, rope))
    mode = _ROPE_MODES[rope]
    if mode == 0 and rope_table is not None:
        raise RuntimeError("%s: rope 'none' takes no rope_table" % name)
    if mode != 0 and rope_table is None:
        raise RuntimeError("%s: rope %r needs a rope_table (kv_append_rope_table(max_pos, 64))" % (name, rope))
    if (q is None) != (q_out is None):
        raise RuntimeError("%s: q and q_out are given together or not at all" % name)
    rows = (c_new, k_pe_new) if fp8 else (c_new, k_pe_new, pool)
    _decode_check(rows + (q, q_out) if q is not None else rows, (block_table, seqlens, cu_q), torch.bfloat16)
    if fp8:
        _mla_fp8_check(name, pool, kv_scale)
    if c_new.dim() != 2 or k_pe_new.dim() != 2 or pool.dim() != 3 or block_table.dim() != 2:
        raise RuntimeError("Tensor size mismatch!")
    total_q = c_new.shape[0]
    P, page, _ = pool.shape
    B, max_pages = block_table.shape
    _check_shape(c_new, total_q, _MLA_DC)
    _check_shape(k_pe_new, total_q, _MLA_DR)
    _check_shape(pool, P, page, _MLA_DK)
    _check_shape(seqlens, B)
    _check_shape(cu_q, B + 1)
    Hq = 1
    if q is not None:
        if q.dim() != 3:
            raise RuntimeError("Tensor size mismatch!")
        Hq = q.shape[1]
        _check_shape(q, total_q, Hq, _MLA_DK)
        _check_shape(q_out, total_q, Hq, _MLA_DK)
    max_pos = _rope_table_max_pos(rope_table, _MLA_DR)
    if page not in _PAGED_PAGES:
        raise _paged_page_error(name, page)
    rc = fn(c_new.data_ptr(), k_pe_new.data_ptr(), pool.data_ptr(), block_table.data_ptr(), seqlens.data_ptr(), cu_q.data_ptr(),
            *((kv_scale.data_ptr(),) if fp8 else ()), None if q is None else q.data_ptr(), None if q is None else q_out.data_ptr(),
            None if rope_table is None else rope_table.data_ptr(), B, total_q, Hq, P, max_pages, page, max_pos, mode, _stream())
    _raise(name, rc, "%s: max_pages * page or total_q too large for one launch" % name)


def _mla_gather(name, pool, block_table, cu_k, kv_scale, out, starts):
    """The body of the two gathers out of the paged latent cache into out: bf16 [total_k,576]; the pool holds bf16, or for the *_fp8 entry e4m3 with
    kv_scale: one more input pointer behind cu_k."""
    fp8 = name.endswith("_fp8")
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * (5 + fp8) + [ctypes.c_int] * 5 + [ctypes.c_void_p])
    _decode_check((out,) if fp8 else (pool, out), (block_table, cu_k) + (() if starts is None else (starts,)), torch.bfloat16)
    if fp8:
        _mla_fp8_check(name, pool, kv_scale)
    if pool.dim() != 3 or block_table.dim() != 2 or out.dim() != 2:
        raise RuntimeError("Tensor size mismatch!")
    P, page, _ = pool.shape
    B, max_pages = block_table.shape
    total_k = out.shape[0]
    _check_shape(pool, P, page, _MLA_DK)
    _check_shape(out, total_k, _MLA_DK)
    _check_shape(cu_k, B + 1)
    if starts is not None:
        _check_shape(starts, B)
    if page not in _PAGED_PAGES:
        raise _paged_page_error(name, page)
    rc = fn(pool.data_ptr(), block_table.data_ptr(), None if starts is None else starts.data_ptr(), cu_k.data_ptr(),
            *((kv_scale.data_ptr(),) if fp8 else ()), out.data_ptr(), B, total_k, P, max_pages, page, _stream())
    _raise(name, rc, "%s: max_pages * page or total_k too large for one launch" % name)


_MLA_DECODE_TOO_LARGE ="%s: max_pages * page or B * ceil(T * Hq / 64) * splits too large for one launch"


def fa2_decode_paged_mla_bf16_plan(B, T, Hq, max_pages, page):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_mla_bf16: fa2d::split_plan on B * ceil(T * Hq / 64) workgroup jobs (a row group of
    64 query rows each), in units of max(page, 64) keys, at D = 512; a function of these five numbers only (cln_fa2_decode_paged_mla_bf16_plan,
    include/cln_amd_ext.h). T in 1 … 8, Hq in 1 … 128. No GPU needed."""
    return _mla_plan("fa2_decode_paged_mla_bf16", (B, T, Hq, max_pages, page), 8, _MLA_DECODE_TOO_LARGE)


def fa2_decode_paged_mla_bf16(q, pool, block_table, seqlens, softmax_scale, out, lse=None, workspace=None):
    """Multi-head latent attention decode over a paged latent cache into out: q torch.bfloat16 [B,T,Hq,576], already absorbed by the model
    (q_nope W_UK in dims 0 … 511, q_pe in 512 … 575); pool torch.bfloat16 [P,page,576], a row [c 512 | k_pe 64] stored once and shared by all
    query heads: the key is the whole row, the value its dims 0 … 511; block_table int32 [B,max_pages] and seqlens int32 [B] on the GPU (never
    read by the host; lengths clamped to [0, max_pages * page] by the kernels; the live table entries must lie in [0, P)); out torch.bfloat16
    [B,T,Hq,512] in latent space; lse fp32 [B,T,Hq] (natural log) or None. seqlens[b] counts the T newest tokens; query t sees the keys
    j < len_b - (T - 1 - t), and a query that sees none gets O = 0 and LSE = -inf. softmax_scale: required, finite and > 0 (the models use
    192 ** -0.5 * mscale ** 2, not 576 ** -0.5). T in 1 … 8, Hq in 1 … 128, page in {16, 32, 64, 128, 256}. workspace: any contiguous GPU tensor
    of at least fa2_decode_paged_mla_bf16_plan(...)[2] bytes; allocated here on the current stream when None and the plan splits the keys.
    Deterministic. C entry cln_fa2_decode_paged_mla_bf16 (include/cln_amd_ext.h); no CPU path."""
    _mla_decode("fa2_decode_paged_mla_bf16", fa2_decode_paged_mla_bf16_plan, q, pool, block_table, seqlens, None, None, softmax_scale, out, lse,
                workspace)


def kv_append_paged_mla_bf16(c_new, k_pe_new, pool, block_table, seqlens, cu_q, q=None, q_out=None, rope_table=None, rope="none"):
    """Write the latent rows of a packed batch of new tokens into the paged latent cache of fa2_decode_paged_mla_bf16, with the rotary embedding
    of k_pe and q_pe fused in; one launch. c_new torch.bfloat16 [total_q,512] goes to pool dims 0 … 511 bit for bit, k_pe_new torch.bfloat16
    [total_q,64] to dims 512 … 575, rotated; pool torch.bfloat16 [P,page,576], written in place; q, q_out torch.bfloat16 [total_q,Hq,576], given
    together or both None (q_out may be q): dims 0 … 511 copied bit for bit, dims 512 … 575 rotated at the same position. cu_q int32 [B+1],
    block_table int32 [B,max_pages], seqlens int32 [B] on the GPU (never read by the host), as for kv_append_paged_varlen_bf16: token i of
    sequence b is packed row cu_q[b] + i and stands at pos = seqlens[b] - T_b + i; liveness and the caller's contract as there; packed rows
    outside [cu_q[0], cu_q[B]) are neither read nor written. rope: "none" (the rotary dims are copied; no rope_table), "half" (pairs
    (i, i + 32)) or "interleaved" (pairs (2i, 2i + 1)), rotated in fp32 by rope_table fp32 [max_pos,64] (kv_append_rope_table(max_pos, 64)) with
    one rounding. Deterministic. C entry cln_kv_append_paged_mla_bf16 (include/cln_amd_ext.h); no CPU path."""
    _mla_append("kv_append_paged_mla_bf16", c_new, k_pe_new, pool, block_table, seqlens, cu_q, None, q, q_out, rope_table, rope)


# ---- the prompt path of multi-head latent attention: un-absorbed prefill (key 192 = 128 + 64 dims, value 128), the merge of
# two attention states, the gather out of the latent pool
_MLA_DN, _MLA_DQ, _MLA_DV = 128, 192, 128
_MERGE_MAX_D = 512


def fa2_prefill_varlen_mla_bf16(q, kv, k_pe, cu_q, cu_k, softmax_scale, out, lse=None, causal=True):
    """Multi-head latent attention prefill (un-absorbed) of a packed batch into out: q torch.bfloat16 [total_q,Hq,192] = [q_nope 128 | q_pe 64],
    already rotated (kv_append_paged_mla_bf16 can rotate q along the way); kv torch.bfloat16 [total_k,Hq,256] = [k_nope 128 | v 128] per head,
    what kv_b_proj writes; k_pe torch.bfloat16 [total_k,64], rotated, one row per token shared by every head; cu_q, cu_k int32 [B+1] on the GPU
    (never read by the host, every offset clamped): sequence b has T_b = cu_q[b+1] - cu_q[b] queries and L_b = cu_k[b+1] - cu_k[b] keys; out
    torch.bfloat16 [total_q,Hq,128]; lse fp32 [total_q,Hq] (natural log) or None. causal=True: query t sees the keys j < L_b - (T_b - 1 - t);
    causal=False: all L_b keys (a context chunk of a chunked prefill). A query that sees no key gets O = 0 and LSE = -inf. softmax_scale:
    required, finite and > 0. Hq in 1 … 128. Packed rows outside [cu_q[0], cu_q[B]) are neither read nor written. Deterministic. C entry
    cln_fa2_prefill_varlen_mla_bf16 (include/cln_amd_ext.h); no CPU path."""
    name = "fa2_prefill_varlen_mla_bf16"
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * 7 + [ctypes.c_int] * 5 + [ctypes.c_float, ctypes.c_void_p])
    scale = _softmax_scale(name, softmax_scale)
    _decode_check((q, kv, k_pe, out), (cu_q, cu_k), torch.bfloat16)
    if q.dim() != 3 or kv.dim() != 3 or k_pe.dim() != 2 or cu_q.dim() != 1:
        raise RuntimeError("Tensor size mismatch!")
    total_q, Hq, Dq = q.shape
    total_k = kv.shape[0]
    B = cu_q.shape[0] - 1
    if Dq != _MLA_DQ:
        raise RuntimeError("%s: q of %d dims not supported (%d = 128 nope + 64 rotary)" % (name, Dq, _MLA_DQ))
    if B < 1 or total_q < 1 or total_k < 1:
        raise RuntimeError("Tensor size mismatch!")
    _check_shape(kv, total_k, Hq, _MLA_DN + _MLA_DV)
    _check_shape(k_pe, total_k, _MLA_DR)
    _check_shape(cu_k, B + 1)
    _check_shape(out, total_q, Hq, _MLA_DV)
    if Hq > _MLA_MAX_HQ:
        raise RuntimeError("%s: %d query heads not supported (1 … %d)" % (name, Hq, _MLA_MAX_HQ))
    lse_ptr = _decode_lse(lse, total_q, Hq)
    rc = fn(q.data_ptr(), kv.data_ptr(), k_pe.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), out.data_ptr(), lse_ptr, B, total_q, total_k, Hq,
            1 if causal else 0, scale, _stream())
    _raise(name, rc, "%s: total_q too large for one launch" % name)


def attn_merge_states_bf16(o_a, lse_a, o_b, lse_b, out, lse=None):
    """Merge two attention states over disjoint key sets into out: o_a, o_b torch.bfloat16 [..., D] of one shape, lse_a, lse_b fp32 of the
    leading shape (natural log), out torch.bfloat16 of o_a's shape (may be o_a), lse fp32 of lse_a's shape or None (may be lse_a). D % 8 == 0,
    8 <= D <= 512. Per row in fp32: m = max(lse_a, lse_b); both -inf: O = 0, LSE = -inf; else w = exp(lse - m), a side whose LSE is -inf is
    selected out (its O may hold anything), O = (w_a O_a + w_b O_b) / (w_a + w_b) rounded once, LSE = m + ln(w_a + w_b). Deterministic. C entry
    cln_attn_merge_states_bf16 (include/cln_amd_ext.h); no CPU path."""
    name = "attn_merge_states_bf16"
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * 6 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p])
    for t in (o_a, o_b, out):
        _check_dtype(t, torch.bfloat16)
    for t in (lse_a, lse_b):
        _check_dtype(t, torch.float32)
    _check_dev(o_a, o_b, out, lse_a, lse_b)
    if o_a.dim() < 2:
        raise RuntimeError("Tensor size mismatch!")
    D = o_a.shape[-1]
    lead = tuple(o_a.shape[:-1])
    _check_shape(o_b, *o_a.shape)
    _check_shape(out, *o_a.shape)
    _check_shape(lse_a, *lead)
    _check_shape(lse_b, *lead)
    if D % 8 != 0 or not 8 <= D <= _MERGE_MAX_D:
        raise RuntimeError("%s: D %d not supported (a multiple of 8 in 8 … %d)" % (name, D, _MERGE_MAX_D))
    rows = lse_a.numel()
    if rows < 1:
        raise RuntimeError("Tensor size mismatch!")
    lse_ptr = _decode_lse(lse, *lead)
    rc = fn(o_a.data_ptr(), lse_a.data_ptr(), o_b.data_ptr(), lse_b.data_ptr(), out.data_ptr(), lse_ptr, rows, D, _stream())
    _raise(name, rc, "%s: too many rows for one launch" % name)


def kv_gather_paged_mla_bf16(pool, block_table, cu_k, out, starts=None):
    """Gather latent rows out of the paged latent cache of fa2_decode_paged_mla_bf16 into a packed batch: pool torch.bfloat16 [P,page,576],
    block_table int32 [B,max_pages], cu_k int32 [B+1], starts int32 [B] or None (0), all on the GPU and never read by the host; out
    torch.bfloat16 [total_k,576]. Packed row cu_k[b] + i receives cache row starts[b] + i of sequence b for i < cu_k[b+1] - cu_k[b], bit for
    bit; a cache row at or past max_pages * page is written as zeros and its table entry never followed; rows of no sequence are untouched. The
    mirror of kv_append_paged_mla_bf16. Deterministic. C entry cln_kv_gather_paged_mla_bf16 (include/cln_amd_ext.h); no CPU path."""
    _mla_gather("kv_gather_paged_mla_bf16", pool, block_table, cu_k, None, out, starts)


# ---- multi-head latent attention over a paged latent cache held in FP8: one pool torch.float8_e4m3fn [P,page,576] of rows
# [c 512 | k_pe 64] in codes and one scale fp32 [1] on the GPU for the whole pool; everything else is bf16 as above
def fa2_decode_paged_mla_bf16_fp8_plan(B, T, Hq, max_pages, page):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_mla_bf16_fp8: exactly fa2_decode_paged_mla_bf16_plan's, the key step is still 64 and
    D still 512 (cln_fa2_decode_paged_mla_bf16_fp8_plan, include/cln_amd_ext.h). T in 1 … 8, Hq in 1 … 128. No GPU needed."""
    return _mla_plan("fa2_decode_paged_mla_bf16_fp8", (B, T, Hq, max_pages, page), 8, _MLA_DECODE_TOO_LARGE)


def fa2_decode_paged_mla_bf16_fp8(q, pool, block_table, seqlens, kv_scale, softmax_scale, out, lse=None, workspace=None):
    """fa2_decode_paged_mla_bf16 over a latent cache held in FP8: q torch.bfloat16 [B,T,Hq,576], absorbed; pool torch.float8_e4m3fn [P,page,576]
    of rows [c 512 | k_pe 64] in codes; kv_scale fp32 [1] on the GPU, one scale for the whole pool: a stored byte c means e4m3(c) * kv_scale
    (finite and > 0, no NaN byte in a live row: the caller's contract, not checked); block_table, seqlens, out torch.bfloat16 [B,T,Hq,512], lse,
    softmax_scale (required, finite and > 0), the mask, T in 1 … 8, Hq in 1 … 128 and the pages as there. The codes are converted to bf16
    exactly on the way to LDS; the fp32 score multiplier is (softmax_scale * log2(e)) * kv_scale and kv_scale multiplies the fp32 result in front
    of its store. workspace: at least fa2_decode_paged_mla_bf16_fp8_plan(...)[2] bytes; allocated here when None and the plan splits the keys.
    Deterministic. C entry cln_fa2_decode_paged_mla_bf16_fp8 (include/cln_amd_ext.h); no CPU path."""
    _mla_decode("fa2_decode_paged_mla_bf16_fp8", fa2_decode_paged_mla_bf16_fp8_plan, q, pool, block_table, seqlens, kv_scale, None, softmax_scale,
                out, lse, workspace)


def kv_append_paged_mla_bf16_fp8(c_new, k_pe_new, pool, block_table, seqlens, cu_q, kv_scale, q=None, q_out=None, rope_table=None, rope="none"):
    """kv_append_paged_mla_bf16 into a latent cache held in FP8; one launch. c_new torch.bfloat16 [total_q,512], k_pe_new torch.bfloat16
    [total_q,64]; pool torch.float8_e4m3fn [P,page,576], written in place; kv_scale fp32 [1] on the GPU. Per element of a live pool row the byte
    is e4m3(clamp(y * (1 / kv_scale), ±448)) in fp32, round to nearest even, y the bf16 input or the fp32 rotation result with no bf16 rounding
    in between. q, q_out torch.bfloat16 [total_q,Hq,576] (q_out may be q), cu_q, block_table, seqlens, rope_table, the three rope modes, liveness
    and the untouched rows of no sequence as there. Deterministic. C entry cln_kv_append_paged_mla_bf16_fp8 (include/cln_amd_ext.h); no CPU
    path."""
    _mla_append("kv_append_paged_mla_bf16_fp8", c_new, k_pe_new, pool, block_table, seqlens, cu_q, kv_scale, q, q_out, rope_table, rope)


def kv_gather_paged_mla_bf16_fp8(pool, block_table, cu_k, kv_scale, out, starts=None):
    """kv_gather_paged_mla_bf16 out of a latent cache held in FP8: pool torch.float8_e4m3fn [P,page,576], kv_scale fp32 [1] on the GPU, out
    torch.bfloat16 [total_k,576]; each element is bf16(fp32(code) * kv_scale), one rounding. block_table, cu_k, starts, the zeros for a cache row
    at or past max_pages * page and the untouched rows of no sequence as there: the context-chunk loop of the prompt path runs unchanged over an
    FP8 pool. Deterministic. C entry cln_kv_gather_paged_mla_bf16_fp8 (include/cln_amd_ext.h); no CPU path."""
    _mla_gather("kv_gather_paged_mla_bf16_fp8", pool, block_table, cu_k, kv_scale, out, starts)


# ---- sparse multi-head latent attention over the paged latent cache: DeepSeek-V3.2's attention behind its indexer. The pool,
# the table, the lengths and the absorbed q are fa2_decode_paged_mla_bf16's; every query token brings its own list of cache positions
def fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, topk, max_pages, page):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_mla_sparse_bf16: a function of the shape only; the splits divide the topk index slots
    of a query token, not the context (cln_fa2_decode_paged_mla_sparse_bf16_plan, include/cln_amd_ext.h). T >= 1 (no cap: a query token is its
    own workgroup job), Hq in 1 … 128, topk >= 1. No GPU needed."""
    return _mla_plan("fa2_decode_paged_mla_sparse_bf16", (B, T, Hq, topk, max_pages, page), None,
                     "%s: max_pages * page, B * T * Hq or B * T * ceil(Hq / 64) * splits too large for one launch")


def fa2_decode_paged_mla_sparse_bf16(q, pool, block_table, seqlens, indices, softmax_scale, out, lse=None, workspace=None):
    """Sparse MLA decode (DeepSeek-V3.2, "DSA") over the paged latent cache; bf16. q torch.bfloat16 [B,T,Hq,576], absorbed; pool torch.bfloat16
    [P,page,576] of rows [c 512 | k_pe 64]; block_table int32 [B,max_pages]; seqlens int32 [B]; out torch.bfloat16 [B,T,Hq,512]; lse fp32 [B,T,Hq]
    or None: all as in fa2_decode_paged_mla_bf16. indices int32 [B,T,topk], contiguous, on the GPU, never read by the host: slot k of
    indices[b,t] is a LOGICAL token position of sequence b (the position space of seqlens), resolved through the block table, shared by all heads
    of that token. A slot is valid iff 0 <= idx < vis(b,t) = clamp(seqlens[b], 0, max_pages * page) - (T - 1 - t); every other value (-1, any
    negative, anything at or past vis) is an empty slot, anywhere in the list, and addresses nothing. Over the valid slots V of a token:
    s_k = softmax_scale * q . row(idx_k), O = softmax_V(s) row[:, 0:512], LSE = ln sum_V exp(s_k); V empty: O = 0, LSE = -inf. A position listed
    twice is two keys: pass distinct positions. softmax_scale required, finite and > 0; Hq in 1 … 128; any T >= 1 (also V3.2's sparse prefill
    over the paged cache); any topk >= 1. workspace: at least fa2_decode_paged_mla_sparse_bf16_plan(...)[2] bytes; allocated here when None and
    the plan splits the list. Deterministic. C entry cln_fa2_decode_paged_mla_sparse_bf16 (include/cln_amd_ext.h); no CPU path."""
    _mla_decode("fa2_decode_paged_mla_sparse_bf16", fa2_decode_paged_mla_sparse_bf16_plan, q, pool, block_table, seqlens, None, indices,
                softmax_scale, out, lse, workspace)


# ---- the same over the latent cache held in FP8: the pool and its scale are fa2_decode_paged_mla_bf16_fp8's, the lists and every
# rule about them the entry's above
_MLA_SPARSE_TOO_LARGE = "%s: max_pages * page, B * T * Hq or B * T * ceil(Hq / 64) * splits too large for one launch"


def fa2_decode_paged_mla_sparse_bf16_fp8_plan(B, T, Hq, topk, max_pages, page):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_mla_sparse_bf16_fp8: exactly fa2_decode_paged_mla_sparse_bf16_plan's, the slot step is
    still 64 and D still 512 (cln_fa2_decode_paged_mla_sparse_bf16_fp8_plan, include/cln_amd_ext.h). T >= 1, Hq in 1 … 128, topk >= 1. No GPU
    needed."""
    return _mla_plan("fa2_decode_paged_mla_sparse_bf16_fp8", (B, T, Hq, topk, max_pages, page), None, _MLA_SPARSE_TOO_LARGE)


def fa2_decode_paged_mla_sparse_bf16_fp8(q, pool, block_table, seqlens, kv_scale, indices, softmax_scale, out, lse=None, workspace=None):
    """fa2_decode_paged_mla_sparse_bf16 over a latent cache held in FP8: the attention of a DeepSeek-V3.2 step on the pool
    kv_append_paged_mla_bf16_fp8 writes. q torch.bfloat16 [B,T,Hq,576], absorbed; pool torch.float8_e4m3fn [P,page,576] of rows
    [c 512 | k_pe 64] in codes; kv_scale fp32 [1] on the GPU, one scale for the whole pool: a stored byte c means e4m3(c) * kv_scale (finite and
    > 0, no NaN byte in a listed row: the caller's contract, not checked; an unlisted row is never read); indices int32 [B,T,topk], contiguous,
    on the GPU, with the validity rule 0 <= idx < vis(b,t), the empty slots anywhere, the duplicates (two keys) and the O = 0, LSE = -inf of a
    token without a valid slot exactly as there; block_table, seqlens, out torch.bfloat16 [B,T,Hq,512], lse, softmax_scale (required, finite
    and > 0), any T >= 1, Hq in 1 … 128, any topk >= 1 and the pages as there. The codes are converted to bf16 exactly on the way to LDS; the
    fp32 score multiplier is (softmax_scale * log2(e)) * kv_scale and kv_scale multiplies the fp32 result in front of its store. workspace: at
    least fa2_decode_paged_mla_sparse_bf16_fp8_plan(...)[2] bytes; allocated here when None and the plan splits the list. Deterministic. C entry
    cln_fa2_decode_paged_mla_sparse_bf16_fp8 (include/cln_amd_ext.h); no CPU path."""
    _mla_decode("fa2_decode_paged_mla_sparse_bf16_fp8", fa2_decode_paged_mla_sparse_bf16_fp8_plan, q, pool, block_table, seqlens, kv_scale,
                indices, softmax_scale, out, lse, workspace)


# ---- the indexer of DeepSeek-V3.2's sparse attention: a paged cache of index keys (128 dims a token) next to the latent cache,
# behind the same block table; the logits of every visible cache position for a query token; the exact top-k of a row of logits, the list
# fa2_decode_paged_mla_sparse_bf16 takes
_IDX_DIM, _IDX_MAX_HEADS = 128, 64


def kv_append_paged_index_bf16(k_idx_new, idx_pool, block_table, seqlens, cu_q):
    """Append the index keys of a packed batch of new tokens to the paged index-key cache; one launch. k_idx_new torch.bfloat16 [total_q,128];
    idx_pool torch.bfloat16 [P,page,128], written in place, bit for bit; block_table int32 [B,max_pages], seqlens int32 [B] (the lengths AFTER
    the append), cu_q int32 [B+1]: all as in kv_append_paged_mla_bf16 -- token i of sequence b is packed row cu_q[b] + i and goes to position
    seqlens[b] - T_b + i, a token that is not live writes nothing, rows of no sequence are untouched. There is no rope argument, on purpose:
    the model rotates the index key and then applies a Hadamard transform before it caches it, so a rotation fused into this copy would sit
    in the wrong place. Deterministic. C entry cln_kv_append_paged_index_bf16 (include/cln_amd_ext.h); no CPU path."""
    name = "kv_append_paged_index_bf16"
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * 5 + [ctypes.c_int] * 5 + [ctypes.c_void_p])
    _decode_check((k_idx_new, idx_pool), (block_table, seqlens, cu_q), torch.bfloat16)
    if k_idx_new.dim() != 2 or idx_pool.dim() != 3 or block_table.dim() != 2:
        raise RuntimeError("Tensor size mismatch!")
    total_q = k_idx_new.shape[0]
    P, page, _ = idx_pool.shape
    B, max_pages = block_table.shape
    _check_shape(k_idx_new, total_q, _IDX_DIM)
    _check_shape(idx_pool, P, page, _IDX_DIM)
    _check_shape(seqlens, B)
    _check_shape(cu_q, B + 1)
    if page not in _PAGED_PAGES:
        raise _paged_page_error(name, page)
    rc = fn(k_idx_new.data_ptr(), idx_pool.data_ptr(), block_table.data_ptr(), seqlens.data_ptr(), cu_q.data_ptr(), B, total_q, P, max_pages,
            page, _stream())
    _raise(name, rc, "%s: max_pages * page too large for one launch" % name)


def mla_index_logits_paged_bf16(q_idx, weights, idx_pool, block_table, seqlens, logits):
    """The logits of DeepSeek-V3.2's indexer over the paged index-key cache; one launch, no workspace. q_idx torch.bfloat16 [B,T,Hi,128];
    weights fp32 [B,T,Hi] (the caller folds Hi^-1/2, 128^-1/2 and anything else into them); idx_pool torch.bfloat16 [P,page,128];
    block_table int32 [B,max_pages]; seqlens int32 [B]; logits fp32 [B,T,ld], contiguous, ld >= 1 the caller's. Writes
    logits[b,t,j] = sum_h weights[b,t,h] * max(0, q_idx[b,t,h] . k_idx[j]) for 0 <= j < vis(b,t) = clamp(seqlens[b], 0, cap) - (T - 1 - t),
    cap = min(max_pages * page, ld), and nothing else: positions at or past vis keep their bytes, and neither their keys nor their table
    entries are read. Any T >= 1 (the prompt too), Hi in 1 … 64. fp32 accumulation on the matrix cores, the head sum in a fixed order:
    deterministic, and a sequence's bits do not depend on its neighbours. C entry cln_mla_index_logits_paged_bf16 (include/cln_amd_ext.h); no
    CPU path."""
    name = "mla_index_logits_paged_bf16"
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * 6 + [ctypes.c_int] * 3 + [ctypes.c_longlong] + [ctypes.c_int] * 3 + [ctypes.c_void_p])
    _decode_check((q_idx, idx_pool), (block_table, seqlens), torch.bfloat16)
    for t in (weights, logits):
        _check_dtype(t, torch.float32)
    _check_dev(weights, logits)
    if q_idx.dim() != 4 or idx_pool.dim() != 3 or block_table.dim() != 2 or logits.dim() != 3:
        raise RuntimeError("Tensor size mismatch!")
    B, T, Hi, D = q_idx.shape
    P, page, _ = idx_pool.shape
    ld = logits.shape[2]
    if D != _IDX_DIM:
        raise RuntimeError("%s: q_idx of %d dims not supported (%d)" % (name, D, _IDX_DIM))
    _check_shape(idx_pool, P, page, _IDX_DIM)
    if block_table.shape[0] != B:
        raise RuntimeError("Tensor size mismatch!")
    max_pages = block_table.shape[1]
    _check_shape(weights, B, T, Hi)
    _check_shape(seqlens, B)
    _check_shape(logits, B, T, ld)
    if Hi > _IDX_MAX_HEADS:
        raise RuntimeError("%s: %d index heads not supported (1 … %d)" % (name, Hi, _IDX_MAX_HEADS))
    if page not in _PAGED_PAGES:
        raise _paged_page_error(name, page)
    rc = fn(q_idx.data_ptr(), weights.data_ptr(), idx_pool.data_ptr(), block_table.data_ptr(), seqlens.data_ptr(), logits.data_ptr(), B, T, Hi,
            ld, P, max_pages, page, _stream())
    _raise(name, rc, "%s: max_pages * page, B * T or B * T * ceil(cap / 1024) too large for one launch" % name)


def mla_index_topk(logits, seqlens, topk, indices):
    """The exact top-k of DeepSeek-V3.2's indexer; one launch, no workspace. logits fp32 [B,T,ld], contiguous; seqlens int32 [B]; indices int32
    [B,T,topk], contiguous, every slot written on every call. With n = max(clamp(seqlens[b], 0, ld) - (T - 1 - t), 0): n <= topk gives the
    dense list [0, …, n - 1, -1, …]; otherwise the topk positions that come first under (logit descending, position ascending), written in
    ascending position order. Only logits[b,t,0 … n-1] is read. The order is fp32's numeric order with -0 as +0 and ±inf ordinary values; a
    NaN is ordered by its bit pattern; whatever the values, every index is -1 or a distinct position in [0, n). The list is what
    fa2_decode_paged_mla_sparse_bf16 takes. Deterministic. C entry cln_mla_index_topk (include/cln_amd_ext.h); no CPU path."""
    name = "mla_index_topk"
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p])
    _check_dtype(logits, torch.float32)
    for t in (seqlens, indices):
        _check_dtype(t, torch.int32)
    _check_dev(logits, seqlens, indices)
    if logits.dim() != 3 or indices.dim() != 3:
        raise RuntimeError("Tensor size mismatch!")
    B, T, ld = logits.shape
    topk = int(topk)
    _check_shape(seqlens, B)
    _check_shape(indices, B, T, topk)
    rc = fn(logits.data_ptr(), seqlens.data_ptr(), indices.data_ptr(), B, T, ld, topk, _stream())
    _raise(name, rc, "%s: ld, B * T or topk * B * T too large for one launch" % name)


# ---- the indexer's cache held in FP8 with one fp32 scale per token: the model's own format, 132 bytes a token. The pool is
# bytes [P,page,132]; inside a page the 128 * page code bytes come first and the page's fp32 scales behind them
_IDX_FP8_ROW = 132


def index_pool_fp8_views(idx_pool):
    """(codes, scales) of an FP8 index pool, torch.uint8 [P,page,132] contiguous and 16-byte aligned: codes torch.float8_e4m3fn [P,page,128]
    (token slot r of page p at byte 128 * r of the page) and scales torch.float32 [P,page] (at byte 128 * page + 4 * r), both views of the
    pool's own storage, no copy. A stored token means k_d = e4m3(code_d) * scale. Works on any device."""
    _check_dtype(idx_pool, torch.uint8)
    if idx_pool.dim() != 3 or idx_pool.shape[2] != _IDX_FP8_ROW or not idx_pool.is_contiguous() or idx_pool.data_ptr() % 16:
        raise RuntimeError("Tensor size mismatch!")
    P, page, _ = idx_pool.shape
    if page not in _PAGED_PAGES:
        raise _paged_page_error("index_pool_fp8_views", page)
    pages = idx_pool.view(P, page * _IDX_FP8_ROW)
    codes = pages[:, :page * _IDX_DIM].view(torch.float8_e4m3fn).view(P, page, _IDX_DIM)
    scales = pages[:, page * _IDX_DIM:].view(torch.float32)
    return codes, scales


def _index_pool_fp8(name, idx_pool):
    """(P, page) of an FP8 index pool, or the refusal: uint8, [P,page,132], a supported page."""
    _check_dtype(idx_pool, torch.uint8)
    if idx_pool.dim() != 3:
        raise RuntimeError("Tensor size mismatch!")
    P, page, _ = idx_pool.shape
    _check_shape(idx_pool, P, page, _IDX_FP8_ROW)
    return P, page


def kv_append_paged_index_bf16_fp8(k_idx_new, idx_pool, block_table, seqlens, cu_q, scale_pow2=False):
    """kv_append_paged_index_bf16 into an index-key cache held in FP8 with one fp32 scale per token; one launch. k_idx_new torch.bfloat16
    [total_q,128]; idx_pool torch.uint8 [P,page,132], contiguous, written in place (the layout: index_pool_fp8_views); block_table, seqlens
    (the lengths AFTER the append) and cu_q, the packed convention, liveness and the untouched rows of no sequence as there. Per live token,
    in IEEE fp32: a = max(amax |k|, 1e-4), scale = a / 448, with scale_pow2 rounded up to a power of two (ue8m0: the model's configuration),
    code = e4m3fn(clamp(k * (1 / scale), ±448)), round to nearest even; every pool byte that is not a live token's 128 codes or 4 scale bytes
    keeps its value. Inputs are finite: the caller's contract. Deterministic. C entry cln_kv_append_paged_index_bf16_fp8
    (include/cln_amd_ext.h); no CPU path."""
    name = "kv_append_paged_index_bf16_fp8"
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * 5 + [ctypes.c_int] * 6 + [ctypes.c_void_p])
    _decode_check((k_idx_new,), (block_table, seqlens, cu_q), torch.bfloat16)
    P, page = _index_pool_fp8(name, idx_pool)
    _check_dev(idx_pool)
    if k_idx_new.dim() != 2 or block_table.dim() != 2:
        raise RuntimeError("Tensor size mismatch!")
    total_q = k_idx_new.shape[0]
    B, max_pages = block_table.shape
    _check_shape(k_idx_new, total_q, _IDX_DIM)
    _check_shape(seqlens, B)
    _check_shape(cu_q, B + 1)
    if page not in _PAGED_PAGES:
        raise _paged_page_error(name, page)
    rc = fn(k_idx_new.data_ptr(), idx_pool.data_ptr(), block_table.data_ptr(), seqlens.data_ptr(), cu_q.data_ptr(), B, total_q, P, max_pages,
            page, 1 if scale_pow2 else 0, _stream())
    _raise(name, rc, "%s: max_pages * page too large for one launch" % name)


def mla_index_logits_paged_bf16_fp8(q_idx, weights, idx_pool, block_table, seqlens, logits):
    """mla_index_logits_paged_bf16 over an index-key cache held in FP8 with one fp32 scale per token; one launch, no workspace. q_idx
    torch.bfloat16 [B,T,Hi,128]; weights fp32 [B,T,Hi]; idx_pool torch.uint8 [P,page,132] (the layout: index_pool_fp8_views); block_table
    int32 [B,max_pages]; seqlens int32 [B]; logits fp32 [B,T,ld], contiguous. With c_j the codes of position j read as numbers and s_j its
    scale, writes logits[b,t,j] = s_j * sum_h weights[b,t,h] * max(0, q_idx[b,t,h] . c_j) for 0 <= j < vis(b,t) and nothing else; cap, vis and
    what is never read are the bf16 entry's. The scale multiplies once per key after the head sum, in fp32: the dequantise-then-ReLU form
    exactly for s_j >= 0 (s_j finite and >= 0 and no NaN code, 0x7F or 0xFF, in a visible row: the caller's contract, not checked; the append
    writes a scale > 0 and, for finite keys, no NaN code). Any T >= 1, Hi in 1 … 64. The codes become bf16
    exactly on the way into the matrix operand; fp32 accumulation, a fixed order: deterministic, and a sequence's bits do not depend on its
    neighbours. C entry cln_mla_index_logits_paged_bf16_fp8 (include/cln_amd_ext.h); no CPU path."""
    name = "mla_index_logits_paged_bf16_fp8"
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * 6 + [ctypes.c_int] * 3 + [ctypes.c_longlong] + [ctypes.c_int] * 3 + [ctypes.c_void_p])
    _decode_check((q_idx,), (block_table, seqlens), torch.bfloat16)
    for t in (weights, logits):
        _check_dtype(t, torch.float32)
    P, page = _index_pool_fp8(name, idx_pool)
    _check_dev(idx_pool, weights, logits)
    if q_idx.dim() != 4 or block_table.dim() != 2 or logits.dim() != 3:
        raise RuntimeError("Tensor size mismatch!")
    B, T, Hi, D = q_idx.shape
    ld = logits.shape[2]
    if D != _IDX_DIM:
        raise RuntimeError("%s: q_idx of %d dims not supported (%d)" % (name, D, _IDX_DIM))
    if block_table.shape[0] != B:
        raise RuntimeError("Tensor size mismatch!")
    max_pages = block_table.shape[1]
    _check_shape(weights, B, T, Hi)
    _check_shape(seqlens, B)
    _check_shape(logits, B, T, ld)
    if Hi > _IDX_MAX_HEADS:
        raise RuntimeError("%s: %d index heads not supported (1 … %d)" % (name, Hi, _IDX_MAX_HEADS))
    if page not in _PAGED_PAGES:
        raise _paged_page_error(name, page)
    rc = fn(q_idx.data_ptr(), weights.data_ptr(), idx_pool.data_ptr(), block_table.data_ptr(), seqlens.data_ptr(), logits.data_ptr(), B, T, Hi,
            ld, P, max_pages, page, _stream())
    _raise(name, rc, "%s: max_pages * page, B * T or B * T * ceil(cap / 1024) too large for one launch" % name)


# ---- the packed ("varlen") DSA step: the three calls behind the append for a packed batch -- [total_q, …] rows and the
# device-side offsets cu_q int32 [B+1] of kv_append_paged_index_bf16 / kv_append_paged_mla_bf16 -- so that one step of continuous batching
# (a prompt chunk next to single-token decode rows) is four calls, whatever the mix. Packed row r is token t = r - cu_q[b] of the sequence b
# with cu_q[b] <= r < cu_q[b+1]; T_b = cu_q[b+1] - cu_q[b] takes the place of T in vis; T_b = 0 is a sequence without a token this step. The
# offsets are clamped to [0, total_q] on the device; a row of no sequence reads no pool, table or length
_DSA_VARLEN_TOO_LARGE = "%s: max_pages * page, total_q * Hq or total_q * ceil(Hq / 64) * splits too large for one launch"


def _index_logits_varlen(name, fp8, q_idx, weights, idx_pool, block_table, seqlens, cu_q, logits):
    """The body of the two packed logits entries: q_idx bf16 [total_q,Hi,128], weights fp32 [total_q,Hi], logits fp32 [total_q,ld]."""
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * 7 + [ctypes.c_int] * 3 + [ctypes.c_longlong] + [ctypes.c_int] * 3 + [ctypes.c_void_p])
    _decode_check((q_idx,) if fp8 else (q_idx, idx_pool), (block_table, seqlens, cu_q), torch.bfloat16)
    for t in (weights, logits):
        _check_dtype(t, torch.float32)
    if fp8:
        P, page = _index_pool_fp8(name, idx_pool)
    _check_dev(idx_pool, weights, logits)
    if q_idx.dim() != 3 or idx_pool.dim() != 3 or block_table.dim() != 2 or logits.dim() != 2:
        raise RuntimeError("Tensor size mismatch!")
    total_q, Hi, D = q_idx.shape
    ld = logits.shape[1]
    if D != _IDX_DIM:
        raise RuntimeError("%s: q_idx of %d dims not supported (%d)" % (name, D, _IDX_DIM))
    if not fp8:
        P, page, _ = idx_pool.shape
        _check_shape(idx_pool, P, page, _IDX_DIM)
    B, max_pages = block_table.shape
    _check_shape(weights, total_q, Hi)
    _check_shape(seqlens, B)
    _check_shape(cu_q, B + 1)
    _check_shape(logits, total_q, ld)
    if Hi > _IDX_MAX_HEADS:
        raise RuntimeError("%s: %d index heads not supported (1 … %d)" % (name, Hi, _IDX_MAX_HEADS))
    if page not in _PAGED_PAGES:
        raise _paged_page_error(name, page)
    rc = fn(q_idx.data_ptr(), weights.data_ptr(), idx_pool.data_ptr(), block_table.data_ptr(), seqlens.data_ptr(), cu_q.data_ptr(),
            logits.data_ptr(), B, total_q, Hi, ld, P, max_pages, page, _stream())
    _raise(name, rc, "%s: max_pages * page or total_q * ceil(cap / 1024) too large for one launch" % name)


def mla_index_logits_paged_varlen_bf16(q_idx, weights, idx_pool, block_table, seqlens, cu_q, logits):
    """mla_index_logits_paged_bf16 for a packed batch; one launch, no workspace. q_idx torch.bfloat16 [total_q,Hi,128]; weights fp32
    [total_q,Hi]; idx_pool torch.bfloat16 [P,page,128]; block_table int32 [B,max_pages]; seqlens int32 [B] (the lengths AFTER the append);
    cu_q int32 [B+1] on the GPU, never read by the host; logits fp32 [total_q,ld], contiguous. For packed row r = cu_q[b] + t writes
    logits[r,j] = sum_h weights[r,h] * max(0, q_idx[r,h] . k_idx[j]) for 0 <= j < vis(r) = clamp(seqlens[b], 0, cap) - (T_b - 1 - t),
    T_b = cu_q[b+1] - cu_q[b], cap = min(max_pages * page, ld), and nothing else; a row of no sequence (in front of cu_q[0], at or behind
    cu_q[B]) writes nothing. T_b = 0 is legal. With cu_q = [0, T, 2T, …] the bits of mla_index_logits_paged_bf16 on the same tensors. Hi in
    1 … 64. Deterministic. C entry cln_mla_index_logits_paged_varlen_bf16 (include/cln_amd_ext.h); no CPU path."""
    _index_logits_varlen("mla_index_logits_paged_varlen_bf16", False, q_idx, weights, idx_pool, block_table, seqlens, cu_q, logits)


def mla_index_logits_paged_varlen_bf16_fp8(q_idx, weights, idx_pool, block_table, seqlens, cu_q, logits):
    """mla_index_logits_paged_bf16_fp8 for a packed batch: idx_pool torch.uint8 [P,page,132] (the layout: index_pool_fp8_views), the scale of
    a key once after the head sum; the packed convention, vis, the rows of no sequence and everything else as in
    mla_index_logits_paged_varlen_bf16. With cu_q = [0, T, 2T, …] the bits of mla_index_logits_paged_bf16_fp8. Deterministic. C entry
    cln_mla_index_logits_paged_varlen_bf16_fp8 (include/cln_amd_ext.h); no CPU path."""
    _index_logits_varlen("mla_index_logits_paged_varlen_bf16_fp8", True, q_idx, weights, idx_pool, block_table, seqlens, cu_q, logits)


def mla_index_topk_varlen(logits, seqlens, cu_q, topk, indices):
    """mla_index_topk for a packed batch; one launch, no workspace. logits fp32 [total_q,ld], contiguous; seqlens int32 [B]; cu_q int32 [B+1]
    on the GPU; indices int32 [total_q,topk], contiguous, every slot of every row written on every call. For packed row r = cu_q[b] + t,
    n = max(clamp(seqlens[b], 0, ld) - (T_b - 1 - t), 0) and the list is mla_index_topk's: dense for n <= topk, else the topk first under
    (logit descending, position ascending) in ascending position order. A row of no sequence gets topk times -1 and reads nothing. The list is
    what fa2_decode_paged_mla_sparse_varlen_bf16 takes. Deterministic. C entry cln_mla_index_topk_varlen (include/cln_amd_ext.h); no CPU path."""
    name = "mla_index_topk_varlen"
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * 4 + [ctypes.c_int] * 2 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p])
    _check_dtype(logits, torch.float32)
    for t in (seqlens, cu_q, indices):
        _check_dtype(t, torch.int32)
    _check_dev(logits, seqlens, cu_q, indices)
    if logits.dim() != 2 or indices.dim() != 2 or seqlens.dim() != 1:
        raise RuntimeError("Tensor size mismatch!")
    total_q, ld = logits.shape
    B = seqlens.shape[0]
    topk = int(topk)
    _check_shape(cu_q, B + 1)
    _check_shape(indices, total_q, topk)
    rc = fn(logits.data_ptr(), seqlens.data_ptr(), cu_q.data_ptr(), indices.data_ptr(), B, total_q, ld, topk, _stream())
    _raise(name, rc, "%s: ld, total_q or topk * total_q too large for one launch" % name)


def fa2_decode_paged_mla_sparse_varlen_bf16_plan(total_q, Hq, topk, max_pages, page):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_mla_sparse_varlen_bf16: fa2_decode_paged_mla_sparse_bf16_plan with total_q in the
    place of B * T -- a function of the packed rows, not of the offsets (cln_fa2_decode_paged_mla_sparse_varlen_bf16_plan,
    include/cln_amd_ext.h). Hq in 1 … 128, topk >= 1. No GPU needed."""
    return _mla_sparse_varlen_plan("fa2_decode_paged_mla_sparse_varlen_bf16", total_q, Hq, topk, max_pages, page)


def fa2_decode_paged_mla_sparse_varlen_bf16_fp8_plan(total_q, Hq, topk, max_pages, page):
    """(splits, chunk, workspace_bytes) of fa2_decode_paged_mla_sparse_varlen_bf16_fp8: exactly fa2_decode_paged_mla_sparse_varlen_bf16_plan's
    (cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8_plan, include/cln_amd_ext.h). No GPU needed."""
    return _mla_sparse_varlen_plan("fa2_decode_paged_mla_sparse_varlen_bf16_fp8", total_q, Hq, topk, max_pages, page)


def _mla_sparse_varlen_plan(name, total_q, Hq, topk, max_pages, page):
    dims = tuple(map(int, (total_q, Hq, topk, max_pages, page)))
    rc, plan = _decode_plan("cln_%s_plan" % name, dims)
    if rc == -2:
        if dims[1] > _MLA_MAX_HQ:
            raise RuntimeError("%s: %d query heads not supported (1 … %d)" % (name, dims[1], _MLA_MAX_HQ))
        if dims[-1] not in _PAGED_PAGES:
            raise _paged_page_error(name, dims[-1])
        raise RuntimeError(_DSA_VARLEN_TOO_LARGE % name)
    _raise(name, rc)
    return plan


def _mla_sparse_varlen(name, plan, q, pool, block_table, seqlens, cu_q, kv_scale, indices, softmax_scale, out, lse, workspace):
    """The body of the two packed sparse entries: q bf16 [total_q,Hq,576], indices int32 [total_q,topk], out bf16 [total_q,Hq,512], lse fp32
    [total_q,Hq]; the pool holds bf16, or for the *_fp8 entry e4m3 with kv_scale: one more input pointer behind cu_q."""
    fp8 = name.endswith("_fp8")
    fn = _ext_fn("cln_" + name, [ctypes.c_void_p] * (9 + fp8) + [ctypes.c_longlong] + [ctypes.c_int] * 7 + [ctypes.c_float, ctypes.c_void_p])
    scale = _softmax_scale(name, softmax_scale)
    _decode_check((q, out) if fp8 else (q, pool, out), (block_table, seqlens, cu_q, indices), torch.bfloat16)
    if fp8:
        _mla_fp8_check(name, pool, kv_scale)
    if q.dim() != 3 or pool.dim() != 3 or block_table.dim() != 2 or indices.dim() != 2:
        raise RuntimeError("Tensor size mismatch!")
    total_q, Hq, Dk = q.shape
    P, page, _ = pool.shape
    if Dk != _MLA_DK:
        raise RuntimeError("%s: q of %d dims not supported (%d = 512 latent + 64 rotary)" % (name, Dk, _MLA_DK))
    _check_shape(pool, P, page, _MLA_DK)
    B, max_pages = block_table.shape
    _check_shape(out, total_q, Hq, _MLA_DC)
    _check_shape(seqlens, B)
    _check_shape(cu_q, B + 1)
    topk = indices.shape[1]
    _check_shape(indices, total_q, topk)
    if not indices.is_contiguous():
        raise RuntimeError("%s: indices must be contiguous [total_q,topk]" % name)
    lse_ptr = _decode_lse(lse, total_q, Hq)
    ws_ptr, ws_bytes = _decode_workspace(name, plan(total_q, Hq, topk, max_pages, page)[2], workspace, q.device)
    more = (kv_scale.data_ptr(),) if fp8 else ()
    rc = fn(q.data_ptr(), pool.data_ptr(), block_table.data_ptr(), seqlens.data_ptr(), cu_q.data_ptr(), *more, indices.data_ptr(), out.data_ptr(),
            lse_ptr, ws_ptr, ws_bytes, B, total_q, Hq, topk, P, max_pages, page, scale, _stream())
    _raise(name, rc)


def fa2_decode_paged_mla_sparse_varlen_bf16(q, pool, block_table, seqlens, cu_q, indices, softmax_scale, out, lse=None, workspace=None):
    """fa2_decode_paged_mla_sparse_bf16 for a packed batch: the attention of a DeepSeek-V3.2 step that mixes prompt chunks and decode rows, one
    call. q torch.bfloat16 [total_q,Hq,576], absorbed; pool torch.bfloat16 [P,page,576]; block_table int32 [B,max_pages]; seqlens int32 [B]
    (the lengths AFTER the append); cu_q int32 [B+1] on the GPU, never read by the host; indices int32 [total_q,topk], contiguous (what
    mla_index_topk_varlen writes); out torch.bfloat16 [total_q,Hq,512]; lse fp32 [total_q,Hq] or None. For packed row r = cu_q[b] + t a slot
    is valid iff 0 <= idx < vis(r) = clamp(seqlens[b], 0, max_pages * page) - (T_b - 1 - t), T_b = cu_q[b+1] - cu_q[b]; from there every rule
    of fa2_decode_paged_mla_sparse_bf16 holds. A row of no sequence reads no pool, table or length and gets O = 0, LSE = -inf. With
    cu_q = [0, T, 2T, …] the plan and the bits of fa2_decode_paged_mla_sparse_bf16 on the same tensors. workspace: at least
    fa2_decode_paged_mla_sparse_varlen_bf16_plan(...)[2] bytes; allocated here when None and the plan splits the list. Deterministic. C entry
    cln_fa2_decode_paged_mla_sparse_varlen_bf16 (include/cln_amd_ext.h); no CPU path."""
    _mla_sparse_varlen("fa2_decode_paged_mla_sparse_varlen_bf16", fa2_decode_paged_mla_sparse_varlen_bf16_plan, q, pool, block_table, seqlens, cu_q,
                       None, indices, softmax_scale, out, lse, workspace)


def fa2_decode_paged_mla_sparse_varlen_bf16_fp8(q, pool, block_table, seqlens, cu_q, kv_scale, indices, softmax_scale, out, lse=None,
                                                workspace=None):
    """fa2_decode_paged_mla_sparse_bf16_fp8 for a packed batch: pool torch.float8_e4m3fn [P,page,576], kv_scale fp32 [1] on the GPU as there;
    the packed convention, vis, the rows of no sequence and everything else as in fa2_decode_paged_mla_sparse_varlen_bf16. With
    cu_q = [0, T, 2T, …] the plan and the bits of fa2_decode_paged_mla_sparse_bf16_fp8. Deterministic. C entry
    cln_fa2_decode_paged_mla_sparse_varlen_bf16_fp8 (include/cln_amd_ext.h); no CPU path."""
    _mla_sparse_varlen("fa2_decode_paged_mla_sparse_varlen_bf16_fp8", fa2_decode_paged_mla_sparse_varlen_bf16_fp8_plan, q, pool, block_table, seqlens,
                       cu_q, kv_scale, indices, softmax_scale, out, lse, workspace)
