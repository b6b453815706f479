"""Helpers of tests/test_gpu_bw_edges.py (no GPU needed; proven by tests/test_bw_reference.py before they judge a kernel):

* Python mirrors of the launchers' dispatch arithmetic -- which kernel, grid, partial last workgroup, ragged tail a size takes
  (csrc/rowwise.cuh, elementwise.hip, activation.hip, reduce.hip, blas1.hip, common.h). The constants are pinned to the sources by
  test_bw_reference.py.
* shape choosers that walk every reachable cell of those mirrors;
* inputs whose answers are exact (small integers), the 256 fp8 codes, guard-band allocation;
* the tolerance rules of tests/test_gpu_activation.py / test_gpu_bandwidth.py, copied (the numbers are held equal to the originals' text).
"""
import torch

# ---------------------------------------------------------------- constants of the sources (pinned by test_bw_reference.py)
ROW_PACKS_PER_LANE = 8        # rowwise.cuh row_threads: (nvec + 7) / 8
ROW_NT_CAP = 1024             # rowwise.cuh row_threads: nt > 1024 -> 1024
ROW_MAXV = (1, 2, 4, 8)       # ROWWISE_DISPATCH_MAXV_FULL
WAVE = 64
STREAM_NT = 256               # __launch_bounds__(256) of the add / unary kernels
STREAM_K1_BLOCKS = 1024       # nvec < 1024 * KB -> the K = 1 kernel
STREAM_KB_WIDE = 4            # KB for accesses of >= 16 bytes
STREAM_KB_BYTES = 64          # ... else 64 / AB packs per lane,
STREAM_KB_MAX = 16            # at most 16
STREAM_WGS_PER_CU = 32        # common.h CLN_STREAM_WGS_PER_CU
STREAM_CUS = 256              # common.h cln_stream_grid: 256LL * CLN_STREAM_WGS_PER_CU
STREAM_CAP_LIFT = 512 << 20   # traffic from which the grid cap is lifted / add's 16-byte rungs go back to one pack per lane
RED_NT = 256
RED_MAX_WG = 1024
RED_K = (4, 8)                # reduce: 16-byte packs / narrower
DOT_K = (2, 4)                # dot
SOFTMAX_ONE_BLOCK_MAX = 65536


ROPE_CAP_WG = 16384           # rope.hip launch_rope: at most this many workgroups,
ROPE_MIN_ROWS = 4             # at least this many rows per thread (also the unroll factor of the row loop)

# ---------------------------------------------------------------- rungs: name -> (torch dtype name, elements per pack[, elements per access])
ADD_RUNGS = {"f32": ("float32", 1, 1), "f32x4": ("float32", 4, 4), "f16": ("float16", 1, 1), "f16x2": ("float16", 2, 2),
             "f16x8": ("float16", 2, 2), "f16x8_pack": ("float16", 8, 8)}   # add's f16x8 rung runs the half2 kernel
UNARY_RUNGS = {"f32": ("float32", 1, 1), "f32x4": ("float32", 4, 4), "f16": ("float16", 1, 1), "f16x2": ("float16", 2, 2),
               "f16x8": ("float16", 8, 2), "f16x8_pack": ("float16", 8, 8)}
ACT_OPS = ("relu", "sigmoid", "gelu", "swish", "elu", "hardswish", "hardshrink")
REDUCE_RUNGS = {
    "f32_f32": ("float32", 1), "f32x4_f32": ("float32", 4), "f16_f16": ("float16", 1), "f16_f32": ("float16", 1), "f16x2_f16": ("float16", 2),
    "f16x2_f32": ("float16", 2), "f16x8_pack_f16": ("float16", 8), "f16x8_pack_f32": ("float16", 8), "bf16_bf16": ("bfloat16", 1),
    "bf16_f32": ("bfloat16", 1), "bf16x2_bf16": ("bfloat16", 2), "bf16x2_f32": ("bfloat16", 2), "bf16x8_pack_bf16": ("bfloat16", 8),
    "bf16x8_pack_f32": ("bfloat16", 8), "fp8_e4m3_f16": ("float8_e4m3fn", 1), "fp8_e4m3x16_pack_f16": ("float8_e4m3fn", 16),
    "fp8_e5m2_f16": ("float8_e5m2", 1), "fp8_e5m2x16_pack_f16": ("float8_e5m2", 16), "i8_i32": ("int8", 1), "i8x16_pack_i32": ("int8", 16)}
DOT_RUNGS = {"dot_prod_f32_f32": ("float32", 1), "dot_prod_f32x4_f32": ("float32", 4), "dot_prod_f16_f32": ("float16", 1),
             "dot_prod_f16x2_f32": ("float16", 2), "dot_prod_f16x8_pack_f32": ("float16", 8)}
SOFTMAX_RUNGS = {  # name -> (dtype, VEC, mode)
    "softmax_f32_per_token": ("float32", 1, "unsafe"), "softmax_f32x4_per_token": ("float32", 4, "unsafe"),
    "safe_softmax_f32_per_token": ("float32", 1, "safe"), "safe_softmax_f32x4_per_token": ("float32", 4, "safe"),
    "safe_softmax_f16_f32_per_token": ("float16", 1, "safe"), "safe_softmax_f16x2_f32_per_token": ("float16", 2, "safe"),
    "safe_softmax_f16x8_pack_f32_per_token": ("float16", 8, "safe"), "online_safe_softmax_f32_per_token": ("float32", 1, "online"),
    "online_safe_softmax_f32x4_pack_per_token": ("float32", 4, "online")}
LAYER_NORM_RUNGS = {"layer_norm_f32": ("float32", 1), "layer_norm_f32x4": ("float32", 4), "layer_norm_f16_f16": ("float16", 1),
                    "layer_norm_f16x2_f16": ("float16", 2), "layer_norm_f16x8_f16": ("float16", 8), "layer_norm_f16x8_pack_f16": ("float16", 8),
                    "layer_norm_f16x8_pack_f32": ("float16", 8), "layer_norm_f16_f32": ("float16", 1)}
RMS_NORM_RUNGS = {"rms_norm_f32": ("float32", 1), "rms_norm_f32x4": ("float32", 4), "rms_norm_f16_f16": ("float16", 1),
                  "rms_norm_f16x2_f16": ("float16", 2), "rms_norm_f16x8_f16": ("float16", 8), "rms_norm_f16x8_f32": ("float16", 8),
                  "rms_norm_f16x8_pack_f16": ("float16", 8), "rms_norm_f16x8_pack_f32": ("float16", 8), "rms_norm_f16_f32": ("float16", 1)}
ROPE_RUNGS = {"rope_f32": 1, "rope_f32_v2": 1, "rope_f32x4_pack": 2}  # name -> pairs per thread


def elem_bytes(dtype):
    return torch.empty(0, dtype=dtype).element_size()


# ---------------------------------------------------------------- mirrors
def rope_grid(seq_len, hidden, pairs):
    """(gridDim.x, gridDim.y, units per row) of csrc/rope.hip launch_rope<PAIRS>."""
    units = hidden // 2 // pairs
    gx = (units + 255) // 256
    gy = max(1, min(65535, ROPE_CAP_WG // gx, (seq_len + ROPE_MIN_ROWS - 1) // ROPE_MIN_ROWS))
    return gx, gy, units


def rope_shapes(pairs):
    """[seq_len, hidden] whose column units are not a multiple of 256 and span two blockIdx.x, with a seq_len that is a multiple neither of the
    gridDim.y the launcher picks nor of the row loop's unroll factor."""
    return [(37, 2 * pairs * (256 + 3)), (1030, 2 * pairs * (256 + 3))]


def row_threads(K, VEC):
    nvec = K // VEC
    nt = (((nvec + ROW_PACKS_PER_LANE - 1) // ROW_PACKS_PER_LANE + WAVE - 1) // WAVE) * WAVE
    return max(WAVE, min(ROW_NT_CAP, nt))


def row_cell(K, VEC):
    """(nt, MAXV, FULL) of a row of K elements on a rung of VEC elements per pack; FULL is the string "unsupported" where the launcher
    returns CLN_ERR_UNSUPPORTED (K not a multiple of VEC, or more than 8 packs per lane)."""
    nt = row_threads(K, VEC)
    if K % VEC:
        return nt, 0, "unsupported"
    vpt = (K // VEC + nt - 1) // nt
    if vpt > ROW_MAXV[-1]:
        return nt, 0, "unsupported"
    mv = next(m for m in ROW_MAXV if vpt <= m)
    return nt, mv, K == mv * nt * VEC


def row_limit(VEC):
    """The longest supported row of a rung."""
    return ROW_MAXV[-1] * ROW_NT_CAP * VEC


def stream_kb(access_bytes):
    return STREAM_KB_WIDE if access_bytes >= 16 else min(STREAM_KB_MAX, STREAM_KB_BYTES // access_bytes)


def stream_cell(n, elem_bytes, VEC, CHUNK, op="unary"):
    """The launch of csrc/activation.hip launch_unary<Op, T, VEC, CHUNK> (op="unary") or csrc/elementwise.hip launch_add<T, VT, VEC> (op="add",
    CHUNK == VEC) on n elements. `kernel`: "k1" / "kb" (block-contiguous, K packs per lane) or "stride" (grid-stride loop); `packs` counts
    accesses of CHUNK elements; `partial`: the last workgroup takes the per-pack guarded branch; `mixed`: some lane of it holds some but not all
    of its K packs; `tail`: elements behind the last whole pack; `trips`: most loop trips of a lane ("stride")."""
    ab = elem_bytes * CHUNK
    kb = stream_kb(ab)
    streams = 3 if op == "add" else 2
    traffic = streams * n * elem_bytes
    nvec = n // CHUNK
    cell = {"packs": nvec, "tail": n - nvec * CHUNK, "trips": 1, "K": 1, "partial": False, "mixed": False}
    if op == "unary" and ab >= 16:
        items = n // VEC + 1
        cap = 0x7fffffff if traffic >= STREAM_CAP_LIFT else STREAM_CUS * STREAM_WGS_PER_CU
        grid = max(1, min(cap, (items + STREAM_NT - 1) // STREAM_NT))
        cell.update(kernel="stride", grid=grid, trips=max(1, -(-nvec // (grid * STREAM_NT))), partial=nvec % STREAM_NT != 0)
        return cell
    if op == "add" and nvec == 0:
        cell.update(kernel="none", grid=0)
        return cell
    if (op == "add" and ab >= 16 and traffic >= STREAM_CAP_LIFT) or nvec < STREAM_K1_BLOCKS * kb:
        grid = (nvec + STREAM_NT - 1) // STREAM_NT + (1 if (op == "unary" and nvec == 0) else 0)
        cell.update(kernel="k1", grid=grid, partial=nvec % STREAM_NT != 0)
        return cell
    per_wg = STREAM_NT * kb
    grid = (nvec + per_wg - 1) // per_wg
    rem = nvec - (grid - 1) * per_wg                     # packs of the last workgroup
    held = [sum(1 for k in range(kb) if t + k * STREAM_NT < rem) for t in (0, STREAM_NT - 1)]  # lane 0 holds the most, lane 255 the fewest
    cell.update(kernel="kb", K=kb, grid=grid, partial=rem < per_wg, mixed=rem < per_wg and (0 < held[0] < kb or 0 < held[1] < kb))
    return cell


def reduce_cell(n, elem_bytes, VEC, op="reduce"):
    """csrc/reduce.hip launch_reduce / reduce_sum_kernel (op="reduce") and csrc/blas1.hip launch_dot / dot_kernel (op="dot")."""
    wide, narrow = RED_K if op == "reduce" else DOT_K
    K = wide if elem_bytes * VEC >= 16 else narrow
    chunk = RED_NT * K
    nvec = n // VEC
    nfull = nvec // chunk
    chunks = (nvec + chunk - 1) // chunk
    grid = max(1, min(RED_MAX_WG, chunks))
    return {"K": K, "chunk": chunk, "nvec": nvec, "nfull": nfull, "grid": grid, "owner": nfull % grid, "leftover": nvec - nfull * chunk,
            "tail": n - nvec * VEC}


# ---------------------------------------------------------------- shape choosers
def row_Ks(VEC):
    """Row lengths that reach every dispatch cell of a rung: each MAXV with and without FULL on one wave, a non-FULL and a FULL row on an
    intermediate workgroup and on 1024 lanes, the longest supported row (last entry but one), and the first unsupported one (last entry)."""
    packs = [40, 64, 100, 128, 130, 256, 300, 512,   # nt = 64: MAXV 1, 1F, 2, 2F, 4 (3 packs per lane), 4F, 8 (5 packs per lane), 8F
             1000, 2048,                             # nt = 128 guarded, nt = 256 FULL
             8000, 8192]                             # nt = 1024 guarded, FULL = the limit
    return [p * VEC for p in packs] + [row_limit(VEC) + VEC]


def stream_sizes(elem_bytes, VEC, CHUNK, op="unary"):
    """Element counts for one add / unary rung: the K = 1 kernel with a partial block (and a ragged tail where the rung has packs), the K = KB kernel
    on a whole grid, with a last workgroup whose lanes hold some but not all of their packs, the same with a ragged tail; for the grid-stride
    rungs a partial block inside one trip and more than one loop trip (with a tail)."""
    ab = elem_bytes * CHUNK
    kb = stream_kb(ab)
    if op == "unary" and ab >= 16:
        one_trip = STREAM_CUS * STREAM_WGS_PER_CU * STREAM_NT  # packs
        return [1000 * VEC + VEC - 1, (one_trip + 5 * STREAM_NT + 3) * VEC + VEC - 1]
    per_wg = STREAM_NT * kb
    base = STREAM_K1_BLOCKS * kb  # first pack count of the KB kernel
    sizes = [1000 * CHUNK + CHUNK - 1, (base + per_wg) * CHUNK, (base + 3 * STREAM_NT + 17) * CHUNK]
    if CHUNK > 1:
        sizes.append((base + 2 * per_wg + STREAM_NT + 201) * CHUNK + CHUNK - 1)
    return sizes


def reduce_sizes(elem_bytes, VEC, op="reduce"):
    """Element counts for one reduce / dot rung: below one pack, whole chunks only, chunks + left-over packs + ragged tail, and more whole chunks than
    workgroups (not a multiple of them) + left-over packs + tail. The last two are the largest."""
    c = reduce_cell(0, elem_bytes, VEC, op)["chunk"]
    t = VEC - 1
    return [max(1, VEC - 1), 3 * c * VEC, (5 * c + 300) * VEC + t, ((RED_MAX_WG + 7) * c + 77) * VEC + t]


# ---------------------------------------------------------------- exact inputs
FP8 = {"e4m3": "float8_e4m3fn", "e5m2": "float8_e5m2"}
ACC_BITS = {"f32": 24, "f16": 11, "bf16": 8, "i32": 31}  # significand bits (sign excluded) of the in-pack accumulator a rung name states


def exact_sum_inputs(n, dtype, seed):
    """n integers in [-2, 2] (half of them 0, mean |x| = 0.6) stored in `dtype`: every partial sum of every order is an integer below 2^24 while
    sum|x| < 2^24, so fp32 accumulation and the in-pack half / bf16 adds (|pack sum| <= 2 * VEC) are exact and the device result must equal the
    int64 sum."""
    g = torch.Generator().manual_seed(seed)
    levels = torch.tensor([-2, -1, 0, 1, 2], dtype=torch.int8)
    u = torch.rand(n, generator=g)
    idx = (u > 0.05).long() + (u > 0.25).long() + (u > 0.75).long() + (u > 0.95).long()
    return levels[idx].to(torch.float32).to(dtype) if dtype != torch.int8 else levels[idx]


def fp8_code_table(fmt):
    """(values float64[256], is_nan bool[256], is_inf bool[256]) of the OCP fp8 format `fmt` ("e4m3" / "e5m2"), decoded by torch."""
    v = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(getattr(torch, FP8[fmt])).to(torch.float32).double()
    return v, torch.isnan(v), torch.isinf(v)


def fp8_pack16_skip(fmt):
    """Codes whose 16-fold pack sum is NOT exact in fp16 (a partial k * value, k <= 16, needs more than 11 bits or leaves the half range)."""
    v, nan, inf = fp8_code_table(fmt)
    skip = []
    for c in range(256):
        if nan[c] or inf[c]:
            continue
        ks = torch.arange(1, 17, dtype=torch.float64) * v[c]
        if not torch.equal(ks.to(torch.float16).double(), ks):
            skip.append(c)
    return skip


# ---------------------------------------------------------------- guard bands
GUARD_BYTES = 256
BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
_SENTINEL = {1: 0xA5, 2: 0xA5A5 - (1 << 16), 4: 0xA5A5A5A5 - (1 << 32)}


def _fill_bits(dtype, fill):
    eb = torch.empty(0, dtype=dtype).element_size()
    if fill == "sentinel":
        return _SENTINEL[eb]
    assert fill == "nan"
    if dtype == torch.int8:
        return 127
    return int(torch.tensor([float("nan")]).to(dtype).view(BITS[eb]).item())


def guarded(n, dtype, dev, fill):
    """(view, buffer): a contiguous view of n elements of `dtype` with GUARD_BYTES in front and behind it, the whole buffer (payload included)
    filled with `fill`: "nan" (NaN; 127 for int8 -- an over-read poisons a sum) or "sentinel" (bytes 0xA5). Both guards are multiples of 16 bytes:
    the view is as aligned as the buffer."""
    eb = torch.empty(0, dtype=dtype).element_size()
    g = GUARD_BYTES // eb
    buf = torch.full((g + n + g,), _fill_bits(dtype, fill), dtype=BITS[eb], device=dev)
    return buf[g:g + n].view(dtype), buf


def guards_intact(buf, n, dtype, fill):
    eb = torch.empty(0, dtype=dtype).element_size()
    g = GUARD_BYTES // eb
    v = _fill_bits(dtype, fill)
    return bool((buf[:g] == v).all()) and bool((buf[g + n:] == v).all())


def untouched(view, fill):
    """Every element of a guarded view still holds its fill pattern."""
    eb = view.element_size()
    return bool((view.view(BITS[eb]) == _fill_bits(view.dtype, fill)).all())


# ---------------------------------------------------------------- the existing tolerance rules, copied
# (file, the line of the original that states the rule); test_bw_reference.py holds each line present in its file and the numbers equal.
RULE_TEXT = {
    "activation": ("test_gpu_activation.py", "tol = (2e-6, 1e-6) if dt == torch.float32 else (1e-3, 1e-4)"),
    "softmax_f32": ("test_gpu_bandwidth.py", "assert torch.allclose(y.cpu(), ref, atol=2e-6, rtol=2e-5), name"),
    "softmax_f16": ("test_gpu_bandwidth.py", "assert torch.allclose(y.cpu().float(), refh.float(), atol=1e-6, rtol=2e-3), name  # 1 fp16 ulp"),
    "layer_norm_f32": ("test_gpu_bandwidth.py", "assert torch.allclose(y.cpu(), ref_k, atol=2e-5, rtol=1e-5), name"),
    "layer_norm_f16": ("test_gpu_bandwidth.py", "assert torch.allclose(y.cpu().float(), ref_kh.float(), atol=1e-3, rtol=2e-3), name  # 1 fp16 ulp"),
    "rms_norm_f32": ("test_gpu_bandwidth.py", "assert torch.allclose(y.cpu(), ref_k, atol=2e-5, rtol=1e-5), name"),
    "rms_norm_f16": ("test_gpu_bandwidth.py", "assert torch.allclose(y.cpu().float(), ref_kh.float(), atol=1e-3, rtol=2e-3), name"),
    "rope": ("test_gpu_bandwidth.py", "bound = (2e-4 + pair_norm * t * freq * 4.8e-7).repeat_interleave(2, dim=1)"),
}
# (rtol, atol)
RULES = {
    "activation_f32": (2e-6, 1e-6), "activation_f16": (1e-3, 1e-4),
    "softmax_f32": (2e-5, 2e-6), "softmax_f16": (2e-3, 1e-6),
    "layer_norm_f32": (1e-5, 2e-5), "layer_norm_f16": (2e-3, 1e-3),
    "rms_norm_f32": (1e-5, 2e-5), "rms_norm_f16": (2e-3, 1e-3),
}
ROPE_RULE = (2e-4, 4.8e-7, 0.75)  # floor, ulp slack of freq per radian of t * freq * |pair|, share of columns that stay under the floor alone


def excess(got, ref, rule):
    """Worst |got - ref| / (atol + rtol |ref|) over the elements (torch.allclose's rule, as a ratio: <= 1 passes); got and ref in float64.
    Elements where both are the same infinity, or both NaN, count as 0; where only one is non-finite, as inf."""
    rtol, atol = RULES[rule] if isinstance(rule, str) else rule
    got, ref = got.double(), ref.double()
    same = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
    ratio = (got - ref).abs() / (atol + rtol * ref.abs())
    ratio = torch.where(same, torch.zeros_like(ratio), ratio)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    if ratio.numel() == 0:
        return 0.0, -1
    i = int(ratio.argmax())
    return float(ratio.flatten()[i]), i


def rope_bound(x):
    """The bound of tests/test_gpu_bandwidth.py::test_rope_matches_torch_oracle, formed as it forms it."""
    S, Hd = x.shape
    t = torch.arange(S, dtype=torch.float64).view(S, 1)
    freq = (1.0 / (10000.0 ** (torch.arange(0, Hd, 2).float() / Hd))).double().view(1, Hd // 2)
    pair_norm = x.double().view(S, -1, 2).norm(dim=-1)
    return (ROPE_RULE[0] + pair_norm * t * freq * ROPE_RULE[1]).repeat_interleave(2, dim=1)


# ---------------------------------------------------------------- activation sweeps
ACT_THRESHOLDS = (0.5, 3.0, 88.3762626647949)


def half_finite_values():
    """All 63488 finite fp16 values (both zeros included)."""
    codes = torch.cat([torch.arange(0, 0x7c00, dtype=torch.int32), torch.arange(0x8000, 0xfc00, dtype=torch.int32)])
    return (codes - ((codes >= 0x8000).int() << 16)).to(torch.int16).view(torch.float16)


def f32_sweep_values(points=4096):
    """fp32: log-spaced magnitudes from 1e-30 to 3e38 in both signs, +-0, and the kernels' thresholds with both fp32 neighbours."""
    mag = torch.logspace(-30, torch.log10(torch.tensor(3e38, dtype=torch.float64)).item(), points, dtype=torch.float64).float()
    th = torch.tensor(ACT_THRESHOLDS, dtype=torch.float32)
    inf = torch.tensor(float("inf"))
    th = torch.cat([th, torch.nextafter(th, inf), torch.nextafter(th, -inf)])
    pos = torch.cat([mag, th, torch.zeros(1)])
    return torch.cat([pos, -pos])


# ---------------------------------------------------------------- CPU emulation of a row kernel's fp32 arithmetic (second rule of the issue's section 2)
def emulate_row_sum_f32(v, VEC):
    """Row sums of v [S, K] (fp32) in the order of the row kernels: lane t adds its packs t, t + nt, ... element by element, the 64 lanes of a wave
    are folded pairwise, the wave totals added in order."""
    S, K = v.shape
    nt, mv, _ = row_cell(K, VEC)
    vp = torch.cat([v.float(), torch.zeros(S, mv * nt * VEC - K)], dim=1).view(S, mv, nt, VEC)
    lane = torch.zeros(S, nt)
    for i in range(mv):
        for c in range(VEC):
            lane = lane + vp[:, i, :, c]
    w = lane.view(S, nt // WAVE, WAVE)
    width = WAVE
    while width > 1:
        width //= 2
        w = w[:, :, :width] + w[:, :, width:2 * width]
    d = torch.zeros(S)
    for i in range(nt // WAVE):
        d = d + w[:, i, 0]
    return d.view(S, 1)


def emulate_layer_norm_f32(x, g, b, VEC):
    """csrc/norm.hip layer_norm_kernel in fp32 torch: two passes, sums in the kernel's order, y = fma(x - mean, rsqrt(var_sum / (K + 1e-5)) * g, b)."""
    K = x.shape[1]
    xf = x.float()
    mean = emulate_row_sum_f32(xf, VEC) / torch.tensor(float(K))
    d = xf - mean
    a = torch.rsqrt(emulate_row_sum_f32(d * d, VEC) / (torch.tensor(float(K)) + torch.tensor(1e-5))) * torch.tensor(g)
    return torch.addcmul(torch.tensor(b), d, a)


def emulate_softmax_f32(x, VEC, safe=True):
    """The row softmax as the kernel orders it, in fp32 torch: lane-strided partial sums (lane t holds packs t, t + nt, ...), a pairwise wave
    reduction, the wave partials added in order, exp in fp32, y = e * (1 / d). Used only to derive a bound where an existing rule is exceeded."""
    S, K = x.shape
    nt, mv, _ = row_cell(K, VEC)
    xf = x.float()
    m = xf.max(dim=1, keepdim=True).values if safe else torch.zeros(S, 1)
    e = torch.exp(xf - m)
    pad = mv * nt * VEC - K
    ep = torch.cat([e, torch.zeros(S, pad)], dim=1).view(S, mv, nt, VEC)
    lane = torch.zeros(S, nt)
    for i in range(mv):
        for c in range(VEC):
            lane = lane + ep[:, i, :, c]
    w = lane.view(S, nt // WAVE, WAVE)
    width = WAVE
    while width > 1:
        width //= 2
        w = w[:, :, :width] + w[:, :, width:2 * width]
    d = torch.zeros(S)
    for i in range(nt // WAVE):
        d = d + w[:, i, 0]
    return e * (1.0 / d).view(S, 1)
