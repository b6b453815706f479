"""Helpers of tests/test_gpu_ix_edges.py (no GPU needed; proven by tests/test_ix_reference.py before they judge a kernel):

* Python mirrors of the launchers' dispatch arithmetic of csrc/blas1.hip (GEMV, transpose) and csrc/indexing.hip (embedding, histogram) -- which
  kernel a call takes, how often its unrolled and remainder loops trip, whether a grid-stride loop trips twice, whether the last workgroup is
  partial. The constants are pinned to the sources by test_ix_reference.py. The SGEMM tile form is asked from the built library
  (manifest.describe evaluates csrc/sgemm.hip sgemm_plan on the host);
* the shape lists of the GPU tests, which reach every cell of those mirrors;
* inputs whose answers are exact: small integers for GEMV / SGEMM, pairwise distinct values and bit patterns for transpose / embedding.

Guard bands are those of tests/bw_reference.py (guarded / guards_intact / untouched), imported unchanged."""
import math

import torch

from bw_reference import STREAM_CUS, STREAM_WGS_PER_CU, guarded, guards_intact, untouched  # noqa: F401  (re-exported for the GPU file)

# ---------------------------------------------------------------- constants of the sources (pinned by test_ix_reference.py)
WAVE = 64
GEMV_U = 8                      # blas1.hip gemv_kernel: constexpr int U = 8
GEMV_ROWS_U = {1: 8, 4: 4}      # CLN_GEMV: launch_gemv_rows<T, VEC, R, 8> (one element per lane) / <T, VEC, R, 4> (x4)
GEMV_ROWS_M = 4096              # rows form from this many rows on (f16 rungs only), two rows per wave
GEMV_ROWS4_M = 16384            # four rows per wave from here on
GEMV_WIDE_K = 512               # one-element rungs: K % 64 == 0 and K >= 512 -> 64 lanes per row
GEMV_ROWS4X_PIECES = 4          # x4 rows form: K % (64 * VEC) == 0 and K >= 4 * 64 * VEC
TR_NT = 256
TR_LDS_TILE = 64
TR_REG_BLOCK = 32
EMB_NT = 256
EMB_KP = 4
EMB_KP1_TRAFFIC = 512 << 20     # 16-byte rungs: one pack per lane from here on
NT_TRAFFIC = 256 << 20          # common.h cln_stream_nt
HIST_LDS_BINS = 8192
HIST_LDS_NT = 1024
HIST_LDS_MAX_WG = 256
HIST_GLOBAL_NT = 256
HIST_GLOBAL_MAX_WG = 4096
HIST_UNROLL = 4
SGEMM_BK = 16                   # sgemm_dma stage depth
SGEMM_RING = 3                  # ring slots
SGEMM_KSPLIT_K = 512            # sgemm_plan: K >= 512 and
SGEMM_KSPLIT_TILES = 128        # at most this many 64x128 tiles -> two halves of K

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1

# ---------------------------------------------------------------- GEMV
# name -> (torch dtype name, VEC, G of the CLN_GEMV line)
GEMV_RUNGS = {"sgemv_k32_f32": ("float32", 1, 32), "sgemv_k128_f32x4": ("float32", 4, 32), "sgemv_k16_f32": ("float32", 1, 16),
              "hgemv_k32_f16": ("float16", 1, 32), "hgemv_k128_f16x4": ("float16", 4, 32), "hgemv_k16_f16": ("float16", 1, 16)}


def gemv_cell(name, M, K):
    """The launch of csrc/blas1.hip CLN_GEMV(name) on a [M, K]: `form` "g16" / "g32" / "g64" (gemv_kernel<G>: 64 / G rows per wave), "rows2" /
    "rows4" (gemv_rows_kernel<R>: R rows per wave, 64 lanes on each) or "unsupported"; `lanes` per row, `VEC`, `U`, `piece` (elements one load
    instruction of a row covers), `unrolled` / `rem` (trips of the U-deep loop and of the remainder loop, the same for every lane), `grid`,
    `last_rows` (rows the last workgroup holds, of `rpb`)."""
    dname, VEC, G = GEMV_RUNGS[name]
    half = dname == "float16"
    ok = K == 16 if G == 16 else K % (32 * VEC) == 0
    if not ok or M <= 0 or K <= 0:
        return {"form": "unsupported"}
    U, R = GEMV_U, 0
    if G == 32 and VEC == 1 and half and K % 64 == 0 and K >= GEMV_WIDE_K and M >= GEMV_ROWS_M:
        R, U = (4 if M >= GEMV_ROWS4_M else 2), GEMV_ROWS_U[1]
    elif G == 32 and VEC == 1 and K % 64 == 0 and K >= GEMV_WIDE_K:
        G = 64
    elif G == 32 and VEC > 1 and half and K % (64 * VEC) == 0 and K >= GEMV_ROWS4X_PIECES * 64 * VEC and M >= GEMV_ROWS_M:
        R, U = (4 if M >= GEMV_ROWS4_M else 2), GEMV_ROWS_U[4]
    lanes = 64 if R else G
    piece = lanes * VEC
    pieces = K // piece
    rpb = 4 * R if R else 4 * (64 // G)
    grid = (M + rpb - 1) // rpb
    return {"form": "rows%d" % R if R else "g%d" % G, "lanes": lanes, "VEC": VEC, "U": U, "piece": piece, "unrolled": pieces // U,
            "rem": pieces % U, "grid": grid, "rpb": rpb, "last_rows": M - (grid - 1) * rpb}


def gemv_lane_trips(K, lanes, VEC, U, lane):
    """The two loops of gemv_kernel / gemv_rows_kernel walked for one lane: (unrolled trips, remainder trips, elements covered)."""
    k, un, rem, seen = lane * VEC, 0, 0, []
    while k + (U - 1) * lanes * VEC < K:
        seen += [k + u * lanes * VEC + e for u in range(U) for e in range(VEC)]
        k += U * lanes * VEC
        un += 1
    while k < K:
        seen += [k + e for e in range(VEC)]
        k += lanes * VEC
        rem += 1
    return un, rem, seen


GEMV_SMALL_M = (1, 5, 9, 17, 37)
GEMV_EDGE_M = (4095, 4096, 4097, 16383, 16384, 16385, 16386, 16387)
GEMV_M = GEMV_SMALL_M + GEMV_EDGE_M
# K per kernel form: zero, one and two unrolled trips with zero, one and U - 1 remainder trips
GEMV_K = {"g32x1": (32, 224, 256, 288, 480, 544), "g64": (512, 576, 960, 1024), "g32x4": (128, 896, 1024, 1152),
          "rows_x1": (512, 576, 960, 1088), "rows_x4": (1024, 1280, 1792, 2304), "g16": (16,)}


def gemv_Ks(name):
    _, VEC, G = GEMV_RUNGS[name]
    if G == 16:
        return GEMV_K["g16"]
    keys = ("g32x1", "g64", "rows_x1") if VEC == 1 else ("g32x4", "rows_x4")
    return tuple(sorted(set(k for key in keys for k in GEMV_K[key])))


def gemv_cases(name):
    """Every (M, K) of the GPU tests for one name."""
    return [(M, K) for K in gemv_Ks(name) for M in GEMV_M]


def gemv_impulse_k0(cell, K):
    """Positions of an x impulse: 0, VEC - 1, the last element of the first load instruction, the first of the next, the last of the unrolled part,
    the first of the remainder, K - 1 (those that exist)."""
    edge = cell["unrolled"] * cell["U"] * cell["piece"]
    ks = [0, cell["VEC"] - 1, cell["piece"] - 1, cell["piece"], edge - 1, edge, K - 1]
    return sorted(set(k for k in ks if 0 <= k < K))


GEMV_RANGE = 4  # operands are integers in [-4, 4]


def gemv_exact_inputs(M, K, seed):
    """(a int8 [M, K], x int8 [K]) with |values| <= 4. Rows with m % 4 == 1 carry the sign of x (every product >= 0): their sums reach K * 16 / 3
    or so, past 2048, where the half result is a rounded one. sum |a||x| <= 16 K < 2^24 for every K used: every partial sum in every order is an
    integer that fp32 holds."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-GEMV_RANGE, GEMV_RANGE + 1, (M, K), generator=g, dtype=torch.int8)
    x = torch.randint(-GEMV_RANGE, GEMV_RANGE + 1, (K,), generator=g, dtype=torch.int8)
    a[1::4] = a[1::4].abs() * torch.sign(x).view(1, K)
    return a, x


def int_matvec(a, x):
    """The exact product in int64."""
    return torch.mv(a.to(torch.int64), x.to(torch.int64))


def abs_sum_bound(a, b):
    """max over outputs of sum_k |a||b| (int64): below 2^24 every partial sum of every order is exact in fp32."""
    a, b = a.to(torch.int64).abs(), b.to(torch.int64).abs()
    return int(torch.mv(a, b).max()) if b.dim() == 1 else int((a @ b).max())


def half_rne(v):
    """int64 -> the nearest half, ties to even, in integer arithmetic; |v| >= 65520 (the tie between 65504, the largest finite half, and 2^16,
    which goes to the even side, away from 65504) gives +-inf; returned as float16."""
    v = v.to(torch.int64)
    mag = v.abs()
    out = mag.clone()
    for sh in range(1, 6):  # mag in [2^(10 + sh), 2^(11 + sh)): the half grid there has spacing 2^sh
        sel = (mag >= (1 << (10 + sh))) & (mag < (1 << (11 + sh)))
        q, r, halfway = mag >> sh, mag & ((1 << sh) - 1), 1 << (sh - 1)
        up = (r > halfway) | ((r == halfway) & ((q & 1) == 1))
        out = torch.where(sel, (q + up.long()) << sh, out)
    res = (torch.sign(v) * out).double()
    res = torch.where(mag >= 65520, torch.sign(v).double() * float("inf"), res)
    return res.to(torch.float16)


def hgemv_bound(ref, K):
    """The sgemv rule (rtol 1e-5, atol 1e-4 sqrt(K)) on the fp32 sum, then one rounding of that sum to half: 2^-11 |ref| (normal range) + 2^-25
    (half an ulp of the subnormal range), the fp32 error itself rounded with the sum (factor 1 + 2^-11). `ref` in float64."""
    return 2.0 ** -11 * ref.abs() + 2.0 ** -25 + (1e-5 * ref.abs() + 1e-4 * K ** 0.5) * (1 + 2.0 ** -11)


def sgemv_bound(ref, K):
    return 1e-5 * ref.abs() + 1e-4 * K ** 0.5


# ---------------------------------------------------------------- transpose
# name -> kind (the TrKind of its CLN_TR line)
TR_RUNGS = {"mat_transpose_f32_col2row": "read1", "mat_transpose_f32x4_col2row": "read4", "mat_transpose_f32_row2col": "write1",
            "mat_transpose_f32x4_row2col": "write4", "mat_transpose_f32_col2row2d": "read1", "mat_transpose_f32x4_col2row2d": "read4_2d",
            "mat_transpose_f32_row2col2d": "write1", "mat_transpose_f32x4_row2col2d": "write4_2d", "mat_transpose_f32_diagonal2d": "diag",
            "mat_transpose_f32x4_shared_col2row2d": "lds", "mat_transpose_f32x4_shared_row2col2d": "lds",
            "mat_transpose_f32x4_shared_bcf_col2row2d": "lds_bcf", "mat_transpose_f32x4_shared_bcf_row2col2d": "lds_bcf"}


def stream_grid(items, block=TR_NT):
    return max(1, min(STREAM_CUS * STREAM_WGS_PER_CU, (items + block - 1) // block))


def tr_cell(name, row, col):
    """The launch of csrc/blas1.hip launch_tr: `kernel` "read1" / "read4" / "write1" / "write4" (grid-stride streaming kernels), "diag", "lds" /
    "lds_bcf", "reg4x4" or "unsupported"; `grid`; `multi`: some lane's grid-stride loop trips more than once; `partial`: the last workgroup is
    partly idle; for "diag": `perm` (the block count is a perfect square above 1: blocks are permuted) and `tail` (elements behind the last whole
    block, never permuted)."""
    kind = TR_RUNGS[name]
    n = row * col
    cell = {"multi": False, "perm": False, "tail": False, "partial": False}
    if kind in ("read4_2d", "write4_2d"):
        if row % TR_REG_BLOCK == 0 and col % TR_REG_BLOCK == 0:
            waves = (row // TR_REG_BLOCK) * (col // TR_REG_BLOCK)
            cell.update(kernel="reg4x4", grid=(waves + 3) // 4, partial=waves % 4 != 0)
            return cell
        kind = kind[:-3]
    if (kind == "read4" and col % 4) or (kind == "write4" and row % 4):
        return {"kernel": "unsupported"}
    if kind in ("lds", "lds_bcf"):
        if row % TR_LDS_TILE or col % TR_LDS_TILE:
            return {"kernel": "unsupported"}
        cell.update(kernel=kind, grid=(row // TR_LDS_TILE) * (col // TR_LDS_TILE))
        return cell
    if kind == "diag":
        nb = n // TR_NT
        cell.update(kernel="diag", grid=(n + TR_NT - 1) // TR_NT, perm=nb > 1 and math.isqrt(nb) ** 2 == nb, tail=n % TR_NT != 0,
                    partial=n % TR_NT != 0)
        return cell
    items = n // (4 if kind in ("read4", "write4") else 1)
    grid = stream_grid(items)
    cell.update(kernel=kind, grid=grid, multi=items > grid * TR_NT, partial=items % TR_NT != 0)
    return cell


def diag_block(b, nb):
    """Block that workgroup b of tr_write_coalesced<1, true> writes (nb whole blocks)."""
    side = math.isqrt(nb)
    if nb > 1 and side * side == nb:
        return (b % side) * side + (b // side + b % side) % side
    return b


TR_BIG = (2052, 4100)  # 2 103 300 float4 items: just past the 2 097 152 lanes of a capped grid; no extent divides by 32
TR_SHAPES = {
    "scalar": [(1, 1), (1, 257), (257, 1), (37, 53)],
    "read4": [(1, 4), (5, 8), (37, 52)],
    "write4": [(4, 1), (8, 5), (52, 37)],
    "reg": [(32, 32), (32, 96), (96, 32), (160, 224), (64, 64)],  # (the last: four waves, a whole workgroup)
    "lds": [(64, 64), (64, 192), (192, 64), (128, 320)],
    "diag": [(16, 16), (48, 48), (33, 32), (37, 53)],
}
TR_REFUSED = {"read4": [(36, 50)], "write4": [(50, 36)], "lds": [(64, 96)]}  # (col % 4 on the read side, row % 4 on the write side)


def tr_shapes(name):
    """(accepted shapes, refused shapes) of one name; the grid-stride shape TR_BIG is on the list of every name that accepts it."""
    kind = TR_RUNGS[name]
    if kind in ("read1", "write1"):
        return TR_SHAPES["scalar"] + [TR_BIG], []
    if kind == "diag":
        return TR_SHAPES["scalar"] + TR_SHAPES["diag"] + [TR_BIG], []
    if kind in ("lds", "lds_bcf"):
        return TR_SHAPES["lds"], TR_REFUSED["lds"] + [TR_BIG]
    side = "read4" if kind.startswith("read4") else "write4"
    other = "write4" if side == "read4" else "read4"
    ok = TR_SHAPES[side] + TR_REFUSED[other] + [TR_BIG] + (TR_SHAPES["reg"] if kind.endswith("_2d") else [(32, 96), (96, 32)])
    return ok, TR_REFUSED[side]


def distinct_f32(n, seed):
    """n pairwise distinct integers below 2^24 as float32: arange, scrambled."""
    assert n < (1 << 24)
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(torch.float32)


# ---------------------------------------------------------------- embedding
# name -> (torch dtype name, VEC)
EMB_RUNGS = {"embedding_f32": ("float32", 1), "embedding_f32x4": ("float32", 4), "embedding_f32x4_pack": ("float32", 4),
             "embedding_f16": ("float16", 1), "embedding_f16x8": ("float16", 8), "embedding_f16x8_pack": ("float16", 8)}


def emb_cell(name, n, emb):
    """The launch of csrc/indexing.hip launch_emb: `KP` packs per lane, `nt` (non-temporal stores), `grid`, `partial` (lanes of the last
    workgroup without a pack), `ppr` packs per row; {"KP": 0} where the launcher refuses (emb % VEC) or launches nothing (n == 0)."""
    dname, VEC = EMB_RUNGS[name]
    eb = 4 if dname == "float32" else 2
    if emb % VEC or n <= 0:
        return {"KP": 0}
    ppr = emb // VEC
    total = n * ppr
    traffic = 2 * n * emb * eb
    kp = 1 if (VEC * eb >= 16 and traffic >= EMB_KP1_TRAFFIC) else EMB_KP
    per_wg = EMB_NT * kp
    return {"KP": kp, "nt": traffic >= NT_TRAFFIC, "grid": (total + per_wg - 1) // per_wg, "partial": total % per_wg != 0, "ppr": ppr,
            "total": total, "traffic": traffic}


def emb_block_live(total, kp, block):
    """live[k][lane] of embedding_kernel for one workgroup, lane by lane."""
    return [[block * (EMB_NT * kp) + lane + k * EMB_NT < total for lane in range(EMB_NT)] for k in range(kp)]


EMB_VOCAB = 64
EMB_WIDE = 1024  # vocab * emb = 65536: the f16 table holds every 16-bit pattern


def emb_small_cases(name):
    """(n, emb, vocab): one pack; n = 3 of emb = 24 (3, 6 or 24 packs per row: none divides 256); total one below, at and above 256 * 4."""
    _, VEC = EMB_RUNGS[name]
    return [(1, VEC, 5), (3, 24, 7), (45, 24, 7), (1023, VEC, 9), (1024, VEC, 9), (1025, VEC, 9)]


def emb_traffic_cases(name):
    """(n, emb, vocab) with a small table, so that only the output is large: exactly 256 MB (nt stores, four packs per lane), exactly 512 MB (one
    pack per lane on the 16-byte rungs), and a row length / count that leaves the last workgroup partial from 256 MB and from 512 MB on (the f16
    table of 1032 columns has 63 rows: 65016 distinct patterns)."""
    dname, _ = EMB_RUNGS[name]
    if dname == "float32":
        return [(32768, EMB_WIDE, EMB_VOCAB), (65536, EMB_WIDE, EMB_VOCAB), (32769, 1028, EMB_VOCAB), (65537, 1028, EMB_VOCAB)]
    return [(65536, EMB_WIDE, EMB_VOCAB), (131072, EMB_WIDE, EMB_VOCAB), (65537, 1032, 63), (131073, 1032, 63)]


F32_SPECIALS = (0x7fc00001, 0xffc12345 - (1 << 32), 0x7f800001, 0x00000001, 0x807fffff - (1 << 32), 0x80000000 - (1 << 32), 0x7f800000, 0)
F16_SPECIALS = (0x7e01, 0xfe55 - (1 << 16), 0x7c01, 0x0001, 0x83ff - (1 << 16), 0x8000 - (1 << 16), 0x7c00, 0)


def emb_table_bits(vocab, emb, dname, seed):
    """[vocab, emb] pairwise distinct bit patterns (int32 / int16; view them as float32 / float16): NaN payloads, denormals, -0 and infinities lead
    the table (as far as it is long), the rest is a bijective scramble of arange -- for vocab * emb = 65536 halves, every 16-bit pattern."""
    n = vocab * emb
    if dname == "float32":
        bits = ((torch.arange(n, dtype=torch.int64) * 2654435761 + seed * 40503 + 977) & 0xffffffff)
        bits = torch.where(bits >= (1 << 31), bits - (1 << 32), bits)
        special, idt = F32_SPECIALS, torch.int32
    else:
        assert n <= 65536
        bits = torch.randperm(65536, generator=torch.Generator().manual_seed(seed))[:n] - 32768
        special, idt = F16_SPECIALS, torch.int16
    for i, s in enumerate(special[:min(len(special), n)]):  # put each special where it already is, or swap it in
        at = (bits == s).nonzero()
        if at.numel():
            bits[int(at[0])] = bits[i]
        bits[i] = s
    return bits.to(idt).view(vocab, emb)


def emb_indices(n, vocab, seed, oob=True):
    """int32 [n]: valid rows with -1, vocab, INT_MIN, INT_MAX, vocab + 1 mixed in (every 7th entry or so, the first and last valid)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, vocab, (n,), generator=g, dtype=torch.int64)
    if n:
        idx[0], idx[-1] = vocab - 1, 0
    if oob and n > 2:
        bad = torch.tensor([-1, vocab, INT_MIN, INT_MAX, vocab + 1], dtype=torch.int64)
        at = torch.arange(1, n - 1, 7)
        idx[at] = bad[torch.arange(at.numel()) % 5]
    return idx.to(torch.int32)


def emb_reference_bits(idx, table_bits):
    """out bits: table rows, all-zero bits where the index is outside [0, vocab)."""
    vocab = table_bits.shape[0]
    i = idx.to(torch.int64)
    ok = (i >= 0) & (i < vocab)
    out = table_bits[i.clamp(0, vocab - 1)]
    out[~ok] = 0
    return out


# ---------------------------------------------------------------- histogram
HIST_RUNGS = {"histogram_i32": 1, "histogram_i32x4": 4}


def hist_cell(name, n, nbins):
    """The launch of csrc/indexing.hip launch_hist: `kernel` "lds" / "global" / "none" (n == 0), `grid`, `nt`, `unrolled` (trips of the 4x-unrolled
    loop of lane 0 of workgroup 0, the lane with the most; the global kernel has no such loop), `single` (trips of its one-pack loop), `tail`
    (elements behind the last whole pack, counted by workgroup 0)."""
    VEC = HIST_RUNGS[name]
    if n == 0:
        return {"kernel": "none"}
    nvec = n // VEC
    if nbins <= HIST_LDS_BINS:
        nt = HIST_LDS_NT
        grid = max(1, min(HIST_LDS_MAX_WG, (nvec + nt - 1) // nt))
        stride = grid * nt
        un = max(0, -(-(nvec - 3 * stride) // (4 * stride)))
        left = nvec - un * 4 * stride
        return {"kernel": "lds", "grid": grid, "nt": nt, "unrolled": un, "single": max(0, -(-left // stride)), "tail": n - nvec * VEC, "nvec": nvec}
    nt = HIST_GLOBAL_NT
    grid = max(1, min(HIST_GLOBAL_MAX_WG, (nvec + nt - 1) // nt))
    return {"kernel": "global", "grid": grid, "nt": nt, "unrolled": 0, "single": max(0, -(-nvec // (grid * nt))), "tail": n - nvec * VEC, "nvec": nvec}


def hist_lane_trips(nvec, stride, start):
    """histogram_lds_kernel's two loops walked for the lane whose first pack is `start`: (unrolled trips, single trips, packs visited)."""
    i, un, single, seen = start, 0, 0, []
    while i + 3 * stride < nvec:
        seen += [i, i + stride, i + 2 * stride, i + 3 * stride]
        i += 4 * stride
        un += 1
    while i < nvec:
        seen.append(i)
        i += stride
        single += 1
    return un, single, seen


HIST_EDGE = 3 * HIST_LDS_MAX_WG * HIST_LDS_NT  # packs at which lane 0 of the full LDS grid enters the unrolled loop: nvec > 3 * stride


def hist_sizes(name):
    """n per rung: short inputs (x4: no whole pack at all, every n % 4), the unrolled loop's edge at the full grid one pack below, at and above
    (x4: times 4, plus every n % 4), and for the global kernel a second trip of its grid-stride loop."""
    VEC = HIST_RUNGS[name]
    short = [1, 2, 3, 5, 6, 7, 1000 + VEC - 1]
    edge = [(HIST_EDGE + d) * VEC for d in (-1, 0, 1)]
    if VEC > 1:
        edge += [(HIST_EDGE + 1) * VEC + r for r in (1, 2, 3)] + [HIST_EDGE * VEC - 1]
    loop2 = [(HIST_GLOBAL_MAX_WG * HIST_GLOBAL_NT + 300) * VEC + VEC - 1, (2 * 4 * HIST_LDS_MAX_WG * HIST_LDS_NT + 3 * HIST_LDS_NT + 5) * VEC + VEC - 1]
    return short + edge + loop2


def hist_values(n, nbins, seed):
    """int32 [n]: about two thirds valid bins (bin 0, nbins - 1 and a crowded bin among them), the rest negative values, nbins, nbins + 1, INT_MIN and
    INT_MAX -- all of which the kernels must ignore."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, nbins, (n,), generator=g, dtype=torch.int64)
    kind = torch.randint(0, 12, (n,), generator=g)
    bad = torch.tensor([-1, -nbins, nbins, nbins + 1, INT_MIN, INT_MAX], dtype=torch.int64)
    v = torch.where(kind < 4, bad[(kind + torch.arange(n)) % 6], v)
    v = torch.where(kind == 4, torch.full_like(v, nbins // 2), v)
    if n > 1:
        v[0], v[-1] = nbins - 1, 0
    return v.to(torch.int32)


def hist_reference(v, nbins):
    v = v.to(torch.int64)
    return torch.bincount(v[(v >= 0) & (v < nbins)], minlength=nbins)


# ---------------------------------------------------------------- SGEMM
MFMA_NAMES = ("sgemm_wmma_m16n16k8_mma4x2_warp2x4_stages", "sgemm_wmma_m16n16k8_mma4x2_warp2x4_stages_dsmem")
SGEMM_TILE_SHAPES = {"64x128": (192, 256), "128x128": (1792, 3584), "256x128": (8192, 8192)}  # (M, N) the planner sends to each tile form
SGEMM_STAGE_KS = tuple(SGEMM_BK * s for s in range(1, 8))                                  # one to seven stages
SGEMM_KSPLIT_SHAPE = (128, 256)
SGEMM_KSPLIT_KS = (512, 528, 544, 560, 576, 592)                                           # halves 16+16, 17+16, 17+17, 18+17, 18+18, 19+18
SGEMM_RANGE = 4
# VALU ladder: name -> (BK, TN)
VALU_RUNGS = {"sgemm_t_8x8_sliced_k_f32x4": (8, 8), "sgemm_t_8x8_sliced_k_f32x4_bcf": (8, 8), "sgemm_t_8x8_sliced_k_f32x4_bcf_offset": (8, 8),
              "sgemm_t_8x8_sliced_k_f32x4_bcf_dbuf": (8, 8), "sgemm_t_8x8_sliced_k_f32x4_bcf_dbuf_offset": (8, 8),
              "sgemm_t_8x4_sliced_k16_f32x4_bcf_dbuf": (16, 4), "sgemm_t_8x4_sliced_k16_f32x4_bcf_dbuf_async": (16, 4),
              "sgemm_t_8x8_sliced_k16_f32x4_bcf_dbuf": (16, 8), "sgemm_t_8x8_sliced_k16_f32x4_bcf_dbuf_async": (16, 8),
              "sgemm_t_8x16_sliced_k16_f32x4_bcf_dbuf": (16, 16), "sgemm_t_8x16_sliced_k16_f32x4_bcf_dbuf_async": (16, 16)}
VALU_K_TILES = (1, 2, 3, 5)
ANY_SHAPE_NAMES = ("sgemm_naive_f32", "sgemm_sliced_k_f32")
ANY_SHAPES = ((1, 4, 1), (33, 68, 37), (100, 100, 50))  # (M, N, K)


def valu_cases(name):
    BK, TN = VALU_RUNGS[name]
    return [(M, N, t * BK) for M in (128, 256) for N in (16 * TN, 32 * TN) for t in VALU_K_TILES]


def ksplit_halves(K):
    """Stages of the two halves of sgemm_dma_kernel<KSPLIT>."""
    nt = K // SGEMM_BK
    first = (nt + 1) // 2
    return first, nt - first


def sgemm_form(describe_text):
    """(tile "64x128" / "128x128" / "256x128", K split) out of the text of manifest.describe."""
    tile = describe_text.split("<")[1].split("x16,")[0]
    return tile, "halves of K" in describe_text


def sgemm_impulse_k0(K, split):
    """Columns of A for the K impulse: first and last of a stage, first of the next, K - 1; with K split also the last column of the first half and
    the first of the second."""
    ks = [0, SGEMM_BK - 1, SGEMM_BK, K - 1]
    if split:
        first, _ = ksplit_halves(K)
        ks += [first * SGEMM_BK - 1, first * SGEMM_BK]
    return sorted(set(k for k in ks if 0 <= k < K))


def sgemm_exact_inputs(M, N, K, seed, device="cpu"):
    """A [M, K], B [K, N] float32 holding integers in [-4, 4]: sum |a||b| <= 16 K < 2^24 for every K used (K <= 592)."""
    g = torch.Generator(device=device).manual_seed(seed)
    a = torch.randint(-SGEMM_RANGE, SGEMM_RANGE + 1, (M, K), generator=g, device=device, dtype=torch.int8)
    b = torch.randint(-SGEMM_RANGE, SGEMM_RANGE + 1, (K, N), generator=g, device=device, dtype=torch.int8)
    return a.to(torch.float32), b.to(torch.float32)
