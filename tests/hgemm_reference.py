"""Helpers of tests/test_gpu_hgemm_edges.py (no GPU needed; proven by tests/test_hgemm_reference.py before they judge a kernel):

* the case table: for every HGEMM kernel family the smallest shapes at which it can still go wrong, each with the entry it is called through.
  Explicit instantiations (VALU rungs, 1-stage MFMA, rings, ping-pong, hgemm_w4 / hgemm_w4s through the probe hook and the fixed-tile names) are
  listed by hand from the launchers' acceptance rules; the shapes of the run-time dispatched names (which tile the planner picks, split-K, tail
  split) are found by search over manifest.describe (host code: csrc/hgemm.hip describe_best / describe_ring / describe_w4);
* inputs whose answers are exact: integers sized per K so that every partial sum in every order and every split is an integer fp32 holds, a
  share of the sums past 2048 (where a half result is a rounded one) and, from K = 4096 on, past 65520 (+-inf);
* a poison plan (one NaN per chosen row of A / column of B, at the edges of K tiles and of fragment / wave / block tiles);
* special values (fp16 subnormal inputs and results, 65504, the tie 65520, +inf against nonzero and against zero).

Guard bands, half_rne (which gives +-inf from 65520 on) and abs_sum_bound are those of tests/ix_reference.py, imported, not copied."""
import functools
import re
from collections import namedtuple

import torch

import ix_reference as ix
from ix_reference import guarded, guards_intact, untouched, half_rne  # noqa: F401  (re-exported for the GPU file)

NN, TN = 0, 1
BEST_NN = "hgemm_mma_m16n8k16_mma2x4_warp4x4x2_stages_dsmem"
BEST_TN = "hgemm_mma_m16n8k16_mma2x4_warp4x4x2_stages_dsmem_tn_swizzle_x4"
FIXED_256x256 = "hgemm_wmma_m16n16k16_mma4x4_warp4x4_stages_dsmem"  # NN
FIXED_256x128 = "hgemm_wmma_m16n16k16_mma4x2_warp4x4_stages_dsmem"  # NN
FIXED_128x256 = "hgemm_mma_stages_block_swizzle_tn_cute"            # TN
LDS_LIMIT = 160 * 1024

# entry: ("g3", name) | ("g6", name, stages) | ("variant", kind, tile, bk, stages) | ("vendor", name)
# bm, bn: block tile; wtm, wtn: wave tile; bk: depth of one K step; scheduled: launched three times (block swizzle alternating);
# big: the reference product is taken on the device in float64 (pinned to the int64 CPU product on sampled rows)
Case = namedtuple("Case", "family cid entry layout M N K bm bn wtm wtn bk scheduled big")
Refused = namedtuple("Refused", "family entry layout M N K")

BIG_MNK = 1 << 28


def _case(family, entry, layout, M, N, K, bm, bn, wtm, wtn, bk, scheduled=False):
    what = entry[1] if entry[0] != "variant" else "variant(kind=%d,tile=%d,bk=%d,stages=%d)" % entry[1:]
    if entry[0] == "g6":
        what += "[stages=%d]" % entry[2]
    cid = "%s %s %dx%dx%d" % (what, "TN" if layout else "NN", M, N, K)
    return Case(family, cid, entry, layout, M, N, K, bm, bn, wtm, wtn, bk, scheduled, M * N * K > BIG_MNK)


# ---------------------------------------------------------------- VALU rungs, naive MFMA, 1-stage MFMA (csrc/hgemm_valu.cuh, hgemm_mfma.cuh)
# name -> (BK, TM) of its launch_valu_tile<BK, TM, dbuf, async>: one name per distinct instantiation (csrc/hgemm.hip CLN_G3 lines)
VALU_TILE_RUNGS = {
    "hgemm_t_8x8_sliced_k_f16x4": (8, 8), "hgemm_t_8x8_sliced_k_f16x8_pack_bcf_dbuf": (8, 8),
    "hgemm_t_8x8_sliced_k16_f16x8_pack_dbuf": (16, 8), "hgemm_t_8x8_sliced_k16_f16x8_pack_dbuf_async": (16, 8),
    "hgemm_t_8x8_sliced_k32_f16x8_pack_dbuf": (32, 8), "hgemm_t_8x8_sliced_k32_f16x8_pack_dbuf_async": (32, 8),
    "hgemm_t_16x8_sliced_k32_f16x8_pack_dbuf": (32, 16), "hgemm_t_16x8_sliced_k32_f16x8_pack_dbuf_async": (32, 16)}
# any-shape rungs: name -> (tile side, K step, K must divide by)
ANY_SHAPE_RUNGS = {"hgemm_naive_f16": (16, 16, 1), "hgemm_sliced_k_f16": (32, 32, 1), "hgemm_mma_m16n8k16_naive": (16, 16, 4)}
ANY_SHAPES = ((100, 100, 64), (9, 20, None))  # (None: one K step + 4 -- K ragged against the step, M below one tile, N one tile + 4)


def valu_cases():
    out, refused = [], []
    for name, (T, ks, kdiv) in ANY_SHAPE_RUNGS.items():
        fam = "naive_mfma" if "mma" in name else "valu"
        for (M, N, K) in ((T, T, ks), (2 * T, 3 * T, 2 * ks), (T, T, 3 * ks)) + tuple((m, n, k or ks + 4) for m, n, k in ANY_SHAPES):
            out.append(_case(fam, ("g3", name), NN, M, N, K, T, T, 16, 16, ks))
        if kdiv > 1:
            refused.append(Refused(fam, ("g3", name), NN, 16, 16, 18))  # launch_naive: K % 4
    for name, (BK, TM) in VALU_TILE_RUNGS.items():
        for (M, N, K) in ((128, 128, BK), (256, 384, 2 * BK), (128, 128, 3 * BK)):
            out.append(_case("valu", ("g3", name), NN, M, N, K, 128, 128, 4 * TM, 128, BK))
        refused += [Refused("valu", ("g3", name), NN, 100, 100, 64), Refused("valu", ("g3", name), NN, 128, 128, BK + 4),
                    Refused("valu", ("g3", name), NN, 64, 128, BK)]
    return out, refused


# 1-stage MFMA: name -> Cfg the launcher picks; launch_1stage_128_or_64 runs Cfg<64,64,64> below 256 tiles of 128 x 128 when M, N, K % 64 == 0
ONE_STAGE_64x128 = "hgemm_wmma_m16n16k16_mma4x2"
ONE_STAGE_SWITCH = ("hgemm_wmma_m16n16k16_mma4x2_warp2x4", "hgemm_mma_m16n8k16_mma2x4_warp4x4")


def one_stage_form(M, N, K):
    """Mirror of csrc/hgemm.hip launch_1stage_128_or_64: (BM, BN, BK) or None where the launcher refuses."""
    if (M // 128) * (N // 128) < 256 and M % 64 == 0 and N % 64 == 0 and K % 64 == 0:
        return (64, 64, 64)
    return (128, 128, 32) if M % 128 == 0 and N % 128 == 0 and K % 32 == 0 else None


def one_stage_cases():
    out = [_case("1stage", ("g3", ONE_STAGE_64x128), NN, M, N, K, 64, 128, 64, 64, 32) for (M, N, K) in ((64, 128, 32), (128, 384, 96))]
    refused = [Refused("1stage", ("g3", ONE_STAGE_64x128), NN, 64, 64, 32), Refused("1stage", ("g3", ONE_STAGE_64x128), NN, 64, 128, 48)]
    for name in ONE_STAGE_SWITCH:
        # Cfg<64,64,64>: one tile, 2 x 3 tiles of 3 BK; Cfg<128,128,32>: K % 64 != 0 (one tile of BK, 2 x 3 tiles of 3 BK);
        # the switch: 15 x 16 = 240 tiles of 128 x 128 -> 64 x 64 tiles, 16 x 16 = 256 -> 128 x 128 tiles
        for (M, N, K) in ((64, 64, 64), (128, 192, 192), (128, 128, 32), (256, 384, 96), (1920, 2048, 64), (2048, 2048, 64)):
            bm, bn, bk = one_stage_form(M, N, K)
            out.append(_case("1stage", ("g3", name), NN, M, N, K, bm, bn, bm // 2, bn // 2, bk))
        refused += [Refused("1stage", ("g3", name), NN, 64, 64, 32), Refused("1stage", ("g3", name), NN, 100, 100, 64)]
    return out, refused


# ---------------------------------------------------------------- rings (csrc/hgemm_ring_impl.inc ring_exact: Cfg<BM, BN, BK, WM, WN, S>)
RING_TILES = {0: (128, 128, 2, 2), 1: (256, 256, 2, 4), 2: (256, 128, 4, 2), 3: (128, 256, 2, 4), 6: (64, 128, 1, 4), 7: (64, 64, 2, 2),
              8: (64, 64, 1, 2)}  # tile id -> (BM, BN, waves along M, waves along N)
RING_BK_STAGES = [(bk, s) for bk in (64, 32) for s in (2, 3, 4, 5)]


def ring_fits(tile, bk, stages):
    BM, BN, _, _ = RING_TILES[tile]
    return stages * (BM + BN) * bk * 2 <= LDS_LIMIT


def ring_cases(tile, layout):
    """K = BK (fewer K tiles than stages), stages x BK exactly and one more tile; grids of 1 x 1 and 2 x 2 tiles. Returns (cases, instantiations
    that do not fit the LDS: the skips of test_every_ring_instantiation)."""
    BM, BN, WM, WN = RING_TILES[tile]
    out, skipped = [], []
    for bk, st in RING_BK_STAGES:
        if not ring_fits(tile, bk, st):
            skipped.append((tile, layout, bk, st))
            continue
        for g in (1, 2):
            for K in (bk, st * bk, (st + 1) * bk):
                out.append(_case("ring_t%d_%s" % (tile, "tn" if layout else "nn"), ("variant", 0, tile, bk, st), layout, g * BM, g * BN, K,
                                 BM, BN, BM // WM, BN // WN, bk))
    return out, skipped


# ---------------------------------------------------------------- ping-pong, hgemm_w4, hgemm_w4s through the probe hook and the fixed-tile names
PP_VARIANTS = ((3, 2), (5, 8), (5, 4), (8, 4), (9, 4))  # (kind, stages): plain / LDS epilogue 8 slots / 4 slots / split DMA / launch_pp32
PP_KS = (64, 128, 320)


def pingpong_cases():
    return [_case("pingpong", ("variant", kind, 1, 64, st), layout, 256, 256, K, 256, 256, 128, 64, 32 if kind == 9 else 64, True)
            for layout in (NN, TN) for kind, st in PP_VARIANTS for K in PP_KS]


W4_KIND15 = {0: (192, 256), 1: (256, 192), 2: (192, 192), 3: (128, 256), 4: (256, 128), 5: (160, 160)}
W4_KS = (384, 448, 640)  # smallest even count of K tiles, smallest odd, one loop pair more
W4_FIXED = ((FIXED_256x256, NN, 256, 256), (FIXED_256x128, NN, 256, 128), (FIXED_128x256, TN, 128, 256))


def w4_k_ok(K):
    """csrc/hgemm_w4.cuh w4_k_ok."""
    return K % 64 == 0 and K >= (448 if (K // 64) & 1 else 384)


def w4_cases():
    out, refused = [], []
    for layout in (NN, TN):
        for tile, (BM, BN) in W4_KIND15.items():
            for (gm, gn) in ((1, 1), (2, 3)):
                for K in W4_KS:
                    out.append(_case("w4", ("variant", 15, tile, 64, 2), layout, gm * BM, gn * BN, K, BM, BN, BM // 2, BN // 2, 64, True))
            refused.append(Refused("w4", ("variant", 15, tile, 64, 2), layout, BM, BN, 320))
    for name, layout, BM, BN in W4_FIXED:
        for (gm, gn) in ((1, 1), (2, 3)):
            for K in W4_KS:
                out.append(_case("w4", ("g6", name, 2), layout, gm * BM, gn * BN, K, BM, BN, BM // 2, BN // 2, 64, True))
    return out, refused


def w4s_k_ok(K, S):
    """csrc/hgemm_w4s.cuh w4s_k_ok."""
    return K % 64 == 0 and K // 32 >= 2 * S


def w4s_cases():
    out, refused = [], []
    for layout in (NN, TN):
        for S in (2, 3, 4, 5):
            K0 = 64 * S  # the smallest legal K: 2 S slots of 32
            out.append(_case("w4s", ("variant", 16, 0, 32, S), layout, 256, 256, K0, 256, 256, 128, 128, 32, True))
            out.append(_case("w4s", ("variant", 16, 0, 32, S), layout, 512, 512, K0 + 64, 256, 256, 128, 128, 32, True))
            refused.append(Refused("w4s", ("variant", 16, 0, 32, S), layout, 256, 256, K0 - 64))
    for S in (3, 4, 5):  # through the 256 x 256 fixed-tile name: stages 3 / 4 / 5
        out.append(_case("w4s", ("g6", FIXED_256x256, S), NN, 256, 256, 64 * S, 256, 256, 128, 128, 32, True))
        out.append(_case("w4s", ("g6", FIXED_256x256, S), NN, 512, 256, 64 * S + 64, 256, 256, 128, 128, 32, True))
    return out, refused


# ---------------------------------------------------------------- the run-time dispatched names: shapes by search over manifest.describe
def family_of(text):
    """The kernel family of a manifest.describe text."""
    if "tail split" in text:
        return "tail_split,%s" % ("fixup" if "in-kernel fix-up" in text else "reduce")
    tile = re.match(r"\w+<(\d+x\d+)", text)
    if "split-K x" in text:
        return "splitk<%s>,%s" % (tile.group(1), "fixup" if "in-kernel fix-up" in text else "reduce")
    if text.startswith("hgemm_w4s<"):
        return "hgemm_w4s<256x256,ring of %s" % re.search(r"ring of (\d)", text).group(1)
    if text.startswith("hgemm_pp32<"):
        return "hgemm_pp32"
    kernel = text.split("<")[0]
    assert kernel in ("hgemm_w4", "hgemm_pp", "mfma_ring"), text
    return "%s<%s" % (kernel, tile.group(1))


SPLITK_TILES = ("256x256", "192x256", "192x192", "128x256", "160x160")  # csrc/hgemm.hip splitk_plan shapes[]
W4_TILES = ("256x256", "192x256", "256x192", "192x192", "128x256", "256x128", "160x160")
# every family describe_best / describe_ring / describe_w4 can name. mfma_ring: plan_tile gives 128x256, 64x128, 64x64, 128x128 and (the 256 x 256
# plan at stages 3 / 5 with K too short for hgemm_w4s) 256x256; 256x128 only through its fixed-tile name.
SINGLE_PASS_FAMILIES = (["mfma_ring<%s" % t for t in ("64x64", "64x128", "128x128", "128x256", "256x256", "256x128")]
                        + ["hgemm_pp<192x256", "hgemm_pp<256x256", "hgemm_pp32"] + ["hgemm_w4<%s" % t for t in W4_TILES]
                        + ["hgemm_w4s<256x256,ring of %d" % s for s in (3, 4, 5)])
DISPATCHED_FAMILIES = [f for f in SINGLE_PASS_FAMILIES if f != "hgemm_w4<256x128"]
TAIL_FAMILIES = ["tail_split,fixup", "tail_split,reduce"]
# families the top rungs never pick below 4608: reached through the name that fixes the tile (describe kinds 0 and 2): name, layout
ONLY_BY_FIXED_NAME = {"mfma_ring<256x128": (FIXED_256x128, NN),  # (hgemm_w4<256x128: w4_cases lists it through the same name)
                      "mfma_ring<128x128": ("hgemm_mma_m16n8k16_mma2x4_warp4x4_stages_dsmem", NN)}
RING_128_TN = "hgemm_mma_m16n8k16_mma2x4_warp4x4_stages_dsmem_tn"
SEARCH_MAX = 4608
SEARCH_KS = (32, 64, 96, 128, 320, 384, 448, 640)
SPLITK_KS = tuple(range(4096, 8257, 64))
TAIL_KS = tuple(range(768, 4097, 64))


def _try_describe(manifest, name, dims, stages):
    try:
        return manifest.describe(name, dims, stages)
    except ValueError:
        return None


@functools.lru_cache(maxsize=None)
def _search(manifest):
    """family -> sorted list of (M * N * K, M, N, K, stages, name, layout) candidates found (the smallest few per family and K)."""
    best = {}

    def offer(fam, M, N, K, st, name, layout, slot):
        key = (fam, slot)
        cand = (M * N * K, M, N, K, st, name, layout)
        if key not in best or cand < best[key]:
            best[key] = cand

    steps = range(64, SEARCH_MAX + 1, 64)
    for K in SEARCH_KS:
        for st in (2, 3, 4, 5):
            for M in steps:
                for N in steps:
                    t = _try_describe(manifest, BEST_NN, (M, N, K), st)
                    if t is not None and "split-K" not in t and "tail split" not in t:
                        offer(family_of(t), M, N, K, st, BEST_NN, NN, K)
    for fam, (name, layout) in ONLY_BY_FIXED_NAME.items():
        BM, BN = (int(x) for x in fam.split("<")[1].split("x"))
        for K in SEARCH_KS:
            for st in (2, 3):
                t = _try_describe(manifest, name, (BM, BN, K), st)
                if t is not None and family_of(t) == fam:
                    offer(fam, BM, BN, K, st, name, layout, K)
    for K in SPLITK_KS:
        for M in steps:
            for N in steps:
                if M * N > 2048 * 2048:
                    break
                t = _try_describe(manifest, BEST_NN, (M, N, K), 2)
                if t is None or "split-K x" not in t or "tail split" in t:
                    continue
                S = int(re.search(r"split-K x (\d+)", t).group(1))
                odd = (K // S // 64) & 1
                # even count: K = 4096 where the family exists there, else its smallest K; odd count: its smallest K
                offer(family_of(t), M, N, K, 2, BEST_NN, NN, "odd" if odd else ("4096" if K == 4096 else "even"))
    for K in TAIL_KS:
        for M in range(256, SEARCH_MAX + 513, 256):
            for N in range(256, SEARCH_MAX + 513, 256):
                t = _try_describe(manifest, BEST_NN, (M, N, K), 2)
                if t is not None and "tail split" in t:
                    offer(family_of(t), M, N, K, 2, BEST_NN, NN, "tail")
    out = {}
    for (fam, slot), cand in best.items():
        out.setdefault(fam, {})[slot] = cand
    return out


def _geometry(fam):
    if fam.startswith("tail_split"):
        return 256, 256, 128, 128, 64
    if fam == "hgemm_pp32":
        return 256, 256, 128, 64, 32
    BM, BN = (int(x) for x in re.search(r"<(\d+)x(\d+)", fam).groups())
    if fam.startswith(("hgemm_w4", "splitk")):
        return BM, BN, BM // 2, BN // 2, 32 if fam.startswith("hgemm_w4s") else 64
    if fam.startswith("hgemm_pp"):
        return BM, BN, BM // 2, BN // 4, 64
    for (bm, bn, wm, wn) in RING_TILES.values():
        if (bm, bn) == (BM, BN):
            return BM, BN, BM // wm, BN // wn, 32
    raise AssertionError(fam)


def dispatched_cases(manifest):
    """Cases of the single-pass families through the run-time dispatched names: per family the smallest shape the search found at up to three K of
    SEARCH_KS (the smallest, the largest and one between), NN and TN (the planner does not look at the layout)."""
    found = _search(manifest)
    out = []
    for fam in DISPATCHED_FAMILIES:
        slots = found.get(fam, {})
        ks = sorted(k for k in slots if isinstance(k, int))
        for K in sorted(set(ks[:1] + ks[len(ks) // 2:len(ks) // 2 + 1] + ks[-1:])):
            _, M, N, _, st, name, layout = slots[K]
            bm, bn, wtm, wtn, bk = _geometry(fam)
            sched = not fam.startswith("mfma_ring")
            out.append(_case("dispatched", ("g6", name, st), layout, M, N, K, bm, bn, wtm, wtn, bk, sched))
            if name == BEST_NN:
                out.append(_case("dispatched", ("g6", BEST_TN, st), TN, M, N, K, bm, bn, wtm, wtn, bk, sched))
            elif fam == "mfma_ring<128x128":
                out.append(_case("dispatched", ("g6", RING_128_TN, st), TN, M, N, K, bm, bn, wtm, wtn, bk, sched))
    return out


def splitk_cases(manifest):
    """Per (tile, form): K = 4096 (or, where the plan has that family only above it, its smallest K) and the smallest K with an odd count of K
    tiles per split, each at the smallest M x N; NN, and TN at the odd one."""
    found = _search(manifest)
    out = []
    for fam in sorted(f for f in found if f.startswith("splitk<")):
        slots = found[fam]
        even = slots.get("4096") or slots.get("even")
        for cand, both in ((even, False), (slots.get("odd"), True)):
            if cand is None:
                continue
            _, M, N, K, st, name, layout = cand
            bm, bn, wtm, wtn, bk = _geometry(fam)
            out.append(_case("splitk", ("g6", BEST_NN, 2), NN, M, N, K, bm, bn, wtm, wtn, bk, True))
            if both:
                out.append(_case("splitk", ("g6", BEST_TN, 2), TN, M, N, K, bm, bn, wtm, wtn, bk, True))
    return out


def tail_cases(manifest):
    found = _search(manifest)
    out = []
    for fam in TAIL_FAMILIES:
        cand = found.get(fam, {}).get("tail")
        if cand is None:
            continue
        _, M, N, K, st, name, layout = cand
        out.append(_case("tail", ("g6", BEST_NN, 2), NN, M, N, K, 256, 256, 128, 128, 64, True))
        out.append(_case("tail", ("g6", BEST_TN, 2), TN, M, N, K, 256, 256, 128, 128, 64, True))
    return out


def tail_m_split(text):
    return int(re.search(r"on rows \[0, (\d+)\)", text).group(1))


def vendor_cases():
    """rocBLAS rows: guard bands and the tolerance of tests/test_gpu_hgemm.py only."""
    return [_case("vendor", ("vendor", name), layout, M, N, K, M, N, M, N, K)
            for name, layout in (("hgemm_cublas_tensor_op_nn", NN), ("hgemm_cublas_tensor_op_tn", TN)) for (M, N, K) in ((256, 384, 512), (104, 72, 40))]


RING_FAMILIES = ["ring_t%d_%s" % (t, l) for t in RING_TILES for l in ("nn", "tn")]
FAMILIES = ["valu", "naive_mfma", "1stage"] + RING_FAMILIES + ["pingpong", "w4", "w4s", "dispatched", "splitk", "tail", "vendor"]


@functools.lru_cache(maxsize=None)
def table(manifest):
    """{"cases": family -> [Case], "refused": [Refused], "lds_skips": [(tile, layout, bk, stages)]} -- the whole table."""
    cases, refused, skips = {f: [] for f in FAMILIES}, [], []

    def add(cs, rf=()):
        for c in cs:
            cases[c.family].append(c)
        refused.extend(rf)

    add(*valu_cases())
    add(*one_stage_cases())
    for tile in RING_TILES:
        for layout in (NN, TN):
            cs, sk = ring_cases(tile, layout)
            add(cs)
            skips += sk
    add(pingpong_cases())
    add(*w4_cases())
    add(*w4s_cases())
    add(dispatched_cases(manifest))
    add(splitk_cases(manifest))
    add(tail_cases(manifest))
    add(vendor_cases())
    return {"cases": cases, "refused": refused, "lds_skips": skips}


def case_count(manifest):
    return sum(len(v) for v in table(manifest)["cases"].values())


def expected_family(case, manifest):
    """The family manifest.describe names for a case called through a run-time dispatched name (None for the other entries)."""
    if case.entry[0] != "g6":
        return None
    try:
        return family_of(manifest.describe(case.entry[1], (case.M, case.N, case.K), case.entry[2]))
    except LookupError:
        return None


# ---------------------------------------------------------------- exact inputs
def magnitude(K):
    """Operands are integers in [-r, r]. The mean of |x| is about r / 2, so a row of A that carries the sign pattern of a column of B sums to about
    K r^2 / 4: r is sized so that this is about 12000 below K = 4096 (past 2048: a half result there is a rounded one; K r^2 <= 4 x 12000 + slack
    stays below 65520) and about 80000 from K = 4096 on (past 65520: +-inf; the half-aligned rows, about 40000, stay finite)."""
    target = 80000.0 if K >= 4096 else 12000.0
    return max(2, min(120, int(round(2.0 * (target / K) ** 0.5))))


def rounding_possible(K):
    """Whether a tenth of the outputs can be rounded ones at all: K r^2 (the largest sum) must pass 2048 with room; it does for every K >= 4 at
    the magnitudes above. (K < 4 would not: no case has one.)"""
    return K * magnitude(K) ** 2 > 4 * 2048


@functools.lru_cache(maxsize=64)
def exact_inputs(M, N, K, seed=0):
    """(a int16 [M, K], b int16 [K, N]) of integers in [-r, r], r = magnitude(K). Columns of B with n % 2 == 1 carry one sign pattern s[k]
    (b = |b| s). Rows of A with m % 4 == 1 carry it over all of K (sums about +K r^2 / 4; rows m % 8 == 5 negated: about -K r^2 / 4), rows with
    m % 4 == 3 over the first half of K only (about half of that). K r^2 < 2^24 for every K used, so every partial sum of every order and split is
    an integer that fp32 holds; tests/test_hgemm_reference.py holds abs_sum_bound below 2^24 case by case."""
    r = magnitude(K)
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * K + 31 * M + N)
    a = torch.randint(-r, r + 1, (M, K), generator=g, dtype=torch.int16)
    b = torch.randint(-r, r + 1, (K, N), generator=g, dtype=torch.int16)
    s = torch.randint(0, 2, (K,), generator=g, dtype=torch.int16) * 2 - 1
    b[:, 1::2] = b[:, 1::2].abs() * s.view(K, 1)
    a[1::4] = a[1::4].abs() * s.view(1, K)
    a[5::8] = -a[5::8]
    h = (K + 1) // 2
    a[3::4, :h] = a[3::4, :h].abs() * s[:h].view(1, h)
    return a, b


def int_product(a, b):
    """The exact integer product as int64. Taken in float64 (BLAS; on the device for the large cases): every partial sum is an integer below 2^24,
    so float64 holds it in any order -- tests/test_hgemm_reference.py pins it to the int64 matmul."""
    return (a.double() @ b.double()).to(torch.int64)


def abs_sum_bound(a, b):
    """ix.abs_sum_bound (int64) for small operands; the same quantity in float64 (exact below 2^53) for large ones, where the int64 matmul of the
    CPU takes seconds."""
    if a.shape[0] * a.shape[1] * b.shape[1] <= (1 << 24):
        return ix.abs_sum_bound(a, b)
    return int((a.abs().double() @ b.abs().double()).max())


def expected_exact(a, b):
    """half_rne of the integer product (+-inf from 65520 on)."""
    return half_rne(int_product(a, b))


def rounded_share(prod):
    """Share of outputs that are not representable in half before rounding (integers: |v| >= 2048 and not on the grid; |v| >= 65520 counts too)."""
    v = prod.double()
    back = v.to(torch.float16).double()
    return float((back != v).double().mean())


# ---------------------------------------------------------------- poison plan
def _edges(n, wt, bt):
    return sorted(set(i for i in (0, 15, 16, wt - 1, wt, bt - 1, bt, n - 1) if 0 <= i < n))


def poison_ks(case):
    """k positions: the first and last element of the first, a middle and the last K tile (of the case's K step and of a 32-deep slot), plus K - 1."""
    K, ks = case.K, set()
    for step in {min(case.bk, K), min(32, K)}:
        nt = (K + step - 1) // step
        for t in {0, nt // 2, nt - 1}:
            ks.update((t * step, min(K - 1, t * step + step - 1)))
    ks.add(K - 1)
    return sorted(ks)


def poison_plan(case):
    """(rows: [(m, k)], cols: [(n, k)]): row m of A gets one NaN at column k, column n of B one NaN at row k. Rows / columns sit at fragment, wave-tile
    and block-tile edges (0, 15, 16, WTM - 1, WTM, BM - 1, BM, M - 1; the same for N); the k values cycle through poison_ks, the columns going on
    where the rows stopped, so that rows and columns together use every k at least once where there are enough of them."""
    ks = poison_ks(case)
    rows = [(m, ks[i % len(ks)]) for i, m in enumerate(_edges(case.M, case.wtm, case.bm))]
    cols = [(n, ks[(len(rows) + i) % len(ks)]) for i, n in enumerate(_edges(case.N, case.wtn, case.bn))]
    return rows, cols


def poison_mask(case):
    rows, cols = poison_plan(case)
    mask = torch.zeros(case.M, case.N, dtype=torch.bool)
    mask[[m for m, _ in rows]] = True
    mask[:, [n for n, _ in cols]] = True
    return mask


# ---------------------------------------------------------------- special values
SPECIAL_ROW_KINDS = 8


def special_inputs(case):
    """(a half [M, K], b half [K, N], expected float64 [M, N] with NaN / inf). A and B are zero except on five k positions (first, last, the two
    middle ones, the second); row m of A is of kind m % 8:
      0  2^-24 (subnormal) x B[ka] = 2^(10 + n % 3) ...                   -> normal results 2^-14 ... 2^-12; 0 where B[ka] is 0 (n % 4 == 3)
      1  2^14 x B[kc] = (n % 7 + 1) 2^-24 (subnormal)                     -> normal / subnormal-free results (n % 7 + 1) 2^-10
      2  2^-10 x B[kb] = (n % 5 + 1) 2^-10                                -> subnormal half results (n % 5 + 1) 2^-20
      3  1 x 32752 + 2047 x 16                                            -> exactly 65504, the largest finite half
      4  2 x 32752 + 1 x 16                                               -> 65520, the tie: +inf
      5  -2 x 32752 - 1 x 16                                              -> -inf
      6  -2^-24 x B[ka] + 2^-10 x B[kb]                                   -> a normal and a subnormal term, exact
      7  +inf x B[ka]                                                     -> +inf against a nonzero, NaN against a zero (n % 4 == 3)
    The expected values are the float64 sum of the five outer products; the builder asserts every finite one is a half exactly (65520 excepted: the
    tie), so no second rounding enters the reference."""
    M, N, K = case.M, case.N, case.K
    assert K >= 8
    ka, kb, kc, kd, ke = 0, K - 1, K // 2, K // 2 - 1, 1
    n = torch.arange(N)
    b = torch.zeros(K, N, dtype=torch.float64)
    b[ka] = torch.where(n % 4 == 3, torch.zeros(N, dtype=torch.float64), 2.0 ** (10 + n % 3).double())
    b[kb] = (n % 5 + 1).double() * 2.0 ** -10
    b[kc] = (n % 7 + 1).double() * 2.0 ** -24
    b[kd] = 32752.0
    b[ke] = 16.0
    a = torch.zeros(M, K, dtype=torch.float64)
    kind = torch.arange(M) % SPECIAL_ROW_KINDS
    inf = float("inf")
    for k_, col in ((ka, {0: 2.0 ** -24, 6: -2.0 ** -24, 7: inf}), (kb, {2: 2.0 ** -10, 6: 2.0 ** -10}), (kc, {1: 2.0 ** 14}),
                    (kd, {3: 1.0, 4: 2.0, 5: -2.0}), (ke, {3: 2047.0, 4: 1.0, 5: -1.0})):
        for kd_, v in col.items():
            a[kind == kd_, k_] = v
    ah, bh = a.to(torch.float16), b.to(torch.float16)
    assert torch.equal(ah.double(), a) and torch.equal(bh.double(), b)  # the inputs are halves exactly
    want = torch.zeros(M, N, dtype=torch.float64)
    for k_ in (ka, kb, kc, kd, ke):
        want = want + a[:, k_:k_ + 1] * b[k_:k_ + 1, :]
    tie = want.abs() == 65520.0
    want = torch.where(tie, torch.sign(want) * inf, want)
    fin = torch.isfinite(want)
    assert torch.equal(want[fin].to(torch.float16).double(), want[fin]) and float(want[fin].abs().max()) <= 65504.0
    return ah, bh, want


def same_with_nan(got, want):
    """Equality with NaN compared by position (got, want: same dtype)."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool(torch.equal(gn, wn)) and bool(torch.equal(torch.where(gn, torch.zeros_like(got), got), torch.where(wn, torch.zeros_like(want), want)))


def sample_rows(M, seam=None):
    """Rows on which a device float64 product is pinned to the CPU's int64 product: the first, the last, and both sides of a split seam."""
    rows = {0, M - 1, M // 2}
    if seam is not None:
        rows |= {seam - 1, seam}
    return sorted(r for r in rows if 0 <= r < M)
