"""The cases of the exact visible-key tests of the sixteen bf16 paged attention entries (tests/test_paged_edge_cases.py on the CPU,
tests/test_gpu_paged_edge_counts.py on the GPU): which keys a row sees, as an interval of integers, at every length and window
at which the kernels have structure -- 16 (an MFMA key block), 32 (a wave's keys), 64 (the prefill's key step), 128 (the decode's key step and
the prefill's row tile), the page, the split chunk C and the base of a windowed split.

Row t of the T new tokens of a sequence of `len` keys (clamped to [0, Nmax] as the entries clamp it) stands at p = len - T + t and sees the keys
max(0, p - W + 1) ... p; p < 0: none. `visible` is that sentence, and with `defect` one of the ways a kernel can get it wrong (DEFECTS).

Why the randn parity tests cannot stand in for this: a row that sees n keys of unit-variance scores moves its LSE by about 1 / n for one key
more or less, and decode_reference.lse_tol is 2^-10 max(1, |LSE|), 5e-3 to 9e-3 in the existing cases. The two criteria here have no such floor:
    counting   q = 0, V = a constant c: every score is exactly 0 whatever scale, cap and k_scale are, so LSE = ln n (ln(n + 1) with a sink of 0)
               and O = c (c n / (n + 1)). LSE is held to 1 / (4 (n + 1)), a quarter of ln(n + 1) - ln n: it separates n from n +- 1. O = c bit
               for bit: every P is 1, l is the integer n, the P V sums are c n, exact in fp32 in any order, the splits merge with factors
               exp2(0) = 1, and c n / n rounds to the bf16 c whether the kernel divides or multiplies by a reciprocal (the fp32 error, 1e-7
               relative, is far below half a bf16 ulp of a value that IS a bf16 number). The several-splits table therefore needs no fallback
               to "one bf16 ulp": it is held bit for bit like the others.
    identity   keys = the +-1 binary code of their position, q = 16 x the code of a target: O = V[target] bit for bit, |LSE - score| <=
               1e-5 score (the rule of the fp16 one-hot test); ONEHOT_MARGIN nats between the target and every other key, asserted here.
No other tolerance is defined; the hidden-target runs of the identity test use the families' fp64 references and their check().

Largest LSE err / bound seen on an MI355X over all sixteen entries at D = 64 and 128 (tests/test_gpu_paged_edge_counts.py, pytest -s; also in
RATIOS_SEEN below and DESIGN 4.4.15): decode with one split 0.0009 (664464 rows; 0.0011 with a sink of 0), decode with several splits 0.0021
(0.0021), packed prefill 0.0024 (0.0024): a few fp32 ulps of ln n at n = 1024 against a bound of 2.4e-4. O was the bits of c on every row of
every table, the several-splits table included; every identity row returned the bits of its V row. No kernel was found wrong.

A plain module: nothing here is collected. The tables are built from the entries' own *_plan functions (cuda_learn_notes_amd, no GPU needed) and
the kernels' constants as the reference modules hold them; no length is written down by hand."""
import collections
import functools
import math

import torch

import decode_reference as dr
import multi_decode_reference as mr
import paged_all_entries as ae
import paged_bf16_fp8_reference as fr
import paged_decode_reference as pr
import paged_window_reference as wr
import prefill_reference as pf

BF = torch.bfloat16
INT_MAX = wr.INT_MAX
NEG_INF = float("-inf")
BLOCK16, WAVE_KEYS, PREFILL_STEP, DECODE_STEP, ROW_TILE = mr.TILE_ROWS, 32, pf.KEY_STEP, mr.KEY_STEP, pf.ROW_TILE
DS = [64, 128]
PAGES = [16, 64, 256]
C_VALUE = 0.375               # exact in bf16, and in e4m3 under the power-of-two v_scales of paged_bf16_fp8_reference.scales(pow2=True)
ONEHOT_MARGIN = 20.0
ONEHOT_WINDOWS = [17, 128, None]

# what one MI355X run of tests/test_gpu_paged_edge_counts.py printed as the largest LSE err / bound (bound = 1 / (4 (n + 1))) per table
RATIOS_SEEN = {("one", False): 0.0009, ("one", True): 0.0011, ("split", False): 0.0021, ("split", True): 0.0021, ("prefill", False): 0.0024,
               ("prefill", True): 0.0024}

ENTRIES = [e for e in ae.ATTN if e.bf16]
assert len(ENTRIES) == 16
DEFECTS = ("causal_plus_one", "causal_minus_one", "window_plus_one", "window_minus_one", "drop_first_key_of_chunk", "double_count_chunk_boundary",
           "drop_last_partial_block16", "window_start_rounded_to_unit", "len_not_clamped")
WINDOW_DEFECTS = ("window_plus_one", "window_minus_one", "window_start_rounded_to_unit")
CHUNK_DEFECTS = ("drop_first_key_of_chunk", "double_count_chunk_boundary")

Vis = collections.namedtuple("Vis", "lo hi n")  # the keys lo ... hi, n of them (with a defect: the n that defect would count); empty: (0, -1, 0)


def unit(page):
    return max(page, DECODE_STEP)


def base_of(length, T, W, page):
    """Where the first split of a windowed decode starts: align_down(max(0, len - T - W + 1), max(page, 128)); 0 without a window."""
    return 0 if W is None else max(0, length - T - W + 1) // unit(page) * unit(page)


def visible(length, T, t, W, Nmax, defect=None, page=16, C=None):
    """Vis(lo, hi, n) of row t of T new tokens. W = None: no window. page and C (the split chunk) only matter to the defects that name them."""
    L = max(int(length), 0)
    if defect != "len_not_clamped":
        L = min(L, Nmax)
    p = L - T + t
    hi = p + (defect == "causal_plus_one") - (defect == "causal_minus_one")
    lo = 0
    if W is not None:
        lo = max(0, p - (W + (defect == "window_plus_one") - (defect == "window_minus_one")) + 1)
    if defect == "window_start_rounded_to_unit" and W is not None:
        lo = lo // unit(page) * unit(page)
    if hi < 0 or hi < lo:
        return Vis(0, -1, 0)
    n = hi - lo + 1
    if defect in CHUNK_DEFECTS and C:
        b = base_of(L, T, W, page)
        at = sum(1 for j in range(b + C, hi + 1, C) if j >= lo)  # the first keys of the later chunks that the row sees
        n += at if defect == "double_count_chunk_boundary" else -at
    if defect == "drop_last_partial_block16" and L % BLOCK16:
        n -= max(0, hi - max(lo, L // BLOCK16 * BLOCK16) + 1)
    return Vis(lo, hi, n)


def applies(defect, case):
    """Whether a defect can show in a case at all."""
    if defect in WINDOW_DEFECTS:
        return case.W is not None
    if defect in CHUNK_DEFECTS:
        return case.table == "split"
    return True


# ---------------------------------------------------------------------------------------------------- the entries

def kind(e):
    return "prefill" if e.form == "varlen" else "decode"


def plan_of(e, B, T, Hq, Hkv, max_pages, page, D, W):
    """(splits, chunk, workspace_bytes) from the decode entry's own *_plan."""
    fn = getattr(ae.pkg(), e.name + "_plan")
    if not e.window:
        return fn(B, T, Hq, Hkv, max_pages, page, D)
    return fn(B, T, Hq, Hkv, max_pages, page, D, INT_MAX if W is None and not e.sink else W)


def tg_choices(e):
    """(T, G) of the decode tables: the any-G entries take all six of the list, the others the powers of two among them and a pair of their own."""
    return [(1, 1), (1, 16), (3, 5), (8, 8), (8, 7), (4, 16)] if e.anyg else [(1, 1), (8, 8), (3, 4)]


def windows(e, page):
    """The W of an entry's tables at a page size: None alone for the two entries without a window."""
    if not e.window:
        return [None]
    return sorted({1, 2, 15, 16, 17, 127, 128, 129, page - 1, page + 1}) + [None]


def softcap_configs(e, D):
    """(softmax_scale, softcap) pairs the counting test runs a soft-cap entry with -- every score is 0, so the bits must agree --; () else."""
    return [(None, None), (1.0 / math.sqrt(1.3 * D), 2.0)] if e.softcap else [()]


def onehot_scale(e, D):
    """The identity test's (softmax_scale, softcap) of a soft-cap entry: a power of two above the default, so the one-hot margin grows."""
    return (0.25 if D == 64 else 0.125, None) if e.softcap else ()


# ---------------------------------------------------------------------------------------------------- the tables

# table: "one" | "split" | "prefill". T: the decode's T, or None for a prefill case whose Ts holds T_b per sequence. S, C: the entry's plan.
Case = collections.namedtuple("Case", "table page T G Hkv Nmax W lens Ts S C")
RS = lambda page: sorted({BLOCK16, WAVE_KEYS, PREFILL_STEP, DECODE_STEP, page, 2 * DECODE_STEP})  # noqa: E731
PREFILL_RS = lambda page: sorted({BLOCK16, PREFILL_STEP, page, ROW_TILE})  # noqa: E731
ONE_B_GUESS, ONE_LIMIT = 64, 2 * (2 * DECODE_STEP + 8) + 16  # room for 2 x 128 + 1 + T + W with W up to 257


def _one_nmax(e, T, G, page, D, W):
    """The largest Nmax <= ONE_LIMIT (a multiple of the page) that the entry's plan does not split."""
    for mp in range(ONE_LIMIT // page, 0, -1):
        if plan_of(e, ONE_B_GUESS, T, G, 1, mp, page, D, W)[0] == 1:
            return mp * page
    raise AssertionError((e.name, T, G, page, D, W))


def _one_lens(T, W, page, Nmax):
    want = {0, 1, T - 1, T, Nmax, Nmax + 3, -2}
    edges = [r + d for r in RS(page) for d in (-1, 0, 1)]
    for x in edges:
        want |= {x, x + T}                       # len and len - T at the edge
    if W is not None:
        for x in [-1, 0, 1] + edges:
            want |= {x + W - 1 + T, x + W}       # the lower edge p - W + 1 of the first and of the last row at the edge
    return sorted(n for n in want if -2 <= n <= Nmax or n == Nmax + 3)


@functools.lru_cache(maxsize=None)
def decode_one_cases(name, D):
    e = ae.BY_NAME[name]
    out, i = [], 0
    for page in PAGES:
        for W in windows(e, page):
            T, G = tg_choices(e)[i % len(tg_choices(e))]
            i += 1
            Nmax = _one_nmax(e, T, G, page, D, W)
            lens = _one_lens(T, W, page, Nmax)
            S, C, _ = plan_of(e, len(lens), T, G, 1, Nmax // page, page, D, W)
            out.append(Case("one", page, T, G, 1, Nmax, W, tuple(lens), None, S, C))
    return out


def _split_nmax(e, T, G, page, D, want_splits=4):
    """The smallest Nmax at which the entry's plan has at least four splits for a small batch."""
    U = unit(page)
    for Nmax in range(U, 64 * U + 1, U):
        if plan_of(e, 24, T, G, 1, Nmax // page, page, D, None)[0] >= want_splits:
            return Nmax
    raise AssertionError((e.name, page, D))


def _split_window(e, T, G, page, D, Nmax):
    """The smallest window (a unit and a bit, so that no edge is aligned by construction) whose span plan splits and leaves room below Nmax."""
    U = unit(page)
    for W in range(U + 44, Nmax - U, 64):
        if plan_of(e, 24, T, G, 1, Nmax // page, page, D, W)[0] > 1:
            return W
    raise AssertionError((e.name, page, D, Nmax))


def _split_lens(T, W, page, Nmax, S, C):
    """The first length of every kind: len - base at k C - 1, k C, k C + 1 for k = 1, 2, S - 1, S; the lower edge of the first row at a chunk
    boundary - 1, + 0, + 1 (with a window); a length that leaves the last splits empty; a length past Nmax."""
    found = {}
    for n in range(1, Nmax + 1):
        b = base_of(n, T, W, page)
        for k in {1, 2, S - 1, S}:
            for d in (-1, 0, 1):
                if n - b == k * C + d:
                    found.setdefault(("hi", k, d), n)
                if n - T - b == k * C + d:
                    found.setdefault(("hi first", k, d), n)
        if W is not None and n - T - W + 1 >= 0:
            rel = (n - T - W + 1 - b) % C
            if rel in (C - 1, 0, 1) and b > 0:
                found.setdefault(("lo", rel), n)
    lens = set(found.values()) | {C // 2 + 3, Nmax + 5, 0}
    return sorted(lens)


@functools.lru_cache(maxsize=None)
def decode_split_cases(name, D):
    e = ae.BY_NAME[name]
    out = []
    tgs = [tg for tg in tg_choices(e) if tg[0] * tg[1] > 1][:2] + [tg_choices(e)[0]]
    i = 0
    for page in (PAGES[0], PAGES[-1]):
        for windowed in ([False, True] if e.window else [False]):
            T, G = tgs[i % len(tgs)]
            i += 1
            Nmax = _split_nmax(e, T, G, page, D)
            W = _split_window(e, T, G, page, D, Nmax) if windowed else None
            S, C, _ = plan_of(e, 24, T, G, 1, Nmax // page, page, D, W)
            lens = _split_lens(T, W, page, Nmax, S, C)
            S2, C2, _ = plan_of(e, len(lens), T, G, 1, Nmax // page, page, D, W)
            assert (S2, C2) == (S, C), (name, page, W)
            out.append(Case("split", page, T, G, 1, Nmax, W, tuple(lens), None, S, C))
    return out


def prefill_groups(e):
    return [3, 7, 12] if e.anyg else [8, 4, 1]


def _prefill_ts(G):
    """T_b with T_b G below, at (where G divides 128) and above the row tile, and two short ones."""
    ts = {(ROW_TILE - 1) // G, -(-ROW_TILE // G), ROW_TILE // G + 1, 1, 5}
    return sorted(t for t in ts if t >= 1)


@functools.lru_cache(maxsize=None)
def prefill_cases(name, D):
    e = ae.BY_NAME[name]
    out, i = [], 0
    for page in PAGES:
        Nmax = -(-(2 * ROW_TILE + page + 64) // page) * page
        for W in windows(e, page):
            G = prefill_groups(e)[i % 3]
            i += 1
            ts = _prefill_ts(G)
            lens, Ts, j = [], [], 0
            for r in PREFILL_RS(page):
                for d in (-1, 0, 1):
                    T = ts[j % len(ts)]
                    j += 1
                    lens.append(r + d + T), Ts.append(T)            # the first new token's upper edge p = len - T at the edge
                    T = ts[j % len(ts)]
                    j += 1
                    if r + d + 1 >= T:
                        lens.append(r + d + 1), Ts.append(T)        # the last new token's upper edge p = len - 1 at the edge
            lens += [0, 2, Nmax + 7, 9 + W if W is not None else 40]   # an empty sequence, len < T, a length past Nmax, rows behind a full window
            Ts += [0, 5, ts[-1], 9]
            out.append(Case("prefill", page, None, G, 1, Nmax, W, tuple(lens), tuple(Ts), 1, 0))
    return out


TABLES = {"one": decode_one_cases, "split": decode_split_cases, "prefill": prefill_cases}


def tables_of(e):
    return ["prefill"] if kind(e) == "prefill" else ["one", "split"]


def rows_of(case):
    """[(b, t, T_b)] of every row of a case, in the order the outputs hold them."""
    return [(b, t, T) for b, T in enumerate(case.Ts if case.T is None else [case.T] * len(case.lens)) for t in range(T)]


def counts(case, defect=None):
    """[Vis] per row of rows_of(case)."""
    return [visible(case.lens[b], T, t, case.W, case.Nmax, defect, case.page, case.C) for b, t, T in rows_of(case)]


def cu_of(case, first=0):
    cu = [first]
    for T in case.Ts:
        cu.append(cu[-1] + T)
    return cu


# ---------------------------------------------------------------------------------------------------- pools

def pow2_scales(Hkv):
    return fr.scales(Hkv, pow2=True)


@functools.lru_cache(maxsize=4)
def count_pool(page, Nmax, lens, Hkv, D, fp8):
    """(pool, (ks, vs) or ()): K randn, V = C_VALUE everywhere, shuffled placement, NaN (the e4m3 NaN byte) in every page no live entry names
    and in the page the dead entries point at. The rows past len in a sequence's last live page are finite: a kernel that counts them is seen
    by its count."""
    g = torch.Generator().manual_seed(page + Nmax + D)
    k = torch.randn(1, Hkv, Nmax, D, generator=g).to(BF).expand(len(lens), Hkv, Nmax, D)
    v = torch.full((1, Hkv, Nmax, D), C_VALUE, dtype=BF).expand(len(lens), Hkv, Nmax, D)
    pool = pr.make_pool(k, v, page, list(lens), seed=len(lens))
    if not fp8:
        return pool, ()
    ks, vs = pow2_scales(Hkv)
    p8 = fr.quantize_pools(pool, ks, vs)
    live = ~torch.isnan(pool[1].float())
    assert bool((fr.dq(p8[1], vs)[live] == C_VALUE).all())  # the constant survives the quantisation exactly
    return p8, (ks, vs)


def code_bits(Nmax):
    return (Nmax - 1).bit_length()


def codes(Nmax, D):
    """[Nmax, D] of +-1 (0 in the unused columns): fa_reference.onehot_problem's keys."""
    nb = code_bits(Nmax)
    r = D // nb
    c = ((torch.arange(Nmax)[:, None] >> torch.arange(nb)[None, :]) & 1) * 2 - 1
    k = torch.zeros(Nmax, D)
    k[:, :r * nb] = c.repeat(1, r).float()
    return k


def onehot_score(Nmax, D, x):
    """(score of the target in nats, its margin over any other key) for the softmax scale x: 16 r bits x and 2 * 16 r x."""
    nb = code_bits(Nmax)
    r = D // nb
    return 16.0 * r * nb * x, 2 * 16.0 * r * x


@functools.lru_cache(maxsize=4)
def onehot_pool(page, Nmax, lens, Hkv, D, fp8):
    """(pool, (ks, vs) or (), V [Hkv,Nmax,D] fp64 as the kernel means it): keys the code of their position, V rows randn in bf16, or over e4m3
    the codes +-2 under k_scale 1/2 and V bytes that cycle through the finite codes under v_scale 1/4 (fp8_paged_attn_cases) -- the 252 that
    are not +-0: the other keys of a row leave about 16 e^-24 x 112 = 7e-8 in every element of O, far below half a bf16 ulp of the smallest
    non-zero value 2^-11 but not below bf16's smallest number, so an element that should be 0 cannot come out as the bits of 0 (fp16, which the
    all-codes test of the fp16 entries runs in, rounds such a residue to 0; bf16 has fp32's range)."""
    k = codes(Nmax, D).to(BF)[None, None].expand(len(lens), Hkv, Nmax, D)
    if fp8:
        table = torch.tensor([c for c in fr.FINITE_CODES if c & 0x7F], dtype=torch.uint8)
        idx = torch.arange(Hkv * Nmax * D)
        v = (table[(idx * 37 + idx // D) % len(table)].view(fr.f8.F8).float() * 0.25).to(BF).view(1, Hkv, Nmax, D)
    else:
        v = torch.randn(1, Hkv, Nmax, D, generator=torch.Generator().manual_seed(Nmax + D)).to(BF)
    pool = pr.make_pool(k, v.expand(len(lens), Hkv, Nmax, D), page, list(lens), seed=3)
    if not fp8:
        return pool, (), v[0].double()
    ks, vs = torch.full((Hkv,), 0.5), torch.full((Hkv,), 0.25)
    p8 = fr.quantize_pools(pool, ks, vs)
    live = ~torch.isnan(pool[0].float())
    assert bool((fr.dq(p8[0], ks)[live] == pool[0].double()[live]).all()) and bool((fr.dq(p8[1], vs)[live] == pool[1].double()[live]).all())
    return p8, (ks, vs), v[0].double()


def onehot_cases(name, D):
    """The identity test's subset: one one-split decode case, one several-splits case and one packed prefill case per window of ONEHOT_WINDOWS
    the entry has, Nmax small enough for the margin."""
    e = ae.BY_NAME[name]
    out = []
    for table in tables_of(e):
        for W in (ONEHOT_WINDOWS if e.window else [None]):
            pick = [c for c in TABLES[table](name, D) if c.W == W and c.page == 16] or [c for c in TABLES[table](name, D) if c.W == W]
            if not pick and table == "split":  # the split table has its own window: take the windowed case
                pick = [c for c in TABLES[table](name, D) if (c.W is None) == (W is None)]
            if pick and pick[0] not in out:
                out.append(pick[0])
    return out


def lse_tol_at(n):
    """decode_reference.lse_tol of a row whose LSE is ln n: what the randn tests hold it to."""
    return dr.lse_tol(torch.tensor([math.log(n)], dtype=torch.float64))


def count_bound(n):
    return 1.0 / (4.0 * (n + 1))
