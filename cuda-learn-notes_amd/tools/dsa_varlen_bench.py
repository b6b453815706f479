"""GPU timing of the packed ("varlen") DSA step (cuda_learn_notes_amd.mla_index_logits_paged_varlen_bf16, mla_index_topk_varlen,
fa2_decode_paged_mla_sparse_varlen_bf16). Launch-inclusive times from one pair of device events around back-to-back calls
after a warm-up, every timed window >= 0.1 s (fa_prefill_paged_bench.timed). Every comparison is INTERLEAVED: the calls of a row take turns
for ROUNDS rounds, and a cell is the median over the rounds with its spread (max - min) / median. One set of pools per row (no rotation):
the two sides of a comparison read the same bytes in the same state, which is what a ratio needs; the absolute times of small rows are
cache-warm.

  Table 1, the cost of the prologue: the packed entries on cu_q = [0, T, 2 T, ...] against the fixed-T entries on the same tensors, page 64,
  Hi 64, Hq 128, topk 2048, every sequence of length `context`. ratio = packed median / fixed median; a row is flagged with * when the packed
  median lies outside [fixed min, fixed max] of the same run.
  Table 2, what the feature buys: one 2048-token prompt chunk + 63 single-token decode rows (total_q 2111) as ONE packed call per kernel,
  against (split) a (1, 2048) and a (63, 1) fixed-T call per kernel and (padded) every sequence padded to T = 2048 -- the padded form at
  B = 8 (the chunk + 7 decode rows), where its q of 8 x 2048 x 128 x 576 bf16 is 2.4 GB; at B = 64 it is eight times that in every tensor.
  python dsa_varlen_bench.py [--quick]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_anyg_bench import BF, pkg  # noqa: E402
from fa_prefill_paged_bench import timed  # noqa: E402

D, HI, HQ, DC, DK = 128, 64, 128, 512, 576
SCALE = 192 ** -0.5
PAGE, TOPK, ROUNDS = 64, 2048, 5
UNIFORM = [((64, 1), 4096), ((64, 1), 32768), ((8, 1), 32768), ((4, 4), 32768), ((1, 2048), 4096), ((256, 1), 4096), ((256, 1), 32768)]
QUICK = [((8, 1), 4096), ((256, 1), 4096)]
MIXED_CTX = (8192, 32768)
CHUNK, DECODES = 2048, 63


def interleaved(calls):
    """{name: (median ms, spread, min, max)} over ROUNDS rounds in which the calls take turns."""
    seen = {n: [] for n in calls}
    for _ in range(ROUNDS):
        for n, f in calls.items():
            seen[n].append(timed(f))
    torch.cuda.synchronize()
    return {n: (statistics.median(v), (max(v) - min(v)) / statistics.median(v), min(v), max(v)) for n, v in seen.items()}


def pools(B, ctx, gen):
    mp = ctx // PAGE
    ipool = torch.empty(B * mp, PAGE, D, dtype=BF, device="cuda").normal_(0.0, 1.0, generator=gen)
    lat = torch.empty(B * mp, PAGE, DK, dtype=BF, device="cuda").normal_(0.0, SCALE, generator=gen)
    return ipool, lat, torch.randperm(B * mp, generator=gen, device="cuda").view(B, mp).to(torch.int32), mp


def tensors(rows, ctx, gen):
    return dict(qi=torch.randn(rows, HI, D, device="cuda", generator=gen).to(BF), w=torch.randn(rows, HI, device="cuda", generator=gen) * (HI * D) ** -0.5,
                q=(torch.randn(rows, HQ, DK, device="cuda", generator=gen) * SCALE).to(BF), lg=torch.full((rows, ctx), float("-inf"), device="cuda"),
                idx=torch.empty(rows, TOPK, dtype=torch.int32, device="cuda"), o=torch.empty(rows, HQ, DC, dtype=BF, device="cuda"))


def fixed_calls(t, lo, B, T, ipool, lat, bt, sl, mp):
    """The three fixed-T calls on rows lo ... lo + B T of the packed tensors, viewed [B, T, ...]."""
    v = {k: x[lo:lo + B * T].view(B, T, *x.shape[1:]) for k, x in t.items()}
    ws = torch.empty(max(pkg.fa2_decode_paged_mla_sparse_bf16_plan(B, T, HQ, TOPK, mp, PAGE)[2], 16), dtype=torch.uint8, device="cuda")
    return (lambda: pkg.mla_index_logits_paged_bf16(v["qi"], v["w"], ipool, bt, sl, v["lg"]),
            lambda: pkg.mla_index_topk(v["lg"], sl, TOPK, v["idx"]),
            lambda: pkg.fa2_decode_paged_mla_sparse_bf16(v["q"], lat, bt, sl, v["idx"], SCALE, v["o"], None, ws))


def packed_calls(t, rows, ipool, lat, bt, sl, cu, mp):
    ws = torch.empty(max(pkg.fa2_decode_paged_mla_sparse_varlen_bf16_plan(rows, HQ, TOPK, mp, PAGE)[2], 16), dtype=torch.uint8, device="cuda")
    return (lambda: pkg.mla_index_logits_paged_varlen_bf16(t["qi"], t["w"], ipool, bt, sl, cu, t["lg"]),
            lambda: pkg.mla_index_topk_varlen(t["lg"], sl, cu, TOPK, t["idx"]),
            lambda: pkg.fa2_decode_paged_mla_sparse_varlen_bf16(t["q"], lat, bt, sl, cu, t["idx"], SCALE, t["o"], None, ws))


def chain(fs):
    def run():
        for f in fs:
            f()
    return run


def uniform_row(B, T, ctx, gen):
    ipool, lat, bt, mp = pools(B, ctx, gen)
    t = tensors(B * T, ctx, gen)
    sl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    cu = (torch.arange(B + 1, dtype=torch.int32, device="cuda") * T).to(torch.int32)
    fx, pk = fixed_calls(t, 0, B, T, ipool, lat, bt, sl, mp), packed_calls(t, B * T, ipool, lat, bt, sl, cu, mp)
    fx[0](), fx[1]()  # logits and lists that the timed top-k and sparse calls read
    calls = {}
    for name, f, p in zip(("logits", "topk", "sparse"), fx, pk):
        calls[name + " fixed"], calls[name + " packed"] = f, p
    return interleaved(calls)


def mixed_row(ctx, gen):
    B = 1 + DECODES
    rows = CHUNK + DECODES
    ipool, lat, bt, mp = pools(B, ctx, gen)
    t = tensors(rows, ctx, gen)
    sl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    cu = torch.tensor([0] + [CHUNK + i for i in range(B)], dtype=torch.int32, device="cuda")
    pk = packed_calls(t, rows, ipool, lat, bt, sl, cu, mp)
    a = fixed_calls(t, 0, 1, CHUNK, ipool, lat, bt[:1], sl[:1], mp)
    b = fixed_calls(t, CHUNK, DECODES, 1, ipool, lat, bt[1:], sl[1:], mp)
    pk[0](), pk[1]()
    calls = {}
    for i, name in enumerate(("logits", "topk", "sparse")):
        calls[name + " packed"], calls[name + " split"] = pk[i], chain((a[i], b[i]))
    calls["chain packed"], calls["chain split"] = chain(pk), chain(a + b)
    out = interleaved(calls)
    del t, a, b, pk
    torch.cuda.empty_cache()
    Bp = 8  # the padded form: the chunk + 7 decode rows, every sequence T = 2048
    tp = tensors(Bp * CHUNK, ctx, gen)
    pd = fixed_calls(tp, 0, Bp, CHUNK, ipool, lat, bt[:Bp], sl[:Bp], mp)
    pd[0](), pd[1]()
    calls = {name + " padded(B=8)": pd[i] for i, name in enumerate(("logits", "topk", "sparse"))}
    calls["chain padded(B=8)"] = chain(pd)
    out.update(interleaved(calls))
    return out


def cell(r):
    return "%9.1f us +-%4.1f%%" % (r[0] * 1e3, 100 * r[1])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    print("the packed DSA step, bf16 caches, page %d, Hi %d, Hq %d, topk %d: median us per call (launch-inclusive) over %d interleaved rounds, "
          "+- = (max - min) / median" % (PAGE, HI, HQ, TOPK, ROUNDS))
    print("table 1: packed entries on uniform cu_q against the fixed-T entries on the same tensors; * = the packed median lies outside the fixed "
          "entry's own [min, max] of this run")
    for (B, T), ctx in (QUICK if a.quick else UNIFORM):
        r = uniform_row(B, T, ctx, gen)
        line = "%-10s ctx %6d" % (str((B, T)), ctx)
        for k in ("logits", "topk", "sparse"):
            f, p = r[k + " fixed"], r[k + " packed"]
            line += " | %s fixed %s packed %s ratio %.3f%s" % (k, cell(f), cell(p), p[0] / f[0], " " if f[2] <= p[0] <= f[3] else "*")
        print(line, flush=True)
        torch.cuda.empty_cache()
    print("table 2: one %d-token chunk + %d decode rows (total_q %d) as one packed call per kernel, against the split form (a (1, %d) and a "
          "(%d, 1) call per kernel) and the padded form at B = 8 (T = %d for every sequence)" % (CHUNK, DECODES, CHUNK + DECODES, CHUNK, DECODES, CHUNK))
    for ctx in (MIXED_CTX[:1] if a.quick else MIXED_CTX):
        r = mixed_row(ctx, gen)
        for k in ("logits", "topk", "sparse", "chain"):
            print("ctx %6d %-7s packed %s | split %s (x%.2f) | padded(B=8) %s (x%.2f)"
                  % (ctx, k, cell(r[k + " packed"]), cell(r[k + " split"]), r[k + " split"][0] / r[k + " packed"][0], cell(r[k + " padded(B=8)"]),
                     r[k + " padded(B=8)"][0] / r[k + " packed"][0]), flush=True)
        torch.cuda.empty_cache()
