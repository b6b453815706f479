"""GPU timing of the sparse multi-head latent attention decode over the paged latent cache (cuda_learn_notes_amd.fa2_decode_paged_mla_sparse_bf16;
DESIGN 4.4.20) in the method of fa_paged_mla_bench.py: launch-inclusive times from one pair of device events around back-to-back calls after a
warm-up, every timed window >= 0.1 s, best of ROUNDS alternating rounds, the pools rotating over sets that together exceed the 256 MiB Infinity
Cache. Everything is measured TWICE (run 1, run 2, on the same pools) and both are printed.
  (B, T, Hq) x context at page 64, topk 2048, every sequence of length `context`, scale 192^-1/2. The list of a query token is a seeded random
  sample of 2048 distinct positions every token of the sequence sees (below context - (T - 1)), unsorted. Three entries in the one run, on the
  same pools and queries:
    sparse   fa2_decode_paged_mla_sparse_bf16 with those lists
    full     fa2_decode_paged_mla_bf16 on the whole context: what a caller without the sparse entry would run (and another function)
    ctx2048  fa2_decode_paged_mla_bf16 on the first 2048 positions of the same sequences (seqlens = 2048, the table cut to 2048 / page entries):
             as many rows per query token, fetched contiguously in position
  The figure of merit is sparse / ctx2048, the price of the indirection; full / sparse is what the entry saves. rd = the latent bytes the sparse
  row addresses, B T 2048 x 1152, over its time, TB/s, beside hipMemcpyDtoD (read + written bytes over time) from the same run.
  python fa_paged_mla_sparse_bench.py [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_d256_bench import COPY_BYTES, copy_rate, spread, two_runs  # noqa: E402
from fa_paged_anyg_bench import BF, pkg  # noqa: E402
from fa_decode_paged_bench import rotating  # noqa: E402
from fa_prefill_paged_varlen_bench import cycle  # noqa: E402

DC, DK = 512, 576
SCALE = 192 ** -0.5
PAGE, TOPK = 64, 2048
SHAPES = [(64, 1, 16), (64, 1, 128), (8, 1, 128), (4, 4, 128)]
CONTEXTS = [4096, 32768, 131072]
QUICK = [((64, 1, 16), 4096), ((4, 4, 128), 32768)]


def latent_sets(B, N, gen):
    """Rotating sets of (pool bf16 [B N / page, page, 576], block_table): randn rows at the scale of the tests, pages placed by a random
    permutation."""
    mp = N // PAGE

    def make():
        pool = torch.empty(B * mp, PAGE, DK, dtype=BF, device="cuda").normal_(0.0, SCALE, generator=gen)
        return pool, torch.randperm(B * mp, generator=gen, device="cuda").view(B, mp).to(torch.int32)
    return rotating(make, B * N * DK * 2)


def sample_lists(B, T, ctx, gen):
    """int32 [B, T, 2048]: per query token 2048 distinct positions below ctx - (T - 1), in random order."""
    out = torch.empty(B * T, TOPK, dtype=torch.int32, device="cuda")
    for i in range(B * T):  # a row at a time: the keys of one token are 4 bytes x context
        out[i] = torch.randperm(ctx - (T - 1), generator=gen, device="cuda")[:TOPK].to(torch.int32)
    return out.view(B, T, TOPK)


def row(B, T, Hq, ctx, gen):
    sets = latent_sets(B, ctx, gen)
    q = (torch.randn(B, T, Hq, DK, device="cuda", generator=gen) * SCALE).to(BF)
    idx = sample_lists(B, T, ctx, gen)
    sl_full = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    sl_2048 = torch.full((B,), TOPK, dtype=torch.int32, device="cuda")
    cut = [bt[:, :TOPK // PAGE].contiguous() for _, bt in sets]
    o = [torch.empty(B, T, Hq, DC, dtype=BF, device="cuda") for _ in range(3)]
    plans = (pkg.fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, TOPK, ctx // PAGE, PAGE), pkg.fa2_decode_paged_mla_bf16_plan(B, T, Hq, ctx // PAGE, PAGE),
             pkg.fa2_decode_paged_mla_bf16_plan(B, T, Hq, TOPK // PAGE, PAGE))
    ws = [torch.empty(max(p[2], 16), dtype=torch.uint8, device="cuda") for p in plans]

    def sparse(nxt=cycle(sets)):
        pool, bt = nxt()
        pkg.fa2_decode_paged_mla_sparse_bf16(q, pool, bt, sl_full, idx, SCALE, o[0], None, ws[0])

    def full(nxt=cycle(sets)):
        pool, bt = nxt()
        pkg.fa2_decode_paged_mla_bf16(q, pool, bt, sl_full, SCALE, o[1], None, ws[1])

    def ctx2048(nxt=cycle(list(zip(sets, cut)))):
        (pool, _), bt = nxt()
        pkg.fa2_decode_paged_mla_bf16(q, pool, bt, sl_2048, SCALE, o[2], None, ws[2])

    runs = two_runs({"sparse": sparse, "full": full, "ctx2048": ctx2048})
    assert all(bool(torch.isfinite(x.float()).all()) for x in o)
    return runs, len(sets), plans


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    copy = [copy_rate() for _ in range(2)]
    print("sparse MLA decode over a paged latent cache (bf16 rows [c 512 | k_pe 64], 1152 bytes a token), topk %d, page %d: us per call "
          "(launch-inclusive), two runs of every number. sparse = fa2_decode_paged_mla_sparse_bf16 on seeded random lists; full = "
          "fa2_decode_paged_mla_bf16 on the whole context; ctx2048 = fa2_decode_paged_mla_bf16 on the first 2048 positions. sp/2048 = sparse / "
          "ctx2048 (the figure of merit), full/sp = full / sparse; rd = B T 2048 x 1152 bytes over the sparse time, TB/s" % (TOPK, PAGE))
    if copy[0]:
        print("hipMemcpyDtoD of %d MiB, read + written bytes over time: %.2f and %.2f TB/s (spread %.1f%%)" % (COPY_BYTES >> 20, copy[0], copy[1],
                                                                                                           100 * spread(*copy)))
    else:
        print("hipMemcpyDtoD: the vendor yardstick unit is not built, no copy rate")
    print("%-16s %7s %4s %-7s %-8s %-7s %9s %9s %9s %9s %9s %9s %8s %8s %8s %8s %5s %5s" % (
        "(B, T, Hq)", "context", "sets", "S x C", "full", "ctx2048", "sparse 1", "sparse 2", "full 1", "full 2", "2048 1", "2048 2", "sp/2048 1",
        "sp/2048 2", "full/sp 1", "full/sp 2", "rd 1", "rd 2"))
    todo = QUICK if a.quick else [(s, c) for s in SHAPES for c in CONTEXTS]
    for (B, T, Hq), ctx in todo:
        runs, nsets, plans = row(B, T, Hq, ctx, gen)
        us = {k: [r[k] * 1e3 for r in runs] for k in ("sparse", "full", "ctx2048")}
        rd = [B * T * TOPK * DK * 2 / (u * 1e-6) * 1e-12 for u in us["sparse"]]
        print("%-16s %7d %4d %-7s %-8s %-7s %9.1f %9.1f %9.1f %9.1f %9.1f %9.1f %9.3f %9.3f %9.2f %9.2f %5.2f %5.2f" % (
            str((B, T, Hq)), ctx, nsets, *("%dx%d" % p[:2] for p in plans), *us["sparse"], *us["full"], *us["ctx2048"],
            us["sparse"][0] / us["ctx2048"][0], us["sparse"][1] / us["ctx2048"][1], us["full"][0] / us["sparse"][0], us["full"][1] / us["sparse"][1],
            rd[0], rd[1]), flush=True)
        torch.cuda.empty_cache()
