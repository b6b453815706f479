"""GPU timing of the DSA indexer (cuda_learn_notes_amd.kv_append_paged_index_bf16, mla_index_logits_paged_bf16, mla_index_topk)
in the method of fa_paged_mla_sparse_bench.py: launch-inclusive times from one pair of device events around back-to-back calls after a warm-up,
every timed window >= 0.1 s, best of ROUNDS alternating rounds, the pools rotating over sets that together exceed the 256 MiB Infinity Cache.
Everything is measured TWICE (run 1, run 2, on the same pools) and both are printed.
  (B, T) x context at page 64, Hi = 64 index heads, topk 2048, every sequence of length `context`; the prefill row is (1, 2048) at context 4096.
    logits   mla_index_logits_paged_bf16; rd = the index-key bytes it addresses, sum over (b, t) of vis(b, t) x 256, over its time, TB/s,
             beside hipMemcpyDtoD (read + written bytes over time) from the same run
    torch    the caller's own indexer: einsum('bthd,bjd->bthj') in bf16 on keys that are ALREADY gathered dense (the gather is not timed),
             relu, the weighted head sum -- every position, no causal edge
    topk     mla_index_topk on the logits entry's output
    t.topk   torch.topk(2048) on the same logits with -inf behind the causal edge
    step     kv_append_paged_index_bf16 (one token a sequence) + logits + topk + fa2_decode_paged_mla_sparse_bf16 (Hq 128), back to back
    dense    fa2_decode_paged_mla_bf16 (Hq 128) on the whole context: the number the sparse path exists to beat (T <= 8 only)
  python mla_index_bench.py [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_d256_bench import COPY_BYTES, copy_rate, spread, two_runs  # noqa: E402
from fa_paged_anyg_bench import BF, pkg  # noqa: E402
from fa_decode_paged_bench import rotating  # noqa: E402
from fa_prefill_paged_varlen_bench import cycle  # noqa: E402

D, HI, HQ, DC, DK = 128, 64, 128, 512, 576
SCALE = 192 ** -0.5
PAGE, TOPK = 64, 2048
ROWS = [((64, 1), 4096), ((64, 1), 32768), ((64, 1), 131072), ((8, 1), 4096), ((8, 1), 32768), ((8, 1), 131072), ((4, 4), 4096), ((4, 4), 32768),
        ((4, 4), 131072), ((1, 2048), 4096)]
QUICK = [((8, 1), 4096), ((4, 4), 32768)]


def row(B, T, ctx, gen):
    mp = ctx // PAGE
    step = T <= 8  # the dense entry's cap; the prefill row times the two new entries only

    def make():
        ipool = torch.empty(B * mp, PAGE, D, dtype=BF, device="cuda").normal_(0.0, 1.0, generator=gen)
        lat = torch.empty(B * mp, PAGE, DK, dtype=BF, device="cuda").normal_(0.0, SCALE, generator=gen) if step else None
        return ipool, lat, torch.randperm(B * mp, generator=gen, device="cuda").view(B, mp).to(torch.int32)
    sets = rotating(make, B * ctx * (D + (DK if step else 0)) * 2)
    qi = torch.randn(B, T, HI, D, device="cuda", generator=gen).to(BF)
    w = torch.randn(B, T, HI, device="cuda", generator=gen) * (HI * D) ** -0.5
    sl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    lg = torch.full((B, T, ctx), float("-inf"), device="cuda")
    idx = torch.empty(B, T, TOPK, dtype=torch.int32, device="cuda")
    k_new = torch.randn(B, D, device="cuda", generator=gen).to(BF)
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda")
    dense_keys = sets[0][0][sets[0][2].long()].view(B, ctx, D)  # the torch indexer's keys, gathered once, outside every timed window
    wb = w.to(BF)

    def logits(nxt=cycle(sets)):
        ipool, _, bt = nxt()
        pkg.mla_index_logits_paged_bf16(qi, w, ipool, bt, sl, lg)

    def torch_indexer():
        return torch.einsum("bthj,bth->btj", torch.einsum("bthd,bjd->bthj", qi, dense_keys).relu_(), wb)

    def topk():
        pkg.mla_index_topk(lg, sl, TOPK, idx)

    def torch_topk():
        return torch.topk(lg, TOPK, dim=-1)

    calls = {"logits": logits, "torch": torch_indexer, "topk": topk, "t.topk": torch_topk}
    logits()  # the logits the two top-k calls select from; positions at or past vis keep -inf
    if step:
        q = (torch.randn(B, T, HQ, DK, device="cuda", generator=gen) * SCALE).to(BF)
        o = [torch.empty(B, T, HQ, DC, dtype=BF, device="cuda") for _ in range(2)]
        plans = (pkg.fa2_decode_paged_mla_sparse_bf16_plan(B, T, HQ, TOPK, mp, PAGE), pkg.fa2_decode_paged_mla_bf16_plan(B, T, HQ, mp, PAGE))
        ws = [torch.empty(max(p[2], 16), dtype=torch.uint8, device="cuda") for p in plans]

        def whole(nxt=cycle(sets)):
            ipool, lat, bt = nxt()
            pkg.kv_append_paged_index_bf16(k_new, ipool, bt, sl, cu)
            pkg.mla_index_logits_paged_bf16(qi, w, ipool, bt, sl, lg)
            pkg.mla_index_topk(lg, sl, TOPK, idx)
            pkg.fa2_decode_paged_mla_sparse_bf16(q, lat, bt, sl, idx, SCALE, o[0], None, ws[0])

        def dense(nxt=cycle(sets)):
            _, lat, bt = nxt()
            pkg.fa2_decode_paged_mla_bf16(q, lat, bt, sl, SCALE, o[1], None, ws[1])

        calls.update({"step": whole, "dense": dense})
    runs = two_runs(calls)
    torch.cuda.synchronize()
    assert bool((idx >= 0).all()) and bool((idx < ctx).all())
    key_bytes = B * sum(ctx - (T - 1 - t) for t in range(T)) * D * 2
    return runs, len(sets), key_bytes


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    copy = [copy_rate() for _ in range(2)]
    print("the DSA indexer over a paged index-key cache (bf16 keys of 128 dims, 256 bytes a token), Hi %d, topk %d, page %d: us per call "
          "(launch-inclusive), two runs of every number. logits = mla_index_logits_paged_bf16, rd = the index-key bytes it addresses over its "
          "time, TB/s; torch = einsum + relu + weighted sum in bf16 on keys gathered beforehand; topk = mla_index_topk; t.topk = torch.topk; "
          "step = index append + logits + topk + fa2_decode_paged_mla_sparse_bf16 (Hq %d); dense = fa2_decode_paged_mla_bf16 on the whole "
          "context (Hq %d)" % (HI, TOPK, PAGE, HQ, HQ))
    if copy[0]:
        print("hipMemcpyDtoD of %d MiB, read + written bytes over time: %.2f and %.2f TB/s (spread %.1f%%)" % (COPY_BYTES >> 20, copy[0], copy[1],
                                                                                                           100 * spread(*copy)))
    else:
        print("hipMemcpyDtoD: the vendor yardstick unit is not built, no copy rate")
    names = ("logits", "torch", "topk", "t.topk", "step", "dense")
    print("%-10s %7s %4s " % ("(B, T)", "context", "sets") + " ".join("%9s %9s" % (n + " 1", n + " 2") for n in names) + "  rd 1  rd 2")
    for (B, T), ctx in (QUICK if a.quick else ROWS):
        runs, nsets, key_bytes = row(B, T, ctx, gen)
        cells = " ".join("%9.1f %9.1f" % tuple(r[n] * 1e3 for r in runs) if n in runs[0] else "%9s %9s" % ("-", "-") for n in names)
        rd = [key_bytes / (r["logits"] * 1e-3) * 1e-12 for r in runs]
        print("%-10s %7d %4d " % (str((B, T)), ctx, nsets) + cells + " %5.2f %5.2f" % tuple(rd), flush=True)
        torch.cuda.empty_cache()
