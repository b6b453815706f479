"""GPU timing of the DSA indexer's FP8 cache (cuda_learn_notes_amd.mla_index_logits_paged_bf16_fp8 and kv_append_paged_index_bf16_fp8;
DESIGN 4.4.24) beside the bf16 entries, in the method of mla_index_bench.py: launch-inclusive times from one pair of device events around
back-to-back calls after a warm-up, every timed window >= 0.1 s, best of ROUNDS alternating rounds -- the fp8 and the bf16 entry alternate
inside every round of one run -- the pools rotating over sets that together exceed the 256 MiB Infinity Cache. Everything is measured TWICE
(run 1, run 2, on the same pools) and both are printed; hipMemcpyDtoD is taken in the same run.
  (B, T) x context at page 64, Hi = 64 index heads, every sequence of length `context` (the rows of DESIGN 4.4.22's table):
    bf16     mla_index_logits_paged_bf16 on a bf16 pool [P,64,128]; rd = sum over (b, t) of vis(b, t) x 256 bytes over its time, TB/s
    fp8      mla_index_logits_paged_bf16_fp8 on a uint8 pool [P,64,132] of the same tokens' worth; rd = ... x 132 bytes over its time, TB/s
  then both appends at (64, 1) and (1, 2048), one pool of 4096 tokens a sequence.
  python mla_index_fp8_bench.py [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_d256_bench import COPY_BYTES, copy_rate, spread, two_runs  # noqa: E402
from fa_paged_anyg_bench import BF, pkg  # noqa: E402
from fa_decode_paged_bench import rotating  # noqa: E402
from fa_prefill_paged_varlen_bench import cycle  # noqa: E402
from mla_index_bench import D, HI, PAGE, QUICK, ROWS  # noqa: E402

ROW8 = 132
APPENDS = [(64, 1), (1, 2048)]


def fp8_pool(P, gen):
    """uint8 [P,PAGE,132]: finite codes (bytes below 0x78, and their negatives), every scale 2^-5."""
    pool = torch.randint(0, 0x78, (P, PAGE, ROW8), dtype=torch.uint8, device="cuda", generator=gen)
    pool |= torch.randint(0, 2, (P, PAGE, ROW8), dtype=torch.uint8, device="cuda", generator=gen) << 7
    pkg.index_pool_fp8_views(pool)[1].fill_(2.0 ** -5)
    return pool


def logits_row(B, T, ctx, gen):
    mp = ctx // PAGE

    def make():
        return (torch.empty(B * mp, PAGE, D, dtype=BF, device="cuda").normal_(0.0, 1.0, generator=gen), fp8_pool(B * mp, gen),
                torch.randperm(B * mp, generator=gen, device="cuda").view(B, mp).to(torch.int32))
    sets = rotating(make, B * ctx * (2 * D + ROW8))
    qi = torch.randn(B, T, HI, D, device="cuda", generator=gen).to(BF)
    w = torch.randn(B, T, HI, device="cuda", generator=gen) * (HI * D) ** -0.5
    sl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    lg = [torch.full((B, T, ctx), float("-inf"), device="cuda") for _ in range(2)]

    def bf16(nxt=cycle(sets)):
        ipool, _, bt = nxt()
        pkg.mla_index_logits_paged_bf16(qi, w, ipool, bt, sl, lg[0])

    def fp8(nxt=cycle(sets)):
        _, ipool8, bt = nxt()
        pkg.mla_index_logits_paged_bf16_fp8(qi, w, ipool8, bt, sl, lg[1])

    runs = two_runs({"bf16": bf16, "fp8": fp8})
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lg[1][:, T - 1]).all())
    keys = B * sum(ctx - (T - 1 - t) for t in range(T))
    return runs, len(sets), keys


def append_row(B, T, gen, ctx=4096):
    mp = ctx // PAGE
    total = B * T

    def make():
        return (torch.empty(B * mp, PAGE, D, dtype=BF, device="cuda").normal_(0.0, 1.0, generator=gen), fp8_pool(B * mp, gen),
                torch.randperm(B * mp, generator=gen, device="cuda").view(B, mp).to(torch.int32))
    sets = rotating(make, B * ctx * (2 * D + ROW8))
    k_new = torch.randn(total, D, device="cuda", generator=gen).to(BF)
    sl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    cu = torch.arange(B + 1, dtype=torch.int32, device="cuda") * T

    def bf16(nxt=cycle(sets)):
        ipool, _, bt = nxt()
        pkg.kv_append_paged_index_bf16(k_new, ipool, bt, sl, cu)

    def fp8(nxt=cycle(sets)):
        _, ipool8, bt = nxt()
        pkg.kv_append_paged_index_bf16_fp8(k_new, ipool8, bt, sl, cu, True)

    return two_runs({"bf16": bf16, "fp8": fp8}), len(sets)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    copy = [copy_rate() for _ in range(2)]
    print("the DSA indexer's logits over a paged index-key cache in bf16 (256 bytes a token) and in e4m3 with one fp32 scale a token (132 bytes), "
          "Hi %d, page %d: us per call (launch-inclusive), two runs of every number, the two entries alternating in every round; rd = the "
          "index-key bytes the entry addresses over its time, TB/s" % (HI, PAGE))
    if copy[0]:
        print("hipMemcpyDtoD of %d MiB, read + written bytes over time: %.2f and %.2f TB/s (spread %.1f%%)" % (COPY_BYTES >> 20, copy[0], copy[1],
                                                                                                           100 * spread(*copy)))
    else:
        print("hipMemcpyDtoD: the vendor yardstick unit is not built, no copy rate")
    print("%-10s %7s %4s %9s %9s %9s %9s %7s %7s %7s %7s %7s %7s" % ("(B, T)", "context", "sets", "bf16 1", "bf16 2", "fp8 1", "fp8 2", "rd bf 1", "rd bf 2",
                                                                  "rd f8 1", "rd f8 2", "ratio 1", "ratio 2"))
    for (B, T), ctx in (QUICK if a.quick else ROWS):
        runs, nsets, keys = logits_row(B, T, ctx, gen)
        us = [r[n] * 1e3 for n in ("bf16", "fp8") for r in runs]
        rd = [keys * nb / (r[n] * 1e-3) * 1e-12 for n, nb in (("bf16", 2 * D), ("fp8", ROW8)) for r in runs]
        print("%-10s %7d %4d %9.1f %9.1f %9.1f %9.1f %7.2f %7.2f %7.2f %7.2f %7.3f %7.3f"
              % (str((B, T)), ctx, nsets, *us, *rd, runs[0]["bf16"] / runs[0]["fp8"], runs[1]["bf16"] / runs[1]["fp8"]), flush=True)
        torch.cuda.empty_cache()
    print("the appends, context 4096: kv_append_paged_index_bf16 and kv_append_paged_index_bf16_fp8 (scale_pow2), us per call")
    for B, T in APPENDS[:1] if a.quick else APPENDS:
        runs, nsets = append_row(B, T, gen)
        print("%-10s %4d %9.1f %9.1f %9.1f %9.1f" % (str((B, T)), nsets, runs[0]["bf16"] * 1e3, runs[1]["bf16"] * 1e3, runs[0]["fp8"] * 1e3,
                                                    runs[1]["fp8"] * 1e3), flush=True)
        torch.cuda.empty_cache()
