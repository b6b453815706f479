"""GPU timing of the multi-head latent attention entries over a paged latent cache held in FP8 (cuda_learn_notes_amd.fa2_decode_paged_mla_bf16_fp8,
kv_append_paged_mla_bf16_fp8, kv_gather_paged_mla_bf16_fp8) in the method of fa_paged_mla_bench.py: launch-inclusive times from
one pair of device events around back-to-back calls after a warm-up, every timed window >= 0.1 s, best of ROUNDS alternating rounds, the pools
rotating over sets that together exceed the 256 MiB Infinity Cache (the sets are counted for the bf16 pools; the FP8 pools are those sets
quantised: the same logical content, the same placement, the same number of sets, half the bytes). Every row is measured TWICE (run 1, run 2, on
the same pools) and each new entry stands beside its bf16 sibling IN THE SAME RUN, the two alternating round by round.
  ratio   bf16 sibling / FP8 entry per run (> 1: the FP8 entry is faster). sib spread = |run 1 - run 2| / min of the sibling: a ratio whose
          distance from 1 does not exceed that spread says nothing.
  decode  fa_paged_mla_bench.py's rows (B, T, Hq, context) at page 16 and 64, scale 192^-1/2, kv_scale 2^-8. rd/copy = the latent bytes the
          row must read (B context 576 for the FP8 pool, 1152 for bf16) over its time, over hipMemcpyDtoD's rate of the same run.
  append  64 sequences x 1 token behind 4096 keys and 4 x 2048 tokens into empty sequences, rope half, q (Hq 16) rotated along.
  gather  8 sequences x 2048 rows out of 4096 keys, with starts.
  python fa_paged_mla_fp8_bench.py [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_d256_bench import COPY_BYTES, copy_rate, spread, two_runs  # noqa: E402
from fa_paged_anyg_bench import BF, pkg  # noqa: E402
from fa_paged_mla_bench import APPEND, DC, DECODE, DK, DR, PAGES, QUICK_DECODE, SCALE, latent_sets  # noqa: E402
from fa_prefill_paged_varlen_bench import cycle  # noqa: E402

F8 = torch.float8_e4m3fn
KV_SCALE = 2.0 ** -8
GATHER = (8, 2048, 4096)  # B, rows per sequence, context


def quantised(pool, kvs):
    """The bf16 pool as e4m3fn codes at the scale kvs: fp32 x (1 / kvs), clamped, rounded to nearest even (the append's quantiser)."""
    return (pool.float() * (1.0 / kvs)).clamp(-448.0, 448.0).to(F8)


def both(runs):
    return {k: [r[k] for r in runs] for k in runs[0]}


def decode_row(B, T, Hq, ctx, page, gen, kvs):
    sets = [(pool, quantised(pool, kvs), bt) for pool, bt in latent_sets(B, ctx, page, gen)]
    sl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    q = (torch.randn(B, T, Hq, DK, device="cuda", generator=gen) * SCALE).to(BF)
    o, o8 = (torch.empty(B, T, Hq, DC, dtype=BF, device="cuda") for _ in range(2))
    S, C, need = pkg.fa2_decode_paged_mla_bf16_fp8_plan(B, T, Hq, ctx // page, page)
    assert (S, C, need) == pkg.fa2_decode_paged_mla_bf16_plan(B, T, Hq, ctx // page, page)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")

    def bf16(nxt=cycle(sets)):
        pool, _, bt = nxt()
        pkg.fa2_decode_paged_mla_bf16(q, pool, bt, sl, SCALE, o, None, ws)

    def fp8(nxt=cycle(sets)):
        _, codes, bt = nxt()
        pkg.fa2_decode_paged_mla_bf16_fp8(q, codes, bt, sl, kvs, SCALE, o8, None, ws)
    r = both(two_runs({"bf16": bf16, "fp8": fp8}))
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(o8.float()).all())
    return r, len(sets), S, C


def append_row(B, T, ctx, page, gen, kvs):
    tq, n = B * T, ctx + T
    N = -(-n // page) * page
    mp = N // page
    sl = torch.full((B,), n, dtype=torch.int32, device="cuda")
    cu = torch.arange(0, tq + 1, T, dtype=torch.int32, device="cuda")
    bt = torch.randperm(B * mp, generator=gen, device="cuda").view(mp, B).t().contiguous().to(torch.int32)
    rnd = lambda *s: (torch.randn(*s, device="cuda", generator=gen) * SCALE).to(BF)  # noqa: E731
    pool = torch.zeros(B * mp, page, DK, dtype=BF, device="cuda")
    pool8 = torch.zeros(B * mp, page, DK, dtype=torch.uint8, device="cuda").view(F8)
    c_new, k_pe, q = rnd(tq, DC), rnd(tq, DR), rnd(tq, 16, DK)
    qo = torch.empty_like(q)
    t64 = pkg.kv_append_rope_table(N, DR, device="cuda")
    return both(two_runs({"bf16": lambda: pkg.kv_append_paged_mla_bf16(c_new, k_pe, pool, bt, sl, cu, q, qo, t64, "half"),
                          "fp8": lambda: pkg.kv_append_paged_mla_bf16_fp8(c_new, k_pe, pool8, bt, sl, cu, kvs, q, qo, t64, "half")}))


def gather_row(B, rows, ctx, page, gen, kvs):
    sets = [(pool, quantised(pool, kvs), bt) for pool, bt in latent_sets(B, ctx, page, gen)]
    cu = torch.arange(0, B * rows + 1, rows, dtype=torch.int32, device="cuda")
    starts = torch.full((B,), ctx - rows, dtype=torch.int32, device="cuda")
    out, out8 = (torch.empty(B * rows, DK, dtype=BF, device="cuda") for _ in range(2))

    def bf16(nxt=cycle(sets)):
        pool, _, bt = nxt()
        pkg.kv_gather_paged_mla_bf16(pool, bt, cu, out, starts)

    def fp8(nxt=cycle(sets)):
        _, codes, bt = nxt()
        pkg.kv_gather_paged_mla_bf16_fp8(codes, bt, cu, kvs, out8, starts)
    return both(two_runs({"bf16": bf16, "fp8": fp8})), len(sets)


def line(what, r):
    b, f = r["bf16"], r["fp8"]
    return "%-26s %10.1f %10.1f %5.1f%% %10.1f %10.1f %5.1f%% %7.3f %7.3f" % (what, b[0] * 1e3, b[1] * 1e3, 100 * spread(*b), f[0] * 1e3, f[1] * 1e3,
                                                                              100 * spread(*f), b[0] / f[0], b[1] / f[1])


HEAD = "%-26s %10s %10s %6s %10s %10s %6s %7s %7s" % ("", "bf16 us 1", "bf16 us 2", "spread", "fp8 us 1", "fp8 us 2", "spread", "ratio 1", "ratio 2")

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    kvs = torch.tensor([KV_SCALE], dtype=torch.float32, device="cuda")
    copy = [copy_rate() for _ in range(2)]
    print("MLA over a paged latent cache held in FP8 (rows of e4m3fn codes [c 512 | k_pe 64], 576 bytes a token, one kv_scale = 2^-8) beside the "
          "bf16 entries (1152 bytes a token) on pools of the same logical content: us per call (launch-inclusive), two runs of every number and "
          "their spread; ratio = bf16 / fp8 per run")
    if copy[0]:
        print("hipMemcpyDtoD of %d MiB, read + written bytes over time: %.2f and %.2f TB/s (spread %.1f%%)" % (COPY_BYTES >> 20, copy[0], copy[1],
                                                                                                           100 * spread(*copy)))
    else:
        print("hipMemcpyDtoD: the vendor yardstick unit is not built, no copy rate")
    print("decode: (B, T, Hq, context) page, sets, S x C; rd/copy of run 1 for either entry")
    print(HEAD + " %9s %9s" % ("bf16 rd/c", "fp8 rd/c"))
    for (B, T, Hq, ctx) in (QUICK_DECODE if a.quick else DECODE):
        for page in PAGES:
            r, nsets, S, C = decode_row(B, T, Hq, ctx, page, gen, kvs)
            rc = ["%9.2f" % (B * ctx * DK * w / (r[k][0] * 1e-3) * 1e-12 / copy[0]) if copy[0] else "%9s" % "-" for k, w in (("bf16", 2), ("fp8", 1))]
            print(line("%s p%d %d %dx%d" % (str((B, T, Hq, ctx)).replace(" ", ""), page, nsets, S, C), r) + " " + " ".join(rc), flush=True)
            torch.cuda.empty_cache()
    print("append, page 16, rope half with q (Hq 16): B x tokens @ context")
    print(HEAD)
    for (B, T, ctx) in (APPEND[:1] if a.quick else APPEND):
        print(line("%d x %d @ %d" % (B, T, ctx), append_row(B, T, ctx, 16, gen, kvs)), flush=True)
        torch.cuda.empty_cache()
    print("gather, page 16, with starts: B x rows out of context, sets")
    print(HEAD)
    r, nsets = gather_row(*GATHER, 16, gen, kvs)
    print(line("%d x %d of %d, %d sets" % (*GATHER, nsets), r), flush=True)
