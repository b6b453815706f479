"""GPU timing of the multi-head latent attention entries over a paged latent cache (cuda_learn_notes_amd.fa2_decode_paged_mla_bf16,
kv_append_paged_mla_bf16) in the method of fa_paged_d256_bench.py: launch-inclusive times from one pair of device events around
back-to-back calls after a warm-up, every timed window >= 0.1 s, best of ROUNDS alternating rounds, the pools rotating over sets that together
exceed the 256 MiB Infinity Cache. Everything is measured TWICE (run 1, run 2, on the same pools) and both are printed with their spread
|a - b| / min(a, b). There is no earlier MLA number.
  decode  (B, T, Hq, context) at page 16 and 64, every sequence of length `context` (the T newest tokens included), scale 192^-1/2. One
          yardstick, measured in the same run: hipMemcpyDtoD of COPY_BYTES (bytes read + bytes written over time). rd = the latent bytes the row
          must read -- B context 1152, a row once whatever Hq is -- over its time, TB/s; rd/copy = that over the copy's rate; for Hq = 128 the
          attention rate 2 R n (576 + 512) flops per sequence over the time, TFLOP/s.
  append  64 sequences x 1 token behind 4096 keys and 4 x 2048 tokens into empty sequences, rope half, q rotated along (Hq 16 for MLA): beside
          kv_append_paged_varlen_bf16 at D = 128, Hkv = 8, Hq = 32 on the same tokens. Both times, no ratio target.
  python fa_paged_mla_bench.py [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_d256_bench import COPY_BYTES, copy_rate, spread, two_runs  # noqa: E402
from fa_paged_anyg_bench import BF, pkg  # noqa: E402
from fa_decode_paged_bench import rotating  # noqa: E402
from fa_prefill_paged_varlen_bench import cycle  # noqa: E402

DC, DR, DK = 512, 64, 576
SCALE = 192 ** -0.5
PAGES = (16, 64)
DECODE = [(64, 1, 16, 4096), (64, 1, 128, 4096), (128, 1, 16, 1024), (8, 2, 128, 16384), (1, 1, 16, 16384), (1, 1, 128, 16384)]
QUICK_DECODE = [(64, 1, 16, 4096), (1, 1, 128, 16384)]
APPEND = [(64, 1, 4096), (4, 2048, 0)]  # (B, tokens per sequence, context)


def latent_sets(B, N, page, gen):
    """Rotating sets of (pool bf16 [B N / page, page, 576], block_table): randn rows at the scale of the tests, pages placed by a random
    permutation of the interleaved order."""
    mp = N // page

    def make():
        dense = (torch.randn(B, N, DK, dtype=torch.float32, device="cuda", generator=gen) * SCALE).to(BF)
        perm = torch.randperm(B * mp, generator=gen, device="cuda")
        pool = torch.empty(B * mp, page, DK, dtype=BF, device="cuda")
        pool[perm] = dense.view(B, mp, page, DK).permute(1, 0, 2, 3).reshape(B * mp, page, DK)
        return pool, perm.view(mp, B).t().contiguous().to(torch.int32)
    return rotating(make, B * N * DK * 2)


def decode_row(B, T, Hq, ctx, page, gen):
    sets = latent_sets(B, ctx, page, gen)
    sl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    q = (torch.randn(B, T, Hq, DK, device="cuda", generator=gen) * SCALE).to(BF)
    o = torch.empty(B, T, Hq, DC, dtype=BF, device="cuda")
    S, C, need = pkg.fa2_decode_paged_mla_bf16_plan(B, T, Hq, ctx // page, page)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")

    def call(nxt=cycle(sets)):
        pool, bt = nxt()
        pkg.fa2_decode_paged_mla_bf16(q, pool, bt, sl, SCALE, o, None, ws)
    runs = [r["mla"] for r in two_runs({"mla": call})]
    assert bool(torch.isfinite(o.float()).all())
    return runs, len(sets), S, C


def append_row(B, T, ctx, page, gen):
    """{name: [ms run 1, ms run 2]} of the MLA append and of the bf16 varlen append at D = 128, Hkv = 8 on the same tokens."""
    tq, n = B * T, ctx + T
    N = -(-n // page) * page
    mp = N // page
    sl = torch.full((B,), n, dtype=torch.int32, device="cuda")
    cu = torch.arange(0, tq + 1, T, dtype=torch.int32, device="cuda")
    bt = torch.randperm(B * mp, generator=gen, device="cuda").view(mp, B).t().contiguous().to(torch.int32)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=gen).to(BF)  # noqa: E731
    pool = torch.zeros(B * mp, page, DK, dtype=BF, device="cuda")
    c_new, k_pe, q = rnd(tq, DC), rnd(tq, DR), rnd(tq, 16, DK)
    qo = torch.empty_like(q)
    t64 = pkg.kv_append_rope_table(N, DR, device="cuda")
    kp, vp = (torch.zeros(B * mp, 8, page, 128, dtype=BF, device="cuda") for _ in range(2))
    k_new, v_new, q128 = rnd(tq, 8, 128), rnd(tq, 8, 128), rnd(tq, 32, 128)
    qo128 = torch.empty_like(q128)
    t128 = pkg.kv_append_rope_table(N, 128, device="cuda")
    calls = {"mla": lambda: pkg.kv_append_paged_mla_bf16(c_new, k_pe, pool, bt, sl, cu, q, qo, t64, "half"),
             "d128": lambda: pkg.kv_append_paged_varlen_bf16(k_new, v_new, kp, vp, bt, sl, cu, q128, qo128, t128, "half")}
    runs = two_runs(calls)
    return {k: [r[k] for r in runs] for k in calls}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    copy = [copy_rate() for _ in range(2)]
    print("MLA decode over a paged latent cache (bf16 rows [c 512 | k_pe 64], 1152 bytes a token whatever Hq): us per call (launch-inclusive), two "
          "runs of every number and their spread. rd = B context 1152 bytes over the time, TB/s per run; rd/copy = that over hipMemcpyDtoD; "
          "TFLOP/s = 2 B T Hq context (576 + 512) over the time, printed for Hq = 128")
    if copy[0]:
        print("hipMemcpyDtoD of %d MiB, read + written bytes over time: %.2f and %.2f TB/s (spread %.1f%%)" % (COPY_BYTES >> 20, copy[0], copy[1],
                                                                                                           100 * spread(*copy)))
    else:
        print("hipMemcpyDtoD: the vendor yardstick unit is not built, no copy rate")
    print("%-22s %4s %4s %-9s %10s %10s %6s %6s %6s %8s %8s %8s %8s" % ("(B, T, Hq, context)", "page", "sets", "S x C", "us 1", "us 2", "spread",
                                                                        "rd 1", "rd 2", "rd/copy1", "rd/copy2", "TFLOPs 1", "TFLOPs 2"))
    for (B, T, Hq, ctx) in (QUICK_DECODE if a.quick else DECODE):
        for page in PAGES:
            ms, nsets, S, C = decode_row(B, T, Hq, ctx, page, gen)
            rd = [B * ctx * DK * 2 / (m * 1e-3) * 1e-12 for m in ms]
            rc = ["%8.2f" % (r / c) if c else "%8s" % "-" for r, c in zip(rd, copy)]
            tf = ["%8.1f" % (2.0 * B * T * Hq * ctx * (DK + DC) / (m * 1e-3) * 1e-12) if Hq == 128 else "%8s" % "-" for m in ms]
            print("%-22s %4d %4d %-9s %10.1f %10.1f %5.1f%% %6.2f %6.2f %s %s %s %s" % (str((B, T, Hq, ctx)), page, nsets, "%dx%d" % (S, C),
                                                                                         ms[0] * 1e3, ms[1] * 1e3, 100 * spread(*ms), rd[0], rd[1],
                                                                                         rc[0], rc[1], tf[0], tf[1]), flush=True)
            torch.cuda.empty_cache()
    print("append, page 16, rope half with q: us per call, two runs. mla = kv_append_paged_mla_bf16 (a token: 1152 bytes of pool row, Hq 16 x 576 "
          "of q); d128 = kv_append_paged_varlen_bf16 at D = 128, Hkv = 8, Hq = 32 (4096 bytes of K and V rows, 32 x 128 of q)")
    print("%-22s %10s %10s %6s %10s %10s %6s" % ("B x tokens @ context", "mla us 1", "mla us 2", "spread", "d128 us 1", "d128 us 2", "spread"))
    for (B, T, ctx) in APPEND:
        r = append_row(B, T, ctx, 16, gen)
        print("%-22s %10.1f %10.1f %5.1f%% %10.1f %10.1f %5.1f%%" % ("%d x %d @ %d" % (B, T, ctx), r["mla"][0] * 1e3, r["mla"][1] * 1e3,
                                                                    100 * spread(*r["mla"]), r["d128"][0] * 1e3, r["d128"][1] * 1e3,
                                                                    100 * spread(*r["d128"])), flush=True)
        torch.cuda.empty_cache()
