"""GPU timing of the bf16 paged KV-cache entries (cuda_learn_notes_amd.fa2_prefill_paged_varlen_bf16, fa2_decode_paged_multi_bf16,
kv_append_paged_varlen_bf16) against their fp16 siblings, both in the same process on pools with the same shuffled placement (the bf16 pools are
the fp16 pools converted, the table shared), in the method of fa_prefill_paged_varlen_bench.py: launch-inclusive times from one pair of device
events around back-to-back calls after a warm-up, every timed window >= 0.1 s, best of ROUNDS alternating rounds, the pools rotating over sets that
together exceed the 256 MiB Infinity Cache (one set where a single one already does). x = bf16 time / fp16 time.
  prefill   the six uniform headline shapes (cu_q = T arange(B + 1)) and the two ragged batches over a common context;
  multi     (B, T, context) at len_b = context + T, the workspace preallocated;
  append    the two ragged batches with rope 'half' and q rotated.
  python fa_paged_bf16_bench.py [--skip prefill multi append]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from fa_prefill_paged_bench import best_of  # noqa: E402
from fa_prefill_paged_varlen_bench import D, HKV, HQ, PAGE, RAGGED, RAGGED_CTX, UNIFORM, cycle, pools_for  # noqa: E402

BF = torch.bfloat16
MULTI = [(1, 1, 16384), (64, 1, 4096), (8, 4, 16384)]  # (B, T, context)


def same(run16, run_bf, o16, o_bf):
    """After the timing: both entries once on the first set -- the same attention (or rotation) up to the formats."""
    run16(), run_bf()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o_bf.float()).all()) and float((o_bf.float() - o16.float()).abs().max()) < 0.5


def both(pools):
    """[(fp16 set, bf16 set)]: the same values up to the conversion, the same table."""
    return [((kp, vp, bt), (kp.to(BF), vp.to(BF), bt)) for (kp, vp, bt) in pools]


def line(kind, name, ctx, sets, best):
    print("%-8s %-24s %6d %4d %10.1f %10.1f %7.3f" % (kind, name, ctx, sets, best["fp16"] * 1e3, best["bf16"] * 1e3, best["bf16"] / best["fp16"]), flush=True)


def batch_name(Ts):
    return str(Ts) if len(Ts) <= 4 else "[%d] + [1] x %d" % (Ts[0], len(Ts) - 1)


def offsets(Ts):
    cu = [0]
    for t in Ts:
        cu.append(cu[-1] + t)
    return cu


def prefill_row(name, Ts, ctx, gen):
    B, tq = len(Ts), sum(Ts)
    N = -(-(ctx + max(Ts)) // PAGE) * PAGE
    sets = both(pools_for(B, N, gen))
    q = torch.randn(tq, HQ, D, dtype=torch.half, device="cuda", generator=gen)
    qb = q.to(BF)
    o, ob = torch.empty_like(q), torch.empty_like(qb)
    sl = torch.tensor([ctx + t for t in Ts], dtype=torch.int32, device="cuda")
    cu = torch.tensor(offsets(Ts), dtype=torch.int32, device="cuda")
    nf, nb = cycle(sets), cycle(sets)

    def fp16(nxt=nf):
        kp, vp, bt = nxt()[0]
        pkg.fa2_prefill_paged_varlen(q, kp, vp, bt, sl, cu, o)

    def bf16(nxt=nb):
        kp, vp, bt = nxt()[1]
        pkg.fa2_prefill_paged_varlen_bf16(qb, kp, vp, bt, sl, cu, ob)
    line("prefill", name, ctx, len(sets), best_of({"fp16": fp16, "bf16": bf16}))
    same(lambda: fp16(lambda: sets[0]), lambda: bf16(lambda: sets[0]), o, ob)


def multi_row(B, T, ctx, gen):
    n = ctx + T
    N = -(-n // PAGE) * PAGE
    sets = both(pools_for(B, N, gen))
    q = torch.randn(B, T, HQ, D, dtype=torch.half, device="cuda", generator=gen)
    qb = q.to(BF)
    o, ob = torch.empty_like(q), torch.empty_like(qb)
    sl = torch.full((B,), n, dtype=torch.int32, device="cuda")
    plan = pkg.fa2_decode_paged_multi_plan(B, T, HQ, HKV, N // PAGE, PAGE, D)
    assert plan == pkg.fa2_decode_paged_multi_bf16_plan(B, T, HQ, HKV, N // PAGE, PAGE, D)
    ws, wsb = (torch.empty(max(plan[2], 16), dtype=torch.uint8, device="cuda") for _ in range(2))
    nf, nb = cycle(sets), cycle(sets)

    def fp16(nxt=nf):
        kp, vp, bt = nxt()[0]
        pkg.fa2_decode_paged_multi(q, kp, vp, bt, sl, o, None, ws)

    def bf16(nxt=nb):
        kp, vp, bt = nxt()[1]
        pkg.fa2_decode_paged_multi_bf16(qb, kp, vp, bt, sl, ob, None, wsb)
    line("multi", "%s S=%d" % ((B, T), plan[0]), ctx, len(sets), best_of({"fp16": fp16, "bf16": bf16}))
    same(lambda: fp16(lambda: sets[0]), lambda: bf16(lambda: sets[0]), o, ob)


def append_row(Ts, ctx, gen):
    B, tq = len(Ts), sum(Ts)
    N = -(-(ctx + max(Ts)) // PAGE) * PAGE
    sets = both(pools_for(B, N, gen))
    half = lambda *s: torch.randn(*s, dtype=torch.half, device="cuda", generator=gen)  # noqa: E731
    q, kn, vn = half(tq, HQ, D), half(tq, HKV, D), half(tq, HKV, D)
    qb, knb, vnb = q.to(BF), kn.to(BF), vn.to(BF)
    qo, qob = torch.empty_like(q), torch.empty_like(qb)
    sl = torch.tensor([ctx + t for t in Ts], dtype=torch.int32, device="cuda")
    cu = torch.tensor(offsets(Ts), dtype=torch.int32, device="cuda")
    rope = pkg.kv_append_rope_table(N, D, device="cuda")
    nf, nb = cycle(sets), cycle(sets)

    def fp16(nxt=nf):
        kp, vp, bt = nxt()[0]
        pkg.kv_append_paged_varlen(kn, vn, kp, vp, bt, sl, cu, q, qo, rope, "half")

    def bf16(nxt=nb):
        kp, vp, bt = nxt()[1]
        pkg.kv_append_paged_varlen_bf16(knb, vnb, kp, vp, bt, sl, cu, qb, qob, rope, "half")
    line("append", batch_name(Ts), ctx, len(sets), best_of({"fp16": fp16, "bf16": bf16}))
    same(lambda: fp16(lambda: sets[0]), lambda: bf16(lambda: sets[0]), qo, qob)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip", nargs="*", default=[], choices=["prefill", "multi", "append"])
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    print("bf16 against fp16 paged entries, Hq = %d, Hkv = %d, D = %d, page %d: us per call (launch-inclusive); x = bf16 time / fp16 time" % (HQ, HKV, D, PAGE))
    print("%-8s %-24s %6s %4s %10s %10s %7s" % ("entry", "batch", "ctx", "sets", "fp16 us", "bf16 us", "x"))
    if "prefill" not in a.skip:
        for (B, T, ctx) in UNIFORM:
            prefill_row("%d x T=%d" % (B, T), [T] * B, ctx, gen)
            torch.cuda.empty_cache()
        for Ts in RAGGED:
            for ctx in RAGGED_CTX:
                prefill_row(batch_name(Ts), Ts, ctx, gen)
                torch.cuda.empty_cache()
    if "multi" not in a.skip:
        for (B, T, ctx) in MULTI:
            multi_row(B, T, ctx, gen)
            torch.cuda.empty_cache()
    if "append" not in a.skip:
        for Ts in RAGGED:
            for ctx in RAGGED_CTX:
                append_row(Ts, ctx, gen)
                torch.cuda.empty_cache()
