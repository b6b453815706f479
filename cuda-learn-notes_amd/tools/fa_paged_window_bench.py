"""GPU timing of the sliding-window bf16 paged entries (cuda_learn_notes_amd.fa2_prefill_paged_varlen_window_bf16,
fa2_decode_paged_multi_window_bf16) against their unwindowed bf16 siblings, all in the same process on the same pools, in the method of
fa_paged_bf16_bench.py: launch-inclusive times from one pair of device events around back-to-back calls after a warm-up, every timed window >= 0.1 s,
best of ROUNDS alternating rounds, the pools rotating over sets that together exceed the 256 MiB Infinity Cache (one set where a single one
already does). The yardsticks are the unwindowed sibling in the same run and the ratio of keys visited: x = windowed time / unwindowed time,
keys = keys the windowed entry walks / keys the unwindowed entry walks (from the kernels' loop bounds, not measured). A windowed entry touches
only the window's part of every pool set, so its rotating footprint is that much smaller than the sibling's.
  multi     (B, T, context) at len_b = context + T, W in {1024, 4096, past the cache}, the workspaces preallocated;
  prefill   the six uniform headline shapes and the two ragged batches, each behind a context of 4096, W in {1024, past the cache}.
  python fa_paged_window_bench.py [--skip prefill multi]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from fa_paged_bf16_bench import MULTI, batch_name, offsets  # noqa: E402
from fa_prefill_paged_bench import best_of  # noqa: E402
from fa_prefill_paged_varlen_bench import D, HKV, HQ, PAGE, RAGGED, UNIFORM, cycle, pools_for  # noqa: E402

BF = torch.bfloat16
G = HQ // HKV
PAST = 2 ** 31 - 1
MULTI_W = (1024, 4096, PAST)
PREFILL_W = (1024, PAST)
PREFILL_CTX = 4096


def bf16_pools(B, N, gen):
    return [(kp.to(BF), vp.to(BF), bt) for (kp, vp, bt) in pools_for(B, N, gen)]


def wname(W):
    return ">=Nmax" if W == PAST else str(W)


def prefill_keys(Ts, ctx, W):
    """Keys the tiles of 128 rows walk, summed over the batch: from align_down(lower edge of the tile's first token, 64) (W = None: from 0) to the
    causal edge of its last, in steps of 64."""
    total = 0
    for T in Ts:
        per = 128 // G  # tokens per tile
        for t0 in range(0, T, per):
            t1 = min(t0 + per, T) - 1
            lo = 0 if W is None else max(0, ctx + t0 + 1 - W) // 64 * 64
            total += -(-(ctx + t1 + 1 - lo) // 64) * 64
    return total


def multi_keys(n, T, W):
    """Keys a sequence of n keys is walked over: from align_down(max(0, n - T - W + 1), 128) (W = None: from 0) to n."""
    return n - (0 if W is None else max(0, n - T - W + 1) // 128 * 128)


def line(kind, name, ctx, sets, W, base, win, keys):
    print("%-8s %-24s %6d %4d %7s %10.1f %10.1f %7.3f %7.3f" % (kind, name, ctx, sets, wname(W), base * 1e3, win * 1e3, win / base, keys), flush=True)


def prefill_row(name, Ts, ctx, gen):
    B, tq = len(Ts), sum(Ts)
    N = -(-(ctx + max(Ts)) // PAGE) * PAGE
    sets = bf16_pools(B, N, gen)
    q = torch.randn(tq, HQ, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
    o = {W: torch.empty_like(q) for W in (None,) + PREFILL_W}
    sl = torch.tensor([ctx + t for t in Ts], dtype=torch.int32, device="cuda")
    cu = torch.tensor(offsets(Ts), dtype=torch.int32, device="cuda")

    def call(W, nxt):
        kp, vp, bt = nxt()
        if W is None:
            pkg.fa2_prefill_paged_varlen_bf16(q, kp, vp, bt, sl, cu, o[W])
        else:
            pkg.fa2_prefill_paged_varlen_window_bf16(q, kp, vp, bt, sl, cu, W, o[W])
    calls = {}
    for W in o:
        calls[W] = (lambda W=W, nxt=cycle(sets): call(W, nxt))
    best = best_of(calls)
    for W in PREFILL_W:
        line("prefill", name, ctx, len(sets), W, best[None], best[W], prefill_keys(Ts, ctx, W) / prefill_keys(Ts, ctx, None))
    for W in o:
        call(W, lambda: sets[0])
    torch.cuda.synchronize()
    assert torch.equal(o[PAST].view(torch.int16), o[None].view(torch.int16)) and bool(torch.isfinite(o[1024].float()).all())


def multi_row(B, T, ctx, gen):
    n = ctx + T
    N = -(-n // PAGE) * PAGE
    sets = bf16_pools(B, N, gen)
    q = torch.randn(B, T, HQ, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
    sl = torch.full((B,), n, dtype=torch.int32, device="cuda")
    plans = {None: pkg.fa2_decode_paged_multi_bf16_plan(B, T, HQ, HKV, N // PAGE, PAGE, D)}
    for W in MULTI_W:
        plans[W] = pkg.fa2_decode_paged_multi_window_bf16_plan(B, T, HQ, HKV, N // PAGE, PAGE, D, W)
    assert plans[PAST] == plans[None]
    o = {W: torch.empty_like(q) for W in plans}
    ws = {W: torch.empty(max(p[2], 16), dtype=torch.uint8, device="cuda") for W, p in plans.items()}

    def call(W, nxt):
        kp, vp, bt = nxt()
        if W is None:
            pkg.fa2_decode_paged_multi_bf16(q, kp, vp, bt, sl, o[W], None, ws[W])
        else:
            pkg.fa2_decode_paged_multi_window_bf16(q, kp, vp, bt, sl, W, o[W], None, ws[W])
    calls = {}
    for W in plans:
        calls[W] = (lambda W=W, nxt=cycle(sets): call(W, nxt))
    best = best_of(calls)
    for W in MULTI_W:
        line("multi", "%s S=%d/%d" % ((B, T), plans[None][0], plans[W][0]), ctx, len(sets), W, best[None], best[W], multi_keys(n, T, W) / multi_keys(n, T, None))
    for W in plans:
        call(W, lambda: sets[0])
    torch.cuda.synchronize()
    assert torch.equal(o[PAST].view(torch.int16), o[None].view(torch.int16)) and bool(torch.isfinite(o[1024].float()).all())


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip", nargs="*", default=[], choices=["prefill", "multi"])
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    print("sliding-window against unwindowed bf16 paged entries, Hq = %d, Hkv = %d, D = %d, page %d: us per call (launch-inclusive); "
          "x = windowed time / unwindowed time; keys = keys walked, windowed / unwindowed; multi: S = splits unwindowed / windowed" % (HQ, HKV, D, PAGE))
    print("%-8s %-24s %6s %4s %7s %10s %10s %7s %7s" % ("entry", "batch", "ctx", "sets", "W", "bf16 us", "window us", "x", "keys"))
    if "multi" not in a.skip:
        for (B, T, ctx) in MULTI:
            multi_row(B, T, ctx, gen)
            torch.cuda.empty_cache()
    if "prefill" not in a.skip:
        for (B, T, _) in UNIFORM:
            prefill_row("%d x T=%d" % (B, T), [T] * B, PREFILL_CTX, gen)
            torch.cuda.empty_cache()
        for Ts in RAGGED:
            prefill_row(batch_name(Ts), Ts, PREFILL_CTX, gen)
            torch.cuda.empty_cache()
