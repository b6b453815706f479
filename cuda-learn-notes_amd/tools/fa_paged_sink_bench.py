"""GPU timing of the attention-sink bf16 paged entries (cuda_learn_notes_amd.fa2_prefill_paged_varlen_window_sink_bf16,
fa2_decode_paged_multi_window_sink_bf16) against their sliding-window siblings without sinks, in the same process on the same pools, in the method
of fa_paged_window_bench.py: launch-inclusive times from one pair of device events around back-to-back calls after a warm-up, every timed window
>= 0.1 s, best of ROUNDS alternating rounds, the pools rotating over sets that together exceed the 256 MiB Infinity Cache. x = sink entry time /
window sibling time. The key loops of the two are the same instructions, so the expectation is x = 1; the yardstick for a row is
the sibling's own spread between two runs of this tool.
  prefill   the six uniform headline shapes and the two ragged batches of fa_paged_window_bench.py behind a context of 4096, W in {1024, None};
  multi     (B, T, context) in {(64, 1, 4096), (8, 4, 16384), (1, 1, 16384)}, W in {1024, None}, the workspaces preallocated;
  gpt-oss   Hq 64, Hkv 8, D 64, W 128: a decode step of 64 sequences and a prefill of 4 x 512 tokens behind a context of 4096.
W = None is a window past the cache (2^31 - 1 for the sibling).
  python fa_paged_sink_bench.py [--skip prefill multi gptoss]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from fa_decode_paged_bench import paged_from, rotating  # noqa: E402
from fa_paged_bf16_bench import batch_name, offsets  # noqa: E402
from fa_prefill_paged_bench import best_of  # noqa: E402
from fa_prefill_paged_varlen_bench import RAGGED, UNIFORM, cycle  # noqa: E402

BF = torch.bfloat16
PAGE = 16
PAST = 2 ** 31 - 1
HEADLINE = (32, 8, 128)  # Hq, Hkv, D of the sibling tool's rows
GPT_OSS = (64, 8, 64)
WINDOWS = (1024, None)
CTX = 4096
MULTI = [(64, 1, 4096), (8, 4, 16384), (1, 1, 16384)]  # (B, T, context)


def pools(B, N, Hkv, D, gen):
    per = 2 * B * Hkv * N * D * 2
    dense = rotating(lambda: tuple(torch.randn(B, Hkv, N, D, dtype=torch.half, device="cuda", generator=gen) for _ in range(2)), per)
    return [(kp.to(BF), vp.to(BF), bt) for (kp, vp, bt) in (paged_from(k, v, PAGE, gen) for (k, v) in dense)]


def line(kind, name, ctx, sets, W, base, sink):
    print("%-8s %-24s %6d %4d %7s %10.1f %10.1f %7.3f" % (kind, name, ctx, sets, "None" if W is None else str(W), base * 1e3, sink * 1e3,
                                                         sink / base), flush=True)


def prefill_row(kind, name, Ts, ctx, shape, windows, gen):
    Hq, Hkv, D = shape
    B, tq = len(Ts), sum(Ts)
    N = -(-(ctx + max(Ts)) // PAGE) * PAGE
    sets = pools(B, N, Hkv, D, gen)
    q = torch.randn(tq, Hq, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
    sinks = torch.randn(Hq, device="cuda", generator=gen) * 2
    o = {(W, s): torch.empty_like(q) for W in windows for s in (0, 1)}
    sl = torch.tensor([ctx + t for t in Ts], dtype=torch.int32, device="cuda")
    cu = torch.tensor(offsets(Ts), dtype=torch.int32, device="cuda")

    def call(key, nxt):
        kp, vp, bt = nxt()
        W, s = key
        if s:
            pkg.fa2_prefill_paged_varlen_window_sink_bf16(q, kp, vp, bt, sl, cu, W, sinks, o[key])
        else:
            pkg.fa2_prefill_paged_varlen_window_bf16(q, kp, vp, bt, sl, cu, PAST if W is None else W, o[key])
    best = best_of({key: (lambda key=key, nxt=cycle(sets): call(key, nxt)) for key in o})
    for W in windows:
        line(kind, name, ctx, len(sets), W, best[(W, 0)], best[(W, 1)])
    for key in o:
        call(key, lambda: sets[0])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in o.values())
    assert all(not torch.equal(o[(W, 0)], o[(W, 1)]) for W in windows)  # the sinks take part


def multi_row(kind, B, T, ctx, shape, windows, gen):
    Hq, Hkv, D = shape
    n = ctx + T
    N = -(-n // PAGE) * PAGE
    sets = pools(B, N, Hkv, D, gen)
    q = torch.randn(B, T, Hq, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
    sinks = torch.randn(Hq, device="cuda", generator=gen) * 2
    sl = torch.full((B,), n, dtype=torch.int32, device="cuda")
    plans = {W: pkg.fa2_decode_paged_multi_window_sink_bf16_plan(B, T, Hq, Hkv, N // PAGE, PAGE, D, W) for W in windows}
    for W in windows:
        assert plans[W] == pkg.fa2_decode_paged_multi_window_bf16_plan(B, T, Hq, Hkv, N // PAGE, PAGE, D, PAST if W is None else W)
    o = {(W, s): torch.empty_like(q) for W in windows for s in (0, 1)}
    ws = {key: torch.empty(max(plans[key[0]][2], 16), dtype=torch.uint8, device="cuda") for key in o}

    def call(key, nxt):
        kp, vp, bt = nxt()
        W, s = key
        if s:
            pkg.fa2_decode_paged_multi_window_sink_bf16(q, kp, vp, bt, sl, W, sinks, o[key], None, ws[key])
        else:
            pkg.fa2_decode_paged_multi_window_bf16(q, kp, vp, bt, sl, PAST if W is None else W, o[key], None, ws[key])
    best = best_of({key: (lambda key=key, nxt=cycle(sets): call(key, nxt)) for key in o})
    for W in windows:
        line(kind, "%s S=%d" % ((B, T), plans[W][0]), ctx, len(sets), W, best[(W, 0)], best[(W, 1)])
    for key in o:
        call(key, lambda: sets[0])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in o.values())
    assert all(not torch.equal(o[(W, 0)], o[(W, 1)]) for W in windows)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip", nargs="*", default=[], choices=["prefill", "multi", "gptoss"])
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    print("attention-sink against sliding-window bf16 paged entries, page %d: us per call (launch-inclusive); x = sink entry time / window sibling "
          "time; prefill and multi rows Hq = %d, Hkv = %d, D = %d; gpt-oss rows Hq = %d, Hkv = %d, D = %d; multi: S = splits" % ((PAGE,) + HEADLINE + GPT_OSS))
    print("%-8s %-24s %6s %4s %7s %10s %10s %7s" % ("entry", "batch", "ctx", "sets", "W", "window us", "sink us", "x"))
    if "multi" not in a.skip:
        for (B, T, ctx) in MULTI:
            multi_row("multi", B, T, ctx, HEADLINE, WINDOWS, gen)
            torch.cuda.empty_cache()
    if "prefill" not in a.skip:
        for (B, T, _) in UNIFORM:
            prefill_row("prefill", "%d x T=%d" % (B, T), [T] * B, CTX, HEADLINE, WINDOWS, gen)
            torch.cuda.empty_cache()
        for Ts in RAGGED:
            prefill_row("prefill", batch_name(Ts), Ts, CTX, HEADLINE, WINDOWS, gen)
            torch.cuda.empty_cache()
    if "gptoss" not in a.skip:
        multi_row("oss-dec", 64, 1, CTX, GPT_OSS, (128,), gen)
        torch.cuda.empty_cache()
        prefill_row("oss-pre", "4 x T=512", [512] * 4, CTX, GPT_OSS, (128,), gen)
