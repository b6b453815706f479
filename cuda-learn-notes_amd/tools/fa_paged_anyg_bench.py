"""GPU timing of the any-group-size bf16 paged attention entries (cuda_learn_notes_amd.fa2_prefill_paged_varlen_window_sink_anyg_bf16[_fp8],
fa2_decode_paged_multi_window_sink_anyg_bf16[_fp8]) in the method of fa_paged_sink_bench.py: launch-inclusive times from one pair
of device events around back-to-back calls after a warm-up, every timed window >= 0.1 s, best of ROUNDS alternating rounds, the pools rotating over
sets that together exceed the 256 MiB Infinity Cache.
  sibling rows  each new entry against its power-of-two sibling in the same run on the same pools, at G = 4 (Hq 32, Hkv 8) and G = 8 (64 / 8),
                D = 128; x = any-G entry time / sibling time. The key loops are the same statements, so the expectation is x = 1; the yardstick
                for a row is the sibling's own spread between two runs of this tool.
  alone rows    G = 7 (28 / 4), G = 5 (40 / 8) and G = 16 (16 / 1), D = 128, which no sibling takes, each beside a G = 8 row of the any-G entry
                with the same Hkv and the same B T Hq (the batch, or the tokens per sequence, scaled by G / 8) at the same context;
                x = time / that G = 8 row's time.
Shapes: the decode (B, T, context) of fa_paged_sink_bench.py, its six uniform prefill batches and its two ragged batches behind a context of
4096, W in {1024, None}. A decode batch whose B G / 8 is no integer has no alone row ((1, 1, 16384)). A ragged batch cannot be scaled by G / 8
token by token, so its alone rows stand beside the SAME batch at G = 8 and the same Hkv: there B T Hq differs by G / 8, and x is to be read
against that ratio. --quick keeps (64, 1, 4096), (8, 4, 16384) and 4 x T=512.
  python fa_paged_anyg_bench.py [--quick] [--skip bf16 fp8 prefill multi]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from fa_paged_bf16_bench import batch_name, offsets  # noqa: E402
from fa_paged_bf16_fp8_bench import pools as both_pools, scales  # noqa: E402
from fa_prefill_paged_bench import best_of  # noqa: E402
from fa_prefill_paged_varlen_bench import RAGGED, UNIFORM, cycle  # noqa: E402

BF = torch.bfloat16
PAGE, D, CTX = 16, 128, 4096
WINDOWS = (1024, None)
SIBLING = [(32, 8), (64, 8)]                       # (Hq, Hkv): G = 4, G = 8
ALONE = [(28, 4), (40, 8), (16, 1)]                # G = 7, 5, 16
MULTI = [(64, 1, 4096), (8, 4, 16384), (1, 1, 16384)]
QUICK_MULTI, QUICK_PREFILL = MULTI[:2], [(4, 512)]


def entries(fp8, anyg):
    tail = ("anyg_" if anyg else "") + "bf16" + ("_fp8" if fp8 else "")
    return (getattr(pkg, "fa2_prefill_paged_varlen_window_sink_" + tail), getattr(pkg, "fa2_decode_paged_multi_window_sink_" + tail),
            getattr(pkg, "fa2_decode_paged_multi_window_sink_" + tail + "_plan"))


def line(fam, kind, name, heads, ctx, sets, W, a, b, what):
    print("%-5s %-8s %-20s %3d/%-2d G=%-2d %6d %4d %7s %10.1f %10.1f %7.3f  %s" % (
        fam, kind, name, heads[0], heads[1], heads[0] // heads[1], ctx, sets, "None" if W is None else str(W), a * 1e3, b * 1e3, b / a, what),
        flush=True)


def make(fp8, B, N, Hkv, gen):
    ks, vs = scales(Hkv)
    sets = [pair[1 if fp8 else 0] for pair in both_pools(B, N, Hkv, D, ks, vs, gen)]
    return sets, ((ks, vs) if fp8 else ())


def prefill_times(fp8, heads, Ts, ctx, variants, gen):
    """{(W, variant): seconds} of len(Ts) sequences of Ts[b] tokens behind ctx keys; variants: anyg flags."""
    Hq, Hkv = heads
    B, tq, N = len(Ts), sum(Ts), -(-(ctx + max(Ts)) // PAGE) * PAGE
    sets, sc = make(fp8, B, N, Hkv, gen)
    q = torch.randn(tq, Hq, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
    sinks = torch.randn(Hq, device="cuda", generator=gen) * 2
    o = {(W, v): torch.empty_like(q) for W in WINDOWS for v in variants}
    sl = torch.tensor([ctx + t for t in Ts], dtype=torch.int32, device="cuda")
    cu = torch.tensor(offsets(Ts), dtype=torch.int32, device="cuda")

    def call(key, nxt):
        kp, vp, bt = nxt()
        entries(fp8, key[1])[0](q, kp, vp, bt, sl, cu, *sc, key[0], sinks, o[key])
    best = best_of({key: (lambda key=key, nxt=cycle(sets): call(key, nxt)) for key in o})
    for key in o:
        call(key, lambda: sets[0])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in o.values())
    if len(variants) == 2:
        assert all(torch.equal(o[(W, False)], o[(W, True)]) for W in WINDOWS)  # the sibling's bits
    return best, len(sets)


def multi_times(fp8, heads, B, T, ctx, variants, gen):
    Hq, Hkv = heads
    n = ctx + T
    N = -(-n // PAGE) * PAGE
    sets, sc = make(fp8, B, N, Hkv, gen)
    q = torch.randn(B, T, Hq, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
    sinks = torch.randn(Hq, device="cuda", generator=gen) * 2
    sl = torch.full((B,), n, dtype=torch.int32, device="cuda")
    o = {(W, v): torch.empty_like(q) for W in WINDOWS for v in variants}
    plans = {key: entries(fp8, key[1])[2](B, T, Hq, Hkv, N // PAGE, PAGE, D, key[0]) for key in o}
    ws = {key: torch.empty(max(plans[key][2], 16), dtype=torch.uint8, device="cuda") for key in o}

    def call(key, nxt):
        kp, vp, bt = nxt()
        entries(fp8, key[1])[1](q, kp, vp, bt, sl, *sc, key[0], sinks, o[key], None, ws[key])
    best = best_of({key: (lambda key=key, nxt=cycle(sets): call(key, nxt)) for key in o})
    for key in o:
        call(key, lambda: sets[0])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in o.values())
    if len(variants) == 2:
        assert all(plans[(W, False)] == plans[(W, True)] and torch.equal(o[(W, False)], o[(W, True)]) for W in WINDOWS)
    return best, len(sets), {W: plans[(W, variants[-1])][0] for W in WINDOWS}


def scaled(x, G):
    """x G / 8 -> x: the batch (or tokens) of the G = 8 row that has the same B T Hq as x at G, with the same Hkv."""
    assert x * G % 8 == 0
    return x * G // 8


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--skip", nargs="*", default=[], choices=["bf16", "fp8", "prefill", "multi"])
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    multi = QUICK_MULTI if a.quick else MULTI
    prefill = QUICK_PREFILL if a.quick else [(B, T) for (B, T, _) in UNIFORM]
    ragged = [] if a.quick else RAGGED
    print("any-G bf16 paged attention entries, page %d, D = %d: us per call (launch-inclusive). sibling rows: a = power-of-two sibling, b = any-G "
          "entry, x = b / a, same pools, bits asserted equal. alone rows: a = the any-G entry at G = 8 with the same Hkv and B T Hq, b = the any-G "
          "entry at the row's G, x = b / a. multi: S = splits" % (PAGE, D))
    print("%-5s %-8s %-20s %-11s %6s %4s %7s %10s %10s %7s" % ("pools", "entry", "batch", "Hq/Hkv", "ctx", "sets", "W", "a us", "b us", "x"))
    for fam in ("bf16", "fp8"):
        if fam in a.skip:
            continue
        fp8 = fam == "fp8"
        if "multi" not in a.skip:
            for (B, T, ctx) in multi:
                for heads in SIBLING:
                    best, n, S = multi_times(fp8, heads, B, T, ctx, (False, True), gen)
                    for W in WINDOWS:
                        line(fam, "multi", "%s S=%d" % ((B, T), S[W]), heads, ctx, n, W, best[(W, False)], best[(W, True)], "sibling")
                    torch.cuda.empty_cache()
                for (Hq, Hkv) in ALONE:
                    G = Hq // Hkv
                    if T * G > 64 or B * G % 8:
                        continue
                    ref, _, _ = multi_times(fp8, (8 * Hkv, Hkv), scaled(B, G), T, ctx, (True,), gen)
                    torch.cuda.empty_cache()
                    best, n, S = multi_times(fp8, (Hq, Hkv), B, T, ctx, (True,), gen)
                    for W in WINDOWS:
                        line(fam, "multi", "%s S=%d" % ((B, T), S[W]), (Hq, Hkv), ctx, n, W, ref[(W, True)], best[(W, True)],
                             "alone; a: B=%d at G=8" % scaled(B, G))
                    torch.cuda.empty_cache()
        if "prefill" not in a.skip:
            for (B, T) in prefill:
                for heads in SIBLING:
                    best, n = prefill_times(fp8, heads, [T] * B, CTX, (False, True), gen)
                    for W in WINDOWS:
                        line(fam, "prefill", "%d x T=%d" % (B, T), heads, CTX, n, W, best[(W, False)], best[(W, True)], "sibling")
                    torch.cuda.empty_cache()
                for (Hq, Hkv) in ALONE:
                    G = Hq // Hkv
                    ref, _ = prefill_times(fp8, (8 * Hkv, Hkv), [scaled(T, G)] * B, CTX, (True,), gen)
                    torch.cuda.empty_cache()
                    best, n = prefill_times(fp8, (Hq, Hkv), [T] * B, CTX, (True,), gen)
                    for W in WINDOWS:
                        line(fam, "prefill", "%d x T=%d" % (B, T), (Hq, Hkv), CTX, n, W, ref[(W, True)], best[(W, True)],
                             "alone; a: T=%d at G=8" % scaled(T, G))
                    torch.cuda.empty_cache()
            for Ts in ragged:
                for heads in SIBLING:
                    best, n = prefill_times(fp8, heads, Ts, CTX, (False, True), gen)
                    for W in WINDOWS:
                        line(fam, "prefill", batch_name(Ts), heads, CTX, n, W, best[(W, False)], best[(W, True)], "sibling")
                    torch.cuda.empty_cache()
                for (Hq, Hkv) in ALONE:
                    ref, _ = prefill_times(fp8, (8 * Hkv, Hkv), Ts, CTX, (True,), gen)
                    torch.cuda.empty_cache()
                    best, n = prefill_times(fp8, (Hq, Hkv), Ts, CTX, (True,), gen)
                    for W in WINDOWS:
                        line(fam, "prefill", batch_name(Ts), (Hq, Hkv), CTX, n, W, ref[(W, True)], best[(W, True)],
                             "alone; a: the same batch at G=8, B T Hq x %.3f" % (8.0 * Hkv / Hq))
                    torch.cuda.empty_cache()
