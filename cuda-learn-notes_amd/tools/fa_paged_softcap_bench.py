"""GPU timing of the bf16 paged attention entries with a softmax scale and logit soft-capping
(cuda_learn_notes_amd.fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16[_fp8], fa2_decode_paged_multi_window_sink_softcap_anyg_bf16[_fp8];
DESIGN 4.4.14) in the method of fa_paged_anyg_bench.py, on its shapes: launch-inclusive times from one pair of device events around back-to-back
calls after a warm-up, every timed window >= 0.1 s, best of ROUNDS alternating rounds, the pools rotating over sets that together exceed the
256 MiB Infinity Cache. D = 128, page 16, G = 4 (Hq 32, Hkv 8) and G = 8 (64 / 8), W in {1024, None}; the three decode shapes, the six uniform
prefill batches and the two ragged batches behind a context of 4096. Per row, in the same run on the same pools:
  anyg   the any-G entry (the comparator)
  none   the new entry with softmax_scale = softcap = None; its bits are asserted equal to the any-G entry's.  x_none = none / anyg: parity expected
  scale  the new entry with softmax_scale = 144^-1/2, no cap.                                                   x_scale = scale / anyg: parity expected
  cap    the new entry with softcap = 50, default scale.                                                        x_cap = cap / none: the price of the cap
--quick keeps (64, 1, 4096), (8, 4, 16384) and 4 x T=512.
  python fa_paged_softcap_bench.py [--quick] [--skip bf16 fp8 prefill multi]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_anyg_bench import BF, CTX, D, MULTI, PAGE, QUICK_MULTI, QUICK_PREFILL, SIBLING, WINDOWS, make, pkg  # noqa: E402
from fa_paged_bf16_bench import batch_name, offsets  # noqa: E402
from fa_prefill_paged_bench import best_of  # noqa: E402
from fa_prefill_paged_varlen_bench import RAGGED, UNIFORM, cycle  # noqa: E402

SCALE, CAP = 144 ** -0.5, 50.0
VARIANTS = {"anyg": None, "none": (None, None), "scale": (SCALE, None), "cap": (None, CAP)}


def entries(fp8, new):
    tail = ("softcap_" if new else "") + "anyg_bf16" + ("_fp8" if fp8 else "")
    return (getattr(pkg, "fa2_prefill_paged_varlen_window_sink_" + tail), getattr(pkg, "fa2_decode_paged_multi_window_sink_" + tail),
            getattr(pkg, "fa2_decode_paged_multi_window_sink_" + tail + "_plan"))


def line(fam, kind, name, heads, ctx, sets, W, t):
    print("%-5s %-8s %-20s %3d/%-2d G=%-2d %6d %4d %7s %10.1f %10.1f %10.1f %10.1f %7.3f %7.3f %7.3f" % (
        fam, kind, name, heads[0], heads[1], heads[0] // heads[1], ctx, sets, "None" if W is None else str(W), t["anyg"] * 1e3, t["none"] * 1e3,
        t["scale"] * 1e3, t["cap"] * 1e3, t["none"] / t["anyg"], t["scale"] / t["anyg"], t["cap"] / t["none"]), flush=True)


def prefill_times(fp8, heads, Ts, ctx, gen):
    """{(W, variant): seconds} of len(Ts) sequences of Ts[b] tokens behind ctx keys."""
    Hq, Hkv = heads
    B, tq, N = len(Ts), sum(Ts), -(-(ctx + max(Ts)) // PAGE) * PAGE
    sets, sc = make(fp8, B, N, Hkv, gen)
    q = torch.randn(tq, Hq, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
    sinks = torch.randn(Hq, device="cuda", generator=gen) * 2
    o = {(W, v): torch.empty_like(q) for W in WINDOWS for v in VARIANTS}
    sl = torch.tensor([ctx + t for t in Ts], dtype=torch.int32, device="cuda")
    cu = torch.tensor(offsets(Ts), dtype=torch.int32, device="cuda")

    def call(key, nxt):
        kp, vp, bt = nxt()
        fl = VARIANTS[key[1]]
        entries(fp8, fl is not None)[0](q, kp, vp, bt, sl, cu, *sc, key[0], sinks, *(fl or ()), o[key])
    best = best_of({key: (lambda key=key, nxt=cycle(sets): call(key, nxt)) for key in o})
    for key in o:
        call(key, lambda: sets[0])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in o.values())
    assert all(torch.equal(o[(W, "anyg")], o[(W, "none")]) for W in WINDOWS)  # the any-G entry's bits
    return best, len(sets)


def multi_times(fp8, heads, B, T, ctx, gen):
    Hq, Hkv = heads
    n = ctx + T
    N = -(-n // PAGE) * PAGE
    sets, sc = make(fp8, B, N, Hkv, gen)
    q = torch.randn(B, T, Hq, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
    sinks = torch.randn(Hq, device="cuda", generator=gen) * 2
    sl = torch.full((B,), n, dtype=torch.int32, device="cuda")
    o = {(W, v): torch.empty_like(q) for W in WINDOWS for v in VARIANTS}
    plans = {key: entries(fp8, VARIANTS[key[1]] is not None)[2](B, T, Hq, Hkv, N // PAGE, PAGE, D, key[0]) for key in o}
    ws = {key: torch.empty(max(plans[key][2], 16), dtype=torch.uint8, device="cuda") for key in o}

    def call(key, nxt):
        kp, vp, bt = nxt()
        fl = VARIANTS[key[1]]
        entries(fp8, fl is not None)[1](q, kp, vp, bt, sl, *sc, key[0], sinks, *(fl or ()), o[key], None, ws[key])
    best = best_of({key: (lambda key=key, nxt=cycle(sets): call(key, nxt)) for key in o})
    for key in o:
        call(key, lambda: sets[0])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in o.values())
    assert all(plans[(W, "anyg")] == plans[(W, v)] for W in WINDOWS for v in VARIANTS)
    assert all(torch.equal(o[(W, "anyg")], o[(W, "none")]) for W in WINDOWS)
    return best, len(sets), {W: plans[(W, "anyg")][0] for W in WINDOWS}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--skip", nargs="*", default=[], choices=["bf16", "fp8", "prefill", "multi"])
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    multi = QUICK_MULTI if a.quick else MULTI
    prefill = QUICK_PREFILL if a.quick else [(B, T) for (B, T, _) in UNIFORM]
    ragged = [] if a.quick else RAGGED
    print("softcap bf16 paged attention entries, page %d, D = %d: us per call (launch-inclusive), same pools. anyg = the any-G entry; none = the new "
          "entry without scale and cap (bits asserted equal to anyg); scale = softmax_scale 144^-1/2; cap = softcap 50. x_none = none / anyg, "
          "x_scale = scale / anyg, x_cap = cap / none. multi: S = splits" % (PAGE, D))
    print("%-5s %-8s %-20s %-11s %6s %4s %7s %10s %10s %10s %10s %7s %7s %7s" % ("pools", "entry", "batch", "Hq/Hkv", "ctx", "sets", "W", "anyg us",
                                                                               "none us", "scale us", "cap us", "x_none", "x_scale", "x_cap"))
    for fam in ("bf16", "fp8"):
        if fam in a.skip:
            continue
        fp8 = fam == "fp8"
        if "multi" not in a.skip:
            for (B, T, ctx) in multi:
                for heads in SIBLING:
                    best, n, S = multi_times(fp8, heads, B, T, ctx, gen)
                    for W in WINDOWS:
                        line(fam, "multi", "%s S=%d" % ((B, T), S[W]), heads, ctx, n, W, {v: best[(W, v)] for v in VARIANTS})
                    torch.cuda.empty_cache()
        if "prefill" not in a.skip:
            for Ts in [[T] * B for (B, T) in prefill] + list(ragged):
                name = "%d x T=%d" % (len(Ts), Ts[0]) if len(set(Ts)) == 1 else batch_name(Ts)
                for heads in SIBLING:
                    best, n = prefill_times(fp8, heads, Ts, CTX, gen)
                    for W in WINDOWS:
                        line(fam, "prefill", name, heads, CTX, n, W, {v: best[(W, v)] for v in VARIANTS})
                    torch.cuda.empty_cache()
