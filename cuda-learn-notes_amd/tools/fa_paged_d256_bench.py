"""GPU timing of the head-dim-256 bf16 paged attention entries (cuda_learn_notes_amd.fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16,
fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16) in the method of fa_paged_softcap_bench.py, on its shapes: launch-inclusive
times from one pair of device events around back-to-back calls after a warm-up, every timed window >= 0.1 s, best of ROUNDS alternating rounds,
the pools rotating over sets that together exceed the 256 MiB Infinity Cache. Page 16, Hkv 8, G = 2 (Hq 16) and G = 4 (Hq 32), W in {None, 1024,
4096}, cap in {None, 50}; the three decode shapes (T G <= 32), the six uniform prefill batches and the two ragged batches behind a context of 4096.
There is no earlier D = 256 number. Per row, measured in the same run, two yardsticks:
  d128   the D = 128 softcap entry at the same B, T, Hq, Hkv, context, W and page (pools of their own with the same geometry). It moves half the
         K / V bytes and does half the flops: x = d256 / d128, and 2.0 is the reference point.
  copy   decode rows only: the K / V bytes the row must read -- 2 B Hkv min(len, W + T - 1) 256 2 -- over its time, against hipMemcpyDtoD of
         COPY_BYTES measured here (bytes read + bytes written over time); rd/copy is the ratio of the two rates.
Everything is measured TWICE (run 1, run 2, on the same pools) and both are printed with their spread |a - b| / min(a, b).
--quick keeps (64, 1, 4096), (8, 4, 16384) and 4 x T=512.
  python fa_paged_d256_bench.py [--quick] [--skip prefill multi]"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_anyg_bench import BF, CTX, MULTI, PAGE, QUICK_MULTI, QUICK_PREFILL, pkg  # noqa: E402
from fa_paged_bf16_bench import batch_name, offsets  # noqa: E402
from fa_decode_paged_bench import paged_from, rotating  # noqa: E402
from fa_prefill_paged_bench import best_of, timed  # noqa: E402
from fa_prefill_paged_varlen_bench import RAGGED, UNIFORM, cycle  # noqa: E402

HKV, GROUPS = 8, (2, 4)
WINDOWS, CAPS = (None, 1024, 4096), (None, 50.0)
COPY_BYTES = 1 << 30
NAMES = {256: ("fa2_prefill_paged_varlen_window_sink_softcap_anyg_d256_bf16", "fa2_decode_paged_multi_window_sink_softcap_anyg_d256_bf16"),
         128: ("fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16", "fa2_decode_paged_multi_window_sink_softcap_anyg_bf16")}


def pools_for(B, N, D, gen):
    """Rotating sets of bf16 (k_pages, v_pages, block_table) at head dim D: randn rows, shuffled placement."""
    per = 2 * B * HKV * N * D * 2
    dense = rotating(lambda: tuple(torch.randn(B, HKV, N, D, dtype=torch.half, device="cuda", generator=gen) for _ in range(2)), per)
    out = []
    for (k, v) in dense:
        kp, vp, bt = paged_from(k, v, PAGE, gen)
        out.append((kp.to(BF), vp.to(BF), bt))
    return out


def copy_rate():
    """TB/s of hipMemcpyDtoD over COPY_BYTES (read + written bytes over time), or None in a build without the vendor yardstick unit."""
    from cuda_learn_notes_amd import _loader
    try:
        lib = ctypes.CDLL(_loader.so_path("libcln_amd_vendor.so"))
        fn = lib.cln_yardstick_copy
    except (OSError, AttributeError):
        return None
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int
    bufs = [torch.empty(COPY_BYTES, dtype=torch.uint8, device="cuda").fill_(i) for i in range(4)]  # two pairs: 4 GiB past the Infinity Cache
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    i = [0]

    def call():
        i[0] ^= 2
        assert fn(bufs[i[0] + 1].data_ptr(), bufs[i[0]].data_ptr(), COPY_BYTES, st) == 0
    ms = min(timed(call) for _ in range(2))
    return 2 * COPY_BYTES / (ms * 1e-3) * 1e-12


def two_runs(calls):
    """[{name: ms} of run 1, of run 2]"""
    return [best_of(calls) for _ in range(2)]


def spread(a, b):
    return abs(a - b) / min(a, b)


def prefill_rows(G, Ts, ctx, gen):
    Hq = HKV * G
    B, tq, N = len(Ts), sum(Ts), -(-(ctx + max(Ts)) // PAGE) * PAGE
    sl = torch.tensor([ctx + t for t in Ts], dtype=torch.int32, device="cuda")
    cu = torch.tensor(offsets(Ts), dtype=torch.int32, device="cuda")
    sinks = torch.randn(Hq, device="cuda", generator=gen) * 2
    calls, keep, nsets = {}, [], {}
    for D in (256, 128):
        sets = pools_for(B, N, D, gen)
        nsets[D] = len(sets)
        q = torch.randn(tq, Hq, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
        o = torch.empty_like(q)
        fn = getattr(pkg, NAMES[D][0])
        keep.append((sets, q, o))
        for W in WINDOWS:
            for cap in CAPS:
                def call(fn=fn, q=q, o=o, W=W, cap=cap, nxt=cycle(sets)):
                    kp, vp, bt = nxt()
                    fn(q, kp, vp, bt, sl, cu, W, sinks, None, cap, o)
                calls[(D, W, cap)] = call
    runs = two_runs(calls)
    assert all(bool(torch.isfinite(o.float()).all()) for (_, _, o) in keep)
    return runs, nsets


def multi_rows(G, B, T, ctx, gen):
    Hq = HKV * G
    n = ctx + T
    N = -(-n // PAGE) * PAGE
    sl = torch.full((B,), n, dtype=torch.int32, device="cuda")
    sinks = torch.randn(Hq, device="cuda", generator=gen) * 2
    calls, keep, nsets, splits = {}, [], {}, {}
    for D in (256, 128):
        sets = pools_for(B, N, D, gen)
        nsets[D] = len(sets)
        q = torch.randn(B, T, Hq, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
        o = torch.empty_like(q)
        fn, plan = getattr(pkg, NAMES[D][1]), getattr(pkg, NAMES[D][1] + "_plan")
        keep.append((sets, q, o))
        for W in WINDOWS:
            S, _, need = plan(B, T, Hq, HKV, N // PAGE, PAGE, D, W)
            splits[(D, W)] = S
            ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
            for cap in CAPS:
                def call(fn=fn, q=q, o=o, W=W, cap=cap, ws=ws, nxt=cycle(sets)):
                    kp, vp, bt = nxt()
                    fn(q, kp, vp, bt, sl, W, sinks, None, cap, o, None, ws)
                calls[(D, W, cap)] = call
    runs = two_runs(calls)
    assert all(bool(torch.isfinite(o.float()).all()) for (_, _, o) in keep)
    return runs, nsets, splits


def line(kind, name, G, ctx, nsets, W, cap, runs, extra=""):
    a = [r[(256, W, cap)] for r in runs]
    b = [r[(128, W, cap)] for r in runs]
    print("%-8s %-22s %2d/%d G=%d %6d %d/%d %5s %4s %10.1f %10.1f %5.1f%% %10.1f %10.1f %5.1f%% %6.2f %6.2f%s" % (
        kind, name, HKV * G, HKV, G, ctx, nsets[256], nsets[128], "None" if W is None else str(W), "-" if cap is None else "%g" % cap,
        a[0] * 1e3, a[1] * 1e3, 100 * spread(*a), b[0] * 1e3, b[1] * 1e3, 100 * spread(*b), a[0] / b[0], a[1] / b[1], extra), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--skip", nargs="*", default=[], choices=["prefill", "multi"])
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    multi = QUICK_MULTI if a.quick else MULTI
    prefill = QUICK_PREFILL if a.quick else [(B, T) for (B, T, _) in UNIFORM]
    ragged = [] if a.quick else RAGGED
    copy = [copy_rate() for _ in range(2)]
    print("head dim 256 bf16 paged attention entries, page %d, Hkv %d: us per call (launch-inclusive), two runs of every number and their spread. "
          "d256 = the new entry, d128 = the D = 128 softcap entry at the same shape; x = d256 / d128 per run (2.0 = half the bytes and flops "
          "there). multi: S = the splits of the two plans; rd = the K / V bytes the row must read over the d256 time, TB/s per run; rd/copy = that "
          "over hipMemcpyDtoD" % (PAGE, HKV))
    if copy[0]:
        print("hipMemcpyDtoD of %d MiB, read + written bytes over time: %.2f and %.2f TB/s (spread %.1f%%)" % (COPY_BYTES >> 20, copy[0], copy[1],
                                                                                                           100 * spread(*copy)))
    else:
        print("hipMemcpyDtoD: the vendor yardstick unit is not built, no copy rate")
    print("%-8s %-22s %-8s %6s %4s %5s %4s %10s %10s %6s %10s %10s %6s %6s %6s" % ("entry", "batch", "Hq/Hkv", "ctx", "sets", "W", "cap", "d256 us 1",
                                                                                 "d256 us 2", "spread", "d128 us 1", "d128 us 2", "spread", "x 1", "x 2"))
    if "multi" not in a.skip:
        for (B, T, ctx) in multi:
            for G in GROUPS:
                runs, nsets, S = multi_rows(G, B, T, ctx, gen)
                for W in WINDOWS:
                    for cap in CAPS:
                        keys = ctx + T if W is None else min(ctx + T, W + T - 1)
                        rd = [2 * B * HKV * keys * 256 * 2 / (r[(256, W, cap)] * 1e-3) * 1e-12 for r in runs]
                        extra = "  S=%d/%d rd %.2f %.2f TB/s" % (S[(256, W)], S[(128, W)], rd[0], rd[1])
                        if copy[0]:
                            extra += " rd/copy %.2f %.2f" % (rd[0] / copy[0], rd[1] / copy[1])
                        line("multi", str((B, T)), G, ctx, nsets, W, cap, runs, extra)
                torch.cuda.empty_cache()
    if "prefill" not in a.skip:
        for Ts in [[T] * B for (B, T) in prefill] + list(ragged):
            name = "%d x T=%d" % (len(Ts), Ts[0]) if len(set(Ts)) == 1 else batch_name(Ts)
            for G in GROUPS:
                runs, nsets = prefill_rows(G, Ts, CTX, gen)
                for W in WINDOWS:
                    for cap in CAPS:
                        line("prefill", name, G, CTX, nsets, W, cap, runs)
                torch.cuda.empty_cache()
