"""GPU timing of the prompt path of multi-head latent attention (cuda_learn_notes_amd.fa2_prefill_varlen_mla_bf16, attn_merge_states_bf16,
kv_gather_paged_mla_bf16) in the method of fa_paged_mla_bench.py: launch-inclusive times from one pair of device events around
back-to-back calls after a warm-up, every timed window >= 0.1 s, best of ROUNDS alternating rounds, the operands rotating over sets that
together exceed the 256 MiB Infinity Cache. Everything is measured TWICE (run 1, run 2, on the same operands) and both are printed with their
spread |a - b| / min(a, b). There is no earlier number for these entries.
  prefill  causal, scale 192^-1/2, every sequence with T new tokens behind `context` keys. The yardstick, in the same run:
           fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16 at D = 128, Hkv = Hq, page 256, no window / sinks / cap, on as many tokens and
           heads. x = mla time / yardstick time; the instruction mix predicts 80 / 64 = 1.25. TFLOP/s = 2 (192 + 128) flops per visible
           (query, key) pair and head over the time.
  merge, gather  beside hipMemcpyDtoD of as many bytes (read + written) from the same run.
  python fa_mla_prefill_bench.py [--quick]"""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_d256_bench import spread, two_runs  # noqa: E402
from fa_paged_anyg_bench import BF, pkg  # noqa: E402
from fa_decode_paged_bench import paged_from, rotating  # noqa: E402
from fa_prefill_paged_bench import timed  # noqa: E402
from fa_prefill_paged_varlen_bench import cycle  # noqa: E402

DN, DR, DQ, DV, DLAT = 128, 64, 192, 128, 576
SCALE = 192 ** -0.5
PAGE = 256
PREFILL = [([4096], 16, 0), ([8192], 16, 0), ([2048] * 4, 128, 0), ([2048], 16, 14336), ([2048, 512, 64, 17], 16, 0)]  # (T per sequence, Hq, context)
QUICK_PREFILL = [([4096], 16, 0), ([2048, 512, 64, 17], 16, 0)]
MERGE = [(4096 * 16, 128), (8192 * 128, 128)]   # (rows, D)
GATHER = [(1, 14336, 256), (4, 2048, 16)]       # (B, tokens per sequence, page)


def cu_of(counts):
    out = [0]
    for c in counts:
        out.append(out[-1] + c)
    return torch.tensor(out, dtype=torch.int32, device="cuda")


def pairs(Ts, ctx):
    """visible (query, key) pairs of the causal batch"""
    return sum(t * ctx + t * (t + 1) // 2 for t in Ts)


def prefill_row(Ts, Hq, ctx, gen):
    B, tq = len(Ts), sum(Ts)
    Ls = [ctx + t for t in Ts]
    tk = sum(Ls)
    cu_q, cu_k = cu_of(Ts), cu_of(Ls)
    rnd = lambda *s: torch.randn(*s, dtype=torch.half, device="cuda", generator=gen).to(BF)  # noqa: E731
    q, o = rnd(tq, Hq, DQ), torch.empty(tq, Hq, DV, dtype=BF, device="cuda")
    sets = rotating(lambda: (rnd(tk, Hq, DN + DV), rnd(tk, DR)), tk * (Hq * (DN + DV) + DR) * 2)
    # the yardstick: paged K / V pools of D = 128 on the same tokens and heads, every sequence padded to whole pages of 256
    N = -(-max(Ls) // PAGE) * PAGE
    ysets = []
    for (k, v) in rotating(lambda: tuple(torch.randn(B, Hq, N, 128, dtype=torch.half, device="cuda", generator=gen) for _ in range(2)),
                           2 * B * Hq * N * 128 * 2):
        kp, vp, bt = paged_from(k, v, PAGE, gen)
        ysets.append((kp.to(BF), vp.to(BF), bt))
    sl = torch.tensor(Ls, dtype=torch.int32, device="cuda")
    q128, o128 = rnd(tq, Hq, 128), torch.empty(tq, Hq, 128, dtype=BF, device="cuda")

    def mla(nxt=cycle(sets)):
        kv, k_pe = nxt()
        pkg.fa2_prefill_varlen_mla_bf16(q, kv, k_pe, cu_q, cu_k, SCALE, o)

    def d128(nxt=cycle(ysets)):
        kp, vp, bt = nxt()
        pkg.fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16(q128, kp, vp, bt, sl, cu_q, None, None, None, None, o128)
    runs = two_runs({"mla": mla, "d128": d128})
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(o128.float()).all())
    return runs, len(sets), len(ysets)


def copy_ms(nbytes):
    """ms of hipMemcpyDtoD of nbytes, rotating over buffers past the Infinity Cache; None in a build without the vendor yardstick unit."""
    from cuda_learn_notes_amd import _loader
    try:
        fn = ctypes.CDLL(_loader.so_path("libcln_amd_vendor.so")).cln_yardstick_copy
    except (OSError, AttributeError):
        return None
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p], ctypes.c_int
    sets = rotating(lambda: tuple(torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(1) for _ in range(2)), 2 * nbytes)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(nxt=cycle(sets)):
        dst, src = nxt()
        assert fn(dst.data_ptr(), src.data_ptr(), nbytes, st) == 0
    return min(timed(call) for _ in range(2))


def merge_row(rows, D, gen):
    mk = lambda: (torch.randn(rows, D, dtype=torch.half, device="cuda", generator=gen).to(BF), torch.randn(rows, device="cuda", generator=gen),  # noqa: E731
                  torch.randn(rows, D, dtype=torch.half, device="cuda", generator=gen).to(BF), torch.randn(rows, device="cuda", generator=gen),
                  torch.empty(rows, D, dtype=BF, device="cuda"), torch.empty(rows, device="cuda"))
    sets = rotating(mk, rows * (3 * D * 2 + 12))

    def call(nxt=cycle(sets)):
        pkg.attn_merge_states_bf16(*nxt())
    return [r["m"] for r in two_runs({"m": call})], rows * (3 * D * 2 + 12)


def gather_row(B, n, page, gen):
    mp = -(-n // page)

    def mk():
        pool = torch.randn(B * mp, page, DLAT, dtype=torch.half, device="cuda", generator=gen).to(BF)
        bt = torch.randperm(B * mp, generator=gen, device="cuda").view(mp, B).t().contiguous().to(torch.int32)
        return pool, bt, torch.empty(B * n, DLAT, dtype=BF, device="cuda")
    sets = rotating(mk, 2 * B * n * DLAT * 2)
    cu = cu_of([n] * B)

    def call(nxt=cycle(sets)):
        pool, bt, out = nxt()
        pkg.kv_gather_paged_mla_bf16(pool, bt, cu, out)
    return [r["g"] for r in two_runs({"g": call})], 2 * B * n * DLAT * 2


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    print("MLA prefill (bf16, key 192 = 128 + 64 dims, value 128, Hkv = Hq), causal, scale 192^-1/2: us per call (launch-inclusive), two runs of "
          "every number and their spread. d128 = fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16 at D = 128, Hkv = Hq, page 256, no window / "
          "sinks / cap, same tokens and heads, same run. x = mla / d128 (the instruction mix predicts 1.25); TFLOP/s = 2 (192 + 128) per visible "
          "pair and head over the mla time")
    print("%-32s %4s %5s %10s %10s %6s %10s %10s %6s %6s %6s %8s %8s" % ("T per sequence @ context", "Hq", "sets", "mla us 1", "mla us 2", "spread",
                                                                        "d128 us 1", "d128 us 2", "spread", "x 1", "x 2", "TFLOPs 1", "TFLOPs 2"))
    for (Ts, Hq, ctx) in (QUICK_PREFILL if a.quick else PREFILL):
        runs, ns, nys = prefill_row(Ts, Hq, ctx, gen)
        m, d = [r["mla"] for r in runs], [r["d128"] for r in runs]
        tf = [2.0 * (DQ + DV) * pairs(Ts, ctx) * Hq / (x * 1e-3) * 1e-12 for x in m]
        name = ("%d x %d" % (len(Ts), Ts[0]) if len(set(Ts)) == 1 else str(Ts)) + " @ %d" % ctx
        print("%-32s %4d %2d/%-2d %10.1f %10.1f %5.1f%% %10.1f %10.1f %5.1f%% %6.3f %6.3f %8.1f %8.1f" % (
            name, Hq, ns, nys, m[0] * 1e3, m[1] * 1e3, 100 * spread(*m), d[0] * 1e3, d[1] * 1e3, 100 * spread(*d), m[0] / d[0], m[1] / d[1],
            tf[0], tf[1]), flush=True)
        torch.cuda.empty_cache()
    print("merge of two states and gather out of the latent pool: us per call, two runs, beside hipMemcpyDtoD of as many bytes (read + written) "
          "from the same run; x = entry / copy")
    print("%-40s %12s %10s %10s %6s %10s %6s" % ("entry", "bytes", "us 1", "us 2", "spread", "copy us", "x"))
    rows = [("attn_merge_states_bf16 rows=%d D=%d" % (r, D), merge_row(r, D, gen)) for (r, D) in (MERGE[:1] if a.quick else MERGE)]
    rows += [("kv_gather_paged_mla_bf16 %d x %d page %d" % g, gather_row(*g, gen)) for g in (GATHER[:1] if a.quick else GATHER)]
    for name, (ms, nbytes) in rows:
        torch.cuda.empty_cache()
        c = copy_ms(nbytes // 2)  # the copy reads and writes nbytes / 2 each
        print("%-40s %12d %10.1f %10.1f %5.1f%% %10s %6s" % (name, nbytes, ms[0] * 1e3, ms[1] * 1e3, 100 * spread(*ms),
                                                           "%.1f" % (c * 1e3) if c else "-", "%.2f" % (min(ms) / c) if c else "-"), flush=True)
