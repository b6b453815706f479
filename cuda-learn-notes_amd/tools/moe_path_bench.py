"""GPU timing of the MoE token path (cuda_learn_notes_amd.moe_route_topk, moe_sort, moe_dispatch_fp8_block128_bf16, moe_combine_bf16; DESIGN
4.4.33) beside the torch chain each entry replaces, on the same inputs: launch-inclusive us per call from one pair of device events around
back-to-back calls after a warm-up, every number measured TWICE (run 1 / run 2) with the spread of the glue row. Per shape (T, E, k, K, N) and
id pattern (softmax logits whose winners are balanced, or Zipf over the experts):
    route     moe_route_topk                 | torch: softmax, topk, renormalise
    sort      moe_sort (1 or 3 launches)     | torch: stable argsort, bincount, cumsum, inverse scatter
    dispatch  moe_dispatch_fp8_block128_bf16 | torch: index_select of x, quant_fp8_block128_bf16   (K % 128 != 0: the MXFP8 pair)
    combine   moe_combine_bf16               | torch: index y by pos, multiply, sum, cast
    glue      the four entries back to back  | the four torch chains back to back
  GB/s: the bytes an entry must move (dispatch: 2 K read + K + K / 32 written a row; combine: 2 N k read + 2 N written a token) over its better
  time; the first line is a device-to-device copy of 1 GiB for comparison.
  python moe_path_bench.py [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_anyg_bench import BF, pkg  # noqa: E402

F8, I32 = torch.float8_e4m3fn, torch.int32
SHAPES = ((256, 8, 7168, 7168), (128, 4, 2880, 2880))  # (E, k, K, N): DeepSeek-V3, gpt-oss
TS = (64, 4096, 32768)


def timed(fn, min_s=0.05):
    """us per call: warm up, size the window to >= min_s, one event pair around it."""
    for _ in range(3):
        fn()
    n, (e0, e1) = 8, (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    while True:
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1e3 * min_s or n >= 1 << 16:
            return 1e3 * ms / n
        n *= 4


def logits_for(T, E, pattern, gen):
    lg = torch.randn(T, E, device="cuda", generator=gen)
    if pattern == "zipf":
        lg += 2.0 * torch.log(1.0 / torch.arange(1, E + 1, device="cuda"))[None, :]
    return lg.to(BF)


def bench(c, T, E, k, K, N, pattern, gen):
    n = T * k
    lg, x = logits_for(T, E, pattern, gen), torch.randn(T, K, device="cuda", generator=gen).to(BF)
    ids, w, pos = (torch.empty(T, k, dtype=d, device="cuda") for d in (I32, torch.float32, I32))
    off, src = torch.empty(E + 1, dtype=I32, device="cuda"), torch.empty(n, dtype=I32, device="cuda")
    ws = torch.empty(max(c.moe_sort_plan(n, E)[2], 4), dtype=torch.uint8, device="cuda")
    mx = K % 128 != 0  # hidden 2880: the MXFP8 pair (moe_dispatch_mxfp8_bf16 beside quant_mxfp8_bf16)
    dispatch, quant = (c.moe_dispatch_mxfp8_bf16, c.quant_mxfp8_bf16) if mx else (c.moe_dispatch_fp8_block128_bf16, c.quant_fp8_block128_bf16)
    codes = torch.empty(n, K, dtype=F8, device="cuda")
    scales = torch.empty(n, K // 32, dtype=torch.uint8, device="cuda").view(torch.float8_e8m0fnu) if mx else torch.empty(n, K // 128, device="cuda")
    y, out = torch.randn(n, N, device="cuda", generator=gen).to(BF), torch.empty(T, N, dtype=BF, device="cuda")
    xg = torch.empty(n, K, dtype=BF, device="cuda")
    ours = {"route": lambda: c.moe_route_topk(lg, ids, w), "sort": lambda: c.moe_sort(ids, E, off, src, pos, ws),
            "dispatch": lambda: dispatch(x, src, k, codes, scales), "combine": lambda: c.moe_combine_bf16(y, pos, w, out)}
    for f in ours.values():
        f()
    ids64, order, posl = ids.long(), src.long().clamp_min(0), pos.long().clamp_min(0)

    def t_route():
        p, i = torch.topk(torch.softmax(lg.float(), dim=-1), k, dim=-1)
        return p / p.sum(dim=-1, keepdim=True), i

    def t_sort():
        o = torch.argsort(ids64.flatten(), stable=True)
        inv = torch.empty_like(o)
        inv[o] = torch.arange(n, device="cuda")
        return o, inv, torch.cumsum(torch.bincount(ids64.flatten(), minlength=E), 0)

    def t_dispatch():
        torch.index_select(x, 0, order // k, out=xg)
        quant(xg, codes, scales)

    def t_combine():
        return (y[posl].float() * w[:, :, None]).sum(dim=1).to(BF)
    theirs = {"route": t_route, "sort": t_sort, "dispatch": t_dispatch, "combine": t_combine}
    for side in (ours, theirs):
        side["glue"] = lambda side=dict(side): [f() for f in side.values()]
    need = {"dispatch": n * (3 * K + K // 32), "combine": T * N * 2 * (k + 1)}
    for name in ("route", "sort", "dispatch", "combine", "glue"):
        a, b = [timed(ours[name]) for _ in range(2)], [timed(theirs[name]) for _ in range(2)]
        rate = "%7.0f GB/s" % (need[name] / min(a) * 1e-3) if name in need else ""
        print("T=%-6d E=%-4d k=%d K=%-5d N=%-5d %-8s %-9s ours %9.1f %9.1f us  torch %9.1f %9.1f us  x%5.2f  spread %4.1f%% %s"
              % (T, E, k, K, N, pattern, name, a[0], a[1], b[0], b[1], min(b) / min(a), 100 * abs(a[0] - a[1]) / min(a), rate), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="T = 64 and 4096 only")
    args = ap.parse_args()
    c, gen = pkg, torch.Generator(device="cuda").manual_seed(0)
    a, b = torch.empty(1 << 30, dtype=torch.uint8, device="cuda"), torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        print("device-to-device copy of 1 GiB: %.0f GB/s (read + write)" % (2 * (1 << 30) / timed(lambda: b.copy_(a)) * 1e-3), flush=True)
    del a, b
    for E, k, K, N in SHAPES:
        for T in TS[:2] if args.quick else TS:
            for pattern in ("balanced", "zipf"):
                bench(c, T, E, k, K, N, pattern, gen)


if __name__ == "__main__":
    main()
