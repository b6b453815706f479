"""GPU timing of the causal attention entry (cuda_learn_notes_amd.fa2_fwd_causal, cln_fa2_fwd_causal) against the plain
flash_attn_mma_stages_split_q_shared_qkv on the same shape, torch scaled_dot_product_attention(is_causal=True) and, with
--orders, the three launch orders of the causal kernel (probe library, M16X_ORDER_*).
FLOPs of a causal launch are counted as 2 B H N^2 D (half the plain count, 4 B H N^2 D).
Device events around back-to-back launches after a warm-up; every timed window is >= 0.1 s; the rows of one shape alternate
causal / plain / SDPA over three rounds and report the best round.
  python fa_causal_bench.py [--orders]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from cuda_learn_notes_amd import bench_utils as bu, host  # noqa: E402

SHAPES = [(4, 8, 2048, 64), (2, 32, 4096, 64), (2, 32, 4096, 128), (1, 32, 8192, 128)]


def timed(fn):
    """ms per launch: iterations sized so that the window is >= 0.1 s."""
    bu.prewarm(fn, 0.1)
    ms = bu.time_region_events(fn, 5)
    iters = max(10, int(100.0 / max(ms, 1e-3)) + 1)
    return bu.time_region_events(fn, iters)


def main():
    orders = "--orders" in sys.argv
    fa = pkg.flash_attn_lib()
    sdpa = torch.nn.functional.scaled_dot_product_attention
    print("causal FLOPs = 2 B H N^2 D; plain FLOPs = 4 B H N^2 D; times in ms (best of 3 alternating rounds)")
    print("%-20s %9s %7s %9s %7s %7s %9s %7s %8s" % ("shape", "causal", "TF", "plain", "TF", "c/p", "sdpa_c", "TF", "c/sdpa"))
    for shape in SHAPES:
        B, H, N, D = shape
        torch.manual_seed(0)
        q, k, v = (torch.randn(B, H, N, D, dtype=torch.half, device="cuda") for _ in range(3))
        oc, op = torch.zeros_like(q), torch.zeros_like(q)
        calls = {"causal": lambda: pkg.fa2_fwd_causal(q, k, v, oc, 2),
                 "plain": lambda: fa.flash_attn_mma_stages_split_q_shared_qkv(q, k, v, op, 2),
                 "sdpa": lambda: sdpa(q, k, v, is_causal=True)}
        best = {n: float("inf") for n in calls}
        for _ in range(3):
            for n, f in calls.items():
                best[n] = min(best[n], timed(f))
        torch.cuda.synchronize()
        ref = sdpa(q, k, v, is_causal=True)
        err = (oc.float() - ref.float()).abs().max().item()
        fc, fp = 2.0 * B * H * N * N * D, 4.0 * B * H * N * N * D
        print("%-20s %9.4f %7.1f %9.4f %7.1f %7.3f %9.4f %7.1f %8.3f   max|causal - sdpa| %.2e" % (
            str(shape), best["causal"], fc / best["causal"] * 1e-9, best["plain"], fp / best["plain"] * 1e-9, best["causal"] / best["plain"],
            best["sdpa"], fc / best["sdpa"] * 1e-9, best["causal"] / best["sdpa"], err), flush=True)
    if orders:
        shape = (2, 32, 4096, 128)
        q, k, v = (torch.randn(*shape, dtype=torch.half, device="cuda") for _ in range(3))
        o, ref = torch.zeros_like(q), torch.zeros_like(q)
        pkg.fa2_fwd_causal(q, k, v, ref, 2)
        names = {0: "plain (ascending row blocks per head)", 1: "heaviest first (product)", 2: "descending row blocks per head"}
        best = {i: float("inf") for i in names}
        for _ in range(3):
            for i in names:
                best[i] = min(best[i], timed(lambda: host.fa2_variant((8, 0, 0, 2700 + i), q, k, v, o)))
        torch.cuda.synchronize()
        host.fa2_variant((8, 0, 0, 2701), q, k, v, o)
        torch.cuda.synchronize()
        for i, nm in names.items():
            print("ORDER %-20s %-40s %9.4f ms %7.1f TF" % (str(shape), nm, best[i], 2.0 * shape[0] * shape[1] * shape[2] ** 2 * shape[3] / best[i] * 1e-9))
        print("ORDER heaviest-first probe == product output: %s" % bool(torch.equal(o, ref)))


if __name__ == "__main__":
    main()
