"""GPU timing of the block-scaled FP8 GEMM (cuda_learn_notes_amd.gemm_fp8_block128_bf16) beside what a caller does without it, in
the method of the other bench tools: launch-inclusive times from one pair of device events around back-to-back calls after a warm-up, every
timed window >= 0.1 s, best of the alternating rounds, the weights rotating over sets that together exceed the 256 MiB Infinity Cache (at most
MAX_SETS sets). Everything is measured TWICE (run 1, run 2, on the same buffers) and both are printed; hipMemcpyDtoD is taken in the same run.
  M x (N, K), us per call:
    fp8      gemm_fp8_block128_bf16 on e4m3 codes with DeepSeek-V3's block scales (the form by M alone: skinny for M <= 64, else tile)
    dq+mm    what a caller does today: torch dequantise of the weight to bf16 (codes -> bf16, times the expanded block scales) + torch.matmul
    mm       torch.matmul alone on the weight already dequantised to bf16 (twice the weight bytes, a second copy of the model)
    hgemm    the library's best-dispatch fp16 HGEMM, TN, at the same M, N, K ("-" where it refuses the shape)
    wt TB/s  M <= 64: N K weight bytes over the fp8 time
  and at M = 64 the tile form through the one public shape that runs it next door, M = 65 (the entry has no form override).
  python gemm_fp8_block128_bench.py [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_d256_bench import COPY_BYTES, copy_rate, spread  # noqa: E402
from fa_paged_anyg_bench import BF, pkg  # noqa: E402
from fa_decode_paged_bench import best_of, rotating  # noqa: E402
from fa_prefill_paged_varlen_bench import cycle  # noqa: E402
from cuda_learn_notes_amd import bench_utils as bu  # noqa: E402

F8 = torch.float8_e4m3fn
MS = (1, 16, 64, 128, 512, 4096)
NK = ((1536, 7168), (576, 7168), (24576, 1536), (32768, 512), (7168, 16384), (4096, 7168), (7168, 2048))
QUICK_MS, QUICK_NK = (1, 64, 512), ((1536, 7168), (7168, 2048))


def codes(rows, cols, gen):
    """e4m3fn [rows,cols]: finite codes (bytes below 0x78, and their negatives)."""
    c = torch.randint(0, 0x78, (rows, cols), dtype=torch.uint8, device="cuda", generator=gen)
    c |= torch.randint(0, 2, (rows, cols), dtype=torch.uint8, device="cuda", generator=gen) << 7
    return c.view(F8)


def rows_of(N, K, ms, gen):
    kb, nb = K // 128, -(-N // 128)
    sb = torch.rand(nb, kb, device="cuda", generator=gen) * 1e-3 + 1e-4
    sbn = sb.repeat_interleave(128, dim=0)[:N].to(BF)[:, :, None]  # the block scales expanded over N, once

    def dequant(b):
        return (b.to(BF).view(N, kb, 128) * sbn).view(N, K)

    def make():
        b = codes(N, K, gen)
        w = dequant(b)
        return b, w, w.to(torch.half).view(K, N)  # the TN operand of the HGEMM keeps the [K,N] shape over the [N,K] memory
    sets = rotating(make, N * K)
    hg, stride = pkg.hgemm_lib(), bu.make_block_swizzle_stride(N, K)
    for M in ms:
        a = codes(M, K, gen)
        sa = torch.rand(M, kb, device="cuda", generator=gen) * 1e-2 + 1e-3
        x = (a.to(BF).view(M, kb, 128) * sa.to(BF)[:, :, None]).view(M, K)
        xh = x.to(torch.half)
        out, oh = torch.empty(M, N, dtype=BF, device="cuda"), torch.empty(M, N, dtype=torch.half, device="cuda")

        def fp8(nxt=cycle(sets)):
            pkg.gemm_fp8_block128_bf16(a, sa, nxt()[0], sb, out)

        def dqmm(nxt=cycle(sets)):
            torch.matmul(x, dequant(nxt()[0]).t(), out=out)

        def mm(nxt=cycle(sets)):
            torch.matmul(x, nxt()[1].t(), out=out)

        def hgemm(nxt=cycle(sets)):
            hg.hgemm_mma_m16n8k16_mma2x4_warp4x4x2_stages_dsmem_tn_swizzle_x4(xh, nxt()[2], oh, 2, True, stride)
        calls = {"fp8": fp8, "dq+mm": dqmm, "mm": mm}
        try:
            hgemm()
            calls["hgemm"] = hgemm
        except RuntimeError:
            pass
        if M == 64:
            a65, sa65, out65 = codes(65, K, gen), torch.rand(65, kb, device="cuda", generator=gen) * 1e-2 + 1e-3, torch.empty(65, N, dtype=BF, device="cuda")

            def tile65(nxt=cycle(sets)):
                pkg.gemm_fp8_block128_bf16(a65, sa65, nxt()[0], sb, out65)
            calls["tile"] = tile65
        runs = [best_of(calls, rounds=2) for _ in range(2)]
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.float()).all())
        cell = lambda n: "%9.1f %9.1f" % tuple(r[n] * 1e3 for r in runs) if n in calls else "%9s %9s" % ("-", "-")  # noqa: E731
        bw = "%6.2f %6.2f" % tuple(N * K / (r["fp8"] * 1e-3) * 1e-12 for r in runs) if M <= 64 else "%6s %6s" % ("", "")
        tf = "%6.0f" % (2.0 * M * N * K / (min(r["fp8"] for r in runs) * 1e-3) * 1e-12)
        print("%5d %6d %6d %4d %s %s %s %s %s %s %5.1f%%%s" % (M, N, K, len(sets), cell("fp8"), cell("dq+mm"), cell("mm"), cell("hgemm"), bw, tf,
                                                             100 * spread(runs[0]["fp8"], runs[1]["fp8"]),
                                                             "   tile form at M = 65: " + cell("tile") if "tile" in calls else ""), flush=True)
    del sets
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    copy = [copy_rate() for _ in range(2)]
    print("gemm_fp8_block128_bf16 beside torch dequantise + matmul, torch.matmul on bf16 weights and the fp16 HGEMM (TN): us per call "
          "(launch-inclusive), two runs of every number, the calls alternating in every round; wt TB/s = N K weight bytes over the fp8 time "
          "(M <= 64); TF = 2 M N K over the better fp8 time; spread = between the two fp8 runs")
    if copy[0]:
        print("hipMemcpyDtoD of %d MiB, read + written bytes over time: %.2f and %.2f TB/s (spread %.1f%%)" % (COPY_BYTES >> 20, copy[0], copy[1],
                                                                                                           100 * spread(*copy)))
    else:
        print("hipMemcpyDtoD: the vendor yardstick unit is not built, no copy rate")
    print("%5s %6s %6s %4s %9s %9s %9s %9s %9s %9s %9s %9s %6s %6s %6s %6s" % ("M", "N", "K", "sets", "fp8 1", "fp8 2", "dq+mm 1", "dq+mm 2", "mm 1", "mm 2",
                                                                          "hgemm 1", "hgemm 2", "wt 1", "wt 2", "TF", "spread"))
    for N, K in (QUICK_NK if args.quick else NK):
        rows_of(N, K, QUICK_MS if args.quick else MS, gen)
