"""GPU timing of paged decode attention over an FP8 (e4m3fn) KV cache (cuda_learn_notes_amd.fa2_decode_paged_fp8, cln_fa2_decode_paged_fp8)
against fa2_decode_paged on an fp16 pool of the same logical content (the dequantised values, which fp16 holds exactly), in the same process,
and of the quantising append kv_append_paged_fp8 against kv_append_paged. The method is that of fa_decode_paged_bench.py: the pages of a pool
are shuffled with the sequences interleaved; times are launch-inclusive (for a split plan: both kernels); the pools rotate over sets that
together exceed the 256 MiB Infinity Cache -- counted on the FP8 bytes alone, 640 MiB of them on every row (one set where a single one already
is that large), so both entries read from HBM;
one pair of device events around back-to-back calls after a warm-up, every timed window >= 0.1 s, best of 3 alternating rounds.
Bytes of a call: 2 len B Hkv D element bytes -- the K and V rows below the lengths, once per KV head. ratio = fp16 time / fp8 time; the byte
ratio is 2.
  python fa_decode_paged_fp8_bench.py [--quick]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from cuda_learn_notes_amd import bench_utils as bu  # noqa: E402

BS, HKV, GS, DS, LENS, PAGES = (1, 8, 64), 8, (1, 4, 8), (64, 128), (1024, 4096, 16384, 32768), (16, 128)
ROTATE_BYTES = 640 << 20
MAX_SETS = 700  # 640 sets of 1 MiB at (B, len, D) = (1, 1024, 64): the FP8 sets alone exceed the cache on every row
F8 = torch.float8_e4m3fn


def timed(fn):
    bu.prewarm(fn, 0.05)
    ms = bu.time_region_events(fn, 5)
    return bu.time_region_events(fn, max(10, int(100.0 / max(ms, 1e-3)) + 1))


def best_of(calls, rounds=3):
    best = {n: float("inf") for n in calls}
    for _ in range(rounds):
        for n, f in calls.items():
            best[n] = min(best[n], timed(f))
    torch.cuda.synchronize()
    return best


def code_values():
    """fp32 [256] on the GPU: the value of every e4m3fn code, from the CPU conversion (no FP8 arithmetic of torch runs on the GPU here)."""
    return torch.arange(256, dtype=torch.uint8).view(F8).float().cuda()


def pool_pair(P, page, D, scales, lut, gen):
    """(k8, v8 e4m3fn, k16, v16 fp16) [P,HKV,page,D]: random codes of magnitude below 2 (no NaN code), and their values times the head's scale."""
    out8, out16 = [], []
    for _ in range(2):
        codes = torch.randint(0, 0x40, (P, HKV, page, D), dtype=torch.uint8, device="cuda", generator=gen)
        codes |= torch.randint(0, 2, codes.shape, dtype=torch.uint8, device="cuda", generator=gen) << 7
        half = torch.empty(codes.shape, dtype=torch.half, device="cuda")
        for p0 in range(0, P, max(1, (1 << 26) // (HKV * page * D))):  # the table lookup in slices: its int64 index is 8 bytes per element
            sl = slice(p0, p0 + max(1, (1 << 26) // (HKV * page * D)))
            half[sl] = (lut[codes[sl].long()] * scales.view(1, HKV, 1, 1)).half()
        out8.append(codes.view(F8)), out16.append(half)
    return out8[0], out8[1], out16[0], out16[1]


def decode_table(quick):
    print("paged decode attention, FP8 cache against fp16 cache, Hkv = %d: us per call (launch-inclusive); GB/s = 2 len B Hkv D (1 | 2) bytes / "
          "time (K and V once per KV head); ratio = fp16 us / fp8 us (byte ratio 2)" % HKV)
    print("%-18s %-4s %-2s %-14s %-14s %9s %9s %9s %9s %7s" % ("(B, len, D)", "page", "G", "fp8 plan", "fp16 plan", "fp8 us", "GB/s", "fp16 us", "GB/s", "ratio"))
    gen = torch.Generator(device="cuda").manual_seed(0)
    lut = code_values()
    scales = torch.tensor([0.5 * (1.0 + 0.25 * h) for h in range(HKV)], device="cuda")
    lens = (4096,) if quick else LENS
    for D in DS:
        for N in lens:
            for B in BS:
                sl = torch.full((B,), N, dtype=torch.int32, device="cuda")
                for page in PAGES:
                    mp = N // page
                    per8 = 2 * B * HKV * N * D
                    nsets = max(1, min(MAX_SETS, -(-ROTATE_BYTES // per8)))
                    sets = []
                    for _ in range(nsets):
                        bt = torch.randperm(B * mp, generator=gen, device="cuda").view(mp, B).t().contiguous().to(torch.int32)
                        sets.append(pool_pair(B * mp, page, D, scales, lut, gen) + (bt,))
                    for G in GS:
                        Hq = HKV * G
                        q = torch.randn(B, Hq, D, dtype=torch.half, device="cuda", generator=gen)
                        o8, o16 = torch.empty_like(q), torch.empty_like(q)
                        p8, p16 = pkg.fa2_decode_paged_fp8_plan(B, Hq, HKV, mp, page, D), pkg.fa2_decode_paged_plan(B, Hq, HKV, mp, page, D)
                        ws8 = torch.empty(max(p8[2], 16), dtype=torch.uint8, device="cuda")
                        ws16 = torch.empty(max(p16[2], 16), dtype=torch.uint8, device="cuda")
                        i, j = [0], [0]

                        def fp8():
                            k8, v8, _, _, bt = sets[i[0] % nsets]
                            i[0] += 1
                            pkg.fa2_decode_paged_fp8(q, k8, v8, bt, sl, scales, scales, o8, None, ws8)

                        def fp16():
                            _, _, k16, v16, bt = sets[j[0] % nsets]
                            j[0] += 1
                            pkg.fa2_decode_paged(q, k16, v16, bt, sl, o16, None, ws16)

                        best = best_of({"fp8": fp8, "fp16": fp16})
                        print("%-18s %-4d %-2d %-14s %-14s %9.2f %9.1f %9.2f %9.1f %7.3f" % (
                            str((B, N, D)), page, G, "S=%d C=%d" % p8[:2], "S=%d C=%d" % p16[:2], best["fp8"] * 1e3, per8 / best["fp8"] * 1e-6,
                            best["fp16"] * 1e3, 2 * per8 / best["fp16"] * 1e-6, best["fp16"] / best["fp8"]), flush=True)
                    del sets
                    torch.cuda.empty_cache()


def append_table():
    print("paged KV append with fused RoPE (half), Hq / Hkv = 32 / 8, D = 128, page 16, T = 1, len 4096: us per call; ratio = fp16 us / fp8 us")
    gen = torch.Generator(device="cuda").manual_seed(1)
    Hq, D, page, T, N = 32, 128, 16, 1, 4096
    mp = N // page
    rope = pkg.kv_append_rope_table(N, D, device="cuda")
    scales = torch.tensor([0.01 * (1.0 + 0.25 * h) for h in range(HKV)], device="cuda")
    for B in (8, 64, 256):
        kn, vn = (torch.randn(B, T, HKV, D, dtype=torch.half, device="cuda", generator=gen) for _ in range(2))
        q = torch.randn(B, T, Hq, D, dtype=torch.half, device="cuda", generator=gen)
        qo = torch.empty_like(q)
        bt = torch.randperm(B * mp, generator=gen, device="cuda").view(mp, B).t().contiguous().to(torch.int32)
        sl = torch.full((B,), N, dtype=torch.int32, device="cuda")
        k16, v16 = (torch.zeros(B * mp, HKV, page, D, dtype=torch.half, device="cuda") for _ in range(2))
        k8, v8 = (torch.zeros(B * mp, HKV, page, D, dtype=torch.uint8, device="cuda").view(F8) for _ in range(2))
        best = best_of({"fp8": lambda: pkg.kv_append_paged_fp8(kn, vn, k8, v8, bt, sl, scales, scales, q, qo, rope, "half"),
                        "fp16": lambda: pkg.kv_append_paged(kn, vn, k16, v16, bt, sl, q, qo, rope, "half")})
        print("B=%-4d fp8 %8.2f us   fp16 %8.2f us   ratio %.3f" % (B, best["fp8"] * 1e3, best["fp16"] * 1e3, best["fp16"] / best["fp8"]), flush=True)


if __name__ == "__main__":
    decode_table("--quick" in sys.argv)
    append_table()
