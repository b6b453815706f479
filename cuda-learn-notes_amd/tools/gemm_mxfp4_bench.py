"""GPU timing of the MXFP4-weight GEMMs (cuda_learn_notes_amd.gemm_mxfp4_bf16, gemm_mxfp4_grouped_bf16) beside the block-scaled
FP8 entries and what a caller does without either, in the method of tools/gemm_fp8_block128_grouped_bench.py: launch-inclusive times from one
pair of device events around back-to-back calls after a warm-up, every timed window >= 0.1 s, best of the alternating rounds, everything
measured TWICE (run 1, run 2, on the same buffers) and both printed. Grouped rows: the experts' weights are ONE pool; the rotating sets are
offset arrays that hand the same group sizes to other experts. Dense rows: rotating weight sets that together exceed the Infinity Cache.
  us per call:
    skinny   gemm_mxfp4[_grouped]_bf16(form="skinny")      tile   (form="tile");   "*" marks the form that form=None runs
    fp8      gemm_fp8_block128[_grouped]_bf16 (form=None) at the same shape on e4m3 weights, where K % 128 == 0 ("-" elsewhere)
    dq+mm    per non-empty expert torch dequantise of its MXFP4 weight to bf16 (nibble table, times the expanded scales) + torch.matmul
    wt TB/s  the touched experts' N K / 2 weight bytes over the better time of the * form (M_total <= 4 E, or dense M <= 64)
    PF       2 M N K over that time, at M >= 2048
  Before timing, both pinned forms are run once and their outputs compared bit for bit.
  python gemm_mxfp4_bench.py [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_d256_bench import spread  # noqa: E402
from fa_paged_anyg_bench import BF, pkg  # noqa: E402
from fa_decode_paged_bench import MAX_SETS, best_of, rotating  # noqa: E402
from fa_prefill_paged_varlen_bench import cycle  # noqa: E402
from gemm_fp8_block128_bench import F8, codes  # noqa: E402
from gemm_fp8_block128_grouped_bench import balanced, zipf  # noqa: E402

E8 = torch.float8_e8m0fnu
# (E, N, K): the gpt-oss-120b experts (gate/up and down at hidden 2880), DeepSeek-V3's expert projections at 32 and 256 experts
GROUPED = ((128, 5760, 2880), (128, 2880, 2880), (32, 4096, 7168), (32, 7168, 2048), (256, 4096, 7168), (256, 7168, 2048))
MS = (64, 512, 2048, 32768)
DENSE_NK, DENSE_MS = ((5760, 2880), (2880, 2880), (4096, 7168), (7168, 2048)), (1, 16, 64, 512, 4096)
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)


def mx_weight(shape, K, gen):
    """(packed e2m1 bytes [..., K/2], e8m0 scale bytes [..., K/32] around 2^-6): every byte value is a pair of valid codes."""
    b = torch.randint(0, 256, (*shape, K // 2), dtype=torch.uint8, device="cuda", generator=gen)
    return b, torch.randint(119, 124, (*shape, K // 32), dtype=torch.uint8, device="cuda", generator=gen)


def mx_rows(M, K, gen):
    """(e4m3fn codes [M,K], e8m0 scale bytes [M,K/32] around 2^-4, their bf16 values)."""
    a = codes(M, K, gen)
    sa = torch.randint(121, 126, (M, K // 32), dtype=torch.uint8, device="cuda", generator=gen)
    x = (a.to(BF).view(M, K // 32, 32) * torch.pow(2.0, sa.float() - 127).to(BF)[:, :, None]).view(M, K)
    return a, sa.view(E8), x


def dequant(b, sb, lut):
    """bf16 [N,K] of one packed weight [N,K/2] with its scale bytes [N,K/32]."""
    N, K = b.shape[0], 2 * b.shape[1]
    v = torch.stack((lut[(b & 15).long()], lut[(b >> 4).long()]), dim=-1).view(N, K // 32, 32)
    return (v * torch.pow(2.0, sb.float() - 127).to(BF)[:, :, None]).view(N, K)


def report(head, runs, calls, auto, wt_bytes, flops, skinny_rule):
    t = min(r[auto] for r in runs) * 1e-3
    cell = lambda n: ("%9.1f %9.1f%s" % (runs[0][n] * 1e3, runs[1][n] * 1e3, "*" if n == auto else " ")) if n in calls else "%9s %9s " % ("-", "-")  # noqa: E731
    print("%s %s %s %s %s %6s %6s %5.1f%%" % (head, cell("skinny"), cell("tile"), cell("fp8"), cell("dq+mm"),
                                             "%6.2f" % (wt_bytes / t * 1e-12) if skinny_rule else "", "%6.2f" % (flops / t * 1e-15) if flops else "",
                                             100 * spread(runs[0][auto], runs[1][auto])), flush=True)


def same_bits(run, out):
    got = []
    for form in ("skinny", "tile"):
        out.zero_()
        run(form)
        got.append(out.clone())
    assert torch.equal(got[0].view(torch.int16), got[1].view(torch.int16)) and bool(torch.isfinite(got[0].float()).all())


def grouped_rows(E, N, K, Ms, gen, cpu_gen, lut):
    b, sb = mx_weight((E, N), K, gen)
    fp8 = K % 128 == 0
    if fp8:
        b8 = torch.empty(E, N, K, dtype=torch.uint8, device="cuda").view(F8)
        for e in range(E):
            b8[e] = codes(N, K, gen)
        sb8 = torch.rand(E, -(-N // 128), K // 128, device="cuda", generator=gen) * 1e-3 + 1e-4
    for M in Ms:
        a, sa, x = mx_rows(M, K, gen)
        sa8 = torch.rand(M, K // 128, device="cuda", generator=gen) * 1e-2 + 1e-3 if fp8 else None
        out = torch.empty(M, N, dtype=BF, device="cuda")
        for dist in ("balanced", "zipf"):
            sizes = balanced(M, E) if dist == "balanced" else zipf(M, E, cpu_gen)
            touched = sum(1 for s in sizes if s)
            sets, nsets = [], 1 if touched == E else min(MAX_SETS, E)
            for i in range(nsets):
                shift = i * E // nsets
                rolled = sizes[E - shift:] + sizes[:E - shift]
                off = torch.tensor([0] + rolled).cumsum(0).tolist()
                sets.append((torch.tensor(off, dtype=torch.int32, device="cuda"), [(e, off[e], off[e + 1]) for e in range(E) if rolled[e]]))

            def mx(form, nxt):
                pkg.gemm_mxfp4_grouped_bf16(a, sa, b, sb, nxt()[0], out, form=form)

            def dqmm(nxt=cycle(sets)):
                for e, r0, r1 in nxt()[1]:
                    torch.matmul(x[r0:r1], dequant(b[e], sb[e], lut).t(), out=out[r0:r1])
            same_bits(lambda form: mx(form, lambda: sets[0]), out)
            calls = {"skinny": lambda nxt=cycle(sets): mx("skinny", nxt), "tile": lambda nxt=cycle(sets): mx("tile", nxt), "dq+mm": dqmm}
            if fp8:
                calls["fp8"] = lambda nxt=cycle(sets): pkg.gemm_fp8_block128_grouped_bf16(a, sa8, b8, sb8, nxt()[0], out)
            runs = [best_of(calls, rounds=2) for _ in range(2)]
            auto = "skinny" if "form skinny" in pkg.manifest.describe_gemm_mxfp4_grouped_bf16(M, E, N, K) else "tile"
            report("%6d %4d %5d %5d %-8s %4d %4d" % (M, E, N, K, dist, touched, len(sets)), runs, calls, auto, touched * N * K / 2,
                   2.0 * M * N * K if M >= 2048 else 0, auto == "skinny")
    del b, sb
    torch.cuda.empty_cache()


def dense_rows(N, K, Ms, gen, lut):
    fp8 = K % 128 == 0
    sb8 = torch.rand(-(-N // 128), K // 128, device="cuda", generator=gen) * 1e-3 + 1e-4 if fp8 else None
    sets = rotating(lambda: mx_weight((N,), K, gen) + ((codes(N, K, gen),) if fp8 else ()), N * K // 2)
    for M in Ms:
        a, sa, x = mx_rows(M, K, gen)
        sa8 = torch.rand(M, K // 128, device="cuda", generator=gen) * 1e-2 + 1e-3 if fp8 else None
        out = torch.empty(M, N, dtype=BF, device="cuda")

        def mx(form, nxt):
            w = nxt()
            pkg.gemm_mxfp4_bf16(a, sa, w[0], w[1], out, form=form)

        def dqmm(nxt=cycle(sets)):
            w = nxt()
            torch.matmul(x, dequant(w[0], w[1], lut).t(), out=out)
        same_bits(lambda form: mx(form, lambda: sets[0]), out)
        calls = {"skinny": lambda nxt=cycle(sets): mx("skinny", nxt), "tile": lambda nxt=cycle(sets): mx("tile", nxt), "dq+mm": dqmm}
        if M > 512:
            del calls["skinny"]  # the pinned skinny form re-reads its strip per 64 rows: not a form for these rows
        if fp8:
            calls["fp8"] = lambda nxt=cycle(sets): pkg.gemm_fp8_block128_bf16(a, sa8, nxt()[2], sb8, out)
        runs = [best_of(calls, rounds=2) for _ in range(2)]
        auto = "skinny" if M <= 64 else "tile"
        report("%6d %4s %5d %5d %-8s %4s %4d" % (M, "-", N, K, "dense", "-", len(sets)), runs, calls, auto, N * K / 2, 2.0 * M * N * K if M >= 2048 else 0,
               auto == "skinny")
    del sets
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    gen, cpu_gen = torch.Generator(device="cuda").manual_seed(0), torch.Generator().manual_seed(0)
    lut = torch.tensor(E2M1, dtype=BF, device="cuda")
    print("gemm_mxfp4[_grouped]_bf16, both pinned forms (* = the form that form=None runs), beside gemm_fp8_block128[_grouped]_bf16 (form=None; where "
          "K % 128 == 0) and torch dequantise + matmul per expert: us per call (launch-inclusive), two runs of every number, the calls alternating "
          "in every round; tchd = non-empty experts; sets = rotating offset arrays (grouped) or weight sets (dense); wt TB/s = touched N K / 2 "
          "bytes, PF = 2 M N K, both over the better time of the * form; spread = between its two runs")
    print("%6s %4s %5s %5s %-8s %4s %4s %9s %9s  %9s %9s  %9s %9s  %9s %9s  %6s %6s %6s" % (
        "M", "E", "N", "K", "rows", "tchd", "sets", "skinny 1", "skinny 2", "tile 1", "tile 2", "fp8 1", "fp8 2", "dq+mm 1", "dq+mm 2", "wtTB/s", "PF",
        "spread"))
    for N, K in (DENSE_NK[:1] + DENSE_NK[2:3] if args.quick else DENSE_NK):
        dense_rows(N, K, (1, 64, 4096) if args.quick else DENSE_MS, gen, lut)
    for E, N, K in (GROUPED[:1] + GROUPED[2:3] if args.quick else GROUPED):
        grouped_rows(E, N, K, (64, 2048) if args.quick else MS, gen, cpu_gen, lut)
