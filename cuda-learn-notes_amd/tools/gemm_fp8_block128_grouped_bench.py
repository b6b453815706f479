"""GPU timing of the grouped (MoE) block-scaled FP8 GEMM (cuda_learn_notes_amd.gemm_fp8_block128_grouped_bf16) beside what a caller
has without it, in the method of tools/gemm_fp8_block128_bench.py: launch-inclusive times from one pair of device events around back-to-back
calls after a warm-up, every timed window >= 0.1 s, best of the alternating rounds, everything measured TWICE (run 1, run 2, on the same buffers)
and both printed. The experts' weights are ONE pool [E, N, K]; the rotating sets are offset arrays that hand the same group sizes to other
experts (the sizes rolled over the experts), so that consecutive calls touch other weights wherever a call touches less than the pool; where
every expert is touched, a call reads the whole pool, which is larger than the 256 MiB Infinity Cache at every shape here.
  (M_total, E) x (N, K) x the distribution of rows over experts (balanced, or Zipf-like: sizes ~ 1 / rank, the ranks shuffled), us per call:
    skinny   gemm_fp8_block128_grouped_bf16(form="skinny")            tile   (form="tile");   "*" marks the form that form=None runs
    loop     (a) a Python loop of gemm_fp8_block128_bf16 over the non-empty experts, on views made beforehand: what a caller had before
    dq+mm    (b) per non-empty expert torch dequantise of its weight to bf16 + torch.matmul
    wt TB/s  the touched experts' N K weight bytes over the time of the form that form=None runs
    PF       2 M_total N K over that time, at M_total >= 2048
  Before timing, the three fp8 paths are run once and their outputs compared bit for bit.
  python gemm_fp8_block128_grouped_bench.py [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_d256_bench import spread  # noqa: E402
from fa_paged_anyg_bench import BF, pkg  # noqa: E402
from fa_decode_paged_bench import MAX_SETS, best_of  # noqa: E402
from fa_prefill_paged_varlen_bench import cycle  # noqa: E402
from gemm_fp8_block128_bench import F8, codes  # noqa: E402

NK = ((4096, 7168), (7168, 2048))  # DeepSeek-V3's expert projections: gate / up, down
ES, MS = (32, 256), (64, 128, 512, 1024, 2048, 32768)  # 128 and 1024: a mean group of 4 rows at either E, where the dispatch rule turns


def balanced(M, E):
    """M rows over E experts as evenly as they go; with M < E the non-empty experts are spread over the pool."""
    if M >= E:
        return [M // E + (1 if e < M % E else 0) for e in range(E)]
    sizes = [0] * E
    for i in range(M):
        sizes[i * E // M] = 1
    return sizes


def zipf(M, E, gen):
    """Sizes ~ 1 / rank by largest remainders, the ranks shuffled over the experts."""
    w = 1.0 / torch.arange(1, E + 1, dtype=torch.float64)
    share = w / w.sum() * M
    sizes = share.floor().long()
    rest = M - int(sizes.sum())
    sizes[torch.argsort(share - sizes, descending=True)[:rest]] += 1
    return sizes[torch.randperm(E, generator=gen)].tolist()


def rows_of(N, K, E, Ms, gen, cpu_gen):
    kb, nb = K // 128, -(-N // 128)
    b = torch.empty(E, N, K, dtype=torch.uint8, device="cuda").view(F8)
    for e in range(E):
        b[e] = codes(N, K, gen)
    sb =torch.rand(E, nb, kb, device="cuda", generator=gen) * 1e-3 + 1e-4
    sbn = sb.repeat_interleave(128, dim=1)[:, :N].to(BF)[:, :, :, None]  # the block scales expanded over N, once
    for M in Ms:
        a = codes(M, K, gen)
        sa = torch.rand(M, kb, device="cuda", generator=gen) * 1e-2 + 1e-3
        x = (a.to(BF).view(M, kb, 128) * sa.to(BF)[:, :, None]).view(M, K)
        out = torch.empty(M, N, dtype=BF, device="cuda")
        for dist in ("balanced", "zipf"):
            sizes = balanced(M, E) if dist == "balanced" else zipf(M, E, cpu_gen)
            touched = sum(1 for s in sizes if s)
            sets, nsets = [], 1 if touched == E else min(MAX_SETS, E)
            for i in range(nsets):
                shift = i * E // nsets
                rolled = sizes[E - shift:] + sizes[:E - shift]
                off = torch.tensor([0] + rolled).cumsum(0).tolist()
                views = [(e, a[off[e]:off[e + 1]], sa[off[e]:off[e + 1]], x[off[e]:off[e + 1]], out[off[e]:off[e + 1]]) for e in range(E) if rolled[e]]
                sets.append((torch.tensor(off, dtype=torch.int32, device="cuda"), views))

            def grouped(form, nxt):
                pkg.gemm_fp8_block128_grouped_bf16(a, sa, b, sb, nxt()[0], out, form=form)

            def loop(nxt=cycle(sets)):
                for e, ae, sae, _, oe in nxt()[1]:
                    pkg.gemm_fp8_block128_bf16(ae, sae, b[e], sb[e], oe)

            def dqmm(nxt=cycle(sets)):
                for e, _, _, xe, oe in nxt()[1]:
                    torch.matmul(xe, (b[e].to(BF).view(N, kb, 128) * sbn[e]).view(N, K).t(), out=oe)
            same = []
            for call in (lambda: grouped("skinny", lambda: sets[0]), lambda: grouped("tile", lambda: sets[0]), lambda: loop(lambda: sets[0])):
                out.zero_()
                call()
                same.append(out.clone())
            assert torch.equal(same[0].view(torch.int16), same[1].view(torch.int16)) and torch.equal(same[0].view(torch.int16), same[2].view(torch.int16))
            assert bool(torch.isfinite(same[0].float()).all())
            del same
            calls = {"skinny": lambda nxt=cycle(sets): grouped("skinny", nxt), "tile": lambda nxt=cycle(sets): grouped("tile", nxt), "loop": loop,
                     "dq+mm": dqmm}
            runs = [best_of(calls, rounds=2) for _ in range(2)]
            auto = "skinny" if "form skinny" in pkg.manifest.describe_gemm_fp8_block128_grouped_bf16(M, E, N, K) else "tile"
            t = min(r[auto] for r in runs) * 1e-3
            cell = lambda n: "%9.1f %9.1f%s" % (runs[0][n] * 1e3, runs[1][n] * 1e3, "*" if n == auto else " ")  # noqa: E731
            print("%6d %4d %5d %5d %-8s %4d %4d %s %s %s %s %6.2f %6s %5.1f%%" % (
                M, E, N, K, dist, touched, len(sets), cell("skinny"), cell("tile"), cell("loop"), cell("dq+mm"), touched * N * K / t * 1e-12,
                "%6.2f" % (2.0 * M * N * K / t * 1e-15) if M >= 2048 else "", 100 * spread(runs[0][auto], runs[1][auto])), flush=True)
    del b, sbn
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    gen, cpu_gen = torch.Generator(device="cuda").manual_seed(0), torch.Generator().manual_seed(0)
    print("gemm_fp8_block128_grouped_bf16, both pinned forms (* = the form that form=None runs), beside (a) a loop of gemm_fp8_block128_bf16 over "
          "the non-empty experts and (b) torch dequantise + matmul per expert: us per call (launch-inclusive), two runs of every number, the calls "
          "alternating in every round; touched = non-empty experts; sets = offset arrays rotating the sizes over the experts; wt TB/s = touched "
          "N K bytes, PF = 2 M_total N K, both over the better time of the * form; spread = between its two runs")
    print("%6s %4s %5s %5s %-8s %4s %4s %9s %9s  %9s %9s  %9s %9s  %9s %9s  %6s %6s %6s" % (
        "M_tot", "E", "N", "K", "rows", "tchd", "sets", "skinny 1", "skinny 2", "tile 1", "tile 2", "loop 1", "loop 2", "dq+mm 1", "dq+mm 2", "wtTB/s",
        "PF", "spread"))
    for N, K in (NK[1:] if args.quick else NK):
        for E in (ES[:1] if args.quick else ES):
            rows_of(N, K, E, (64, 2048) if args.quick else MS, gen, cpu_gen)
