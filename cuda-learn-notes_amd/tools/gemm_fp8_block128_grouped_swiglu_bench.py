"""GPU timing of the fused gate/up + SiLU-mul + quantise grouped FP8 GEMM (cuda_learn_notes_amd.gemm_fp8_block128_grouped_swiglu_fp8; DESIGN
4.4.30) beside the chain it replaces, in the method of tools/gemm_fp8_block128_grouped_bench.py: launch-inclusive times from one pair of device
events around back-to-back calls after a warm-up, every timed window >= 0.1 s, best of the alternating rounds, everything measured TWICE (run
1, run 2, on the same buffers) and both printed. The experts' weights are ONE pool [E, 2 I, K]; the rotating sets are offset arrays that hand
the same (balanced) group sizes to other experts, so that consecutive calls touch other weights wherever a call touches less than the pool.
  (M_total, E, I, K), us per call:
    skinny   gemm_fp8_block128_grouped_swiglu_fp8(form="skinny")      tile   (form="tile");   "*" marks the form that form=None runs
    chain    gemm_fp8_block128_grouped_bf16 (form=None) into gate_up bf16 [M_total, 2 I], torch silu(gate) * up, quant_fp8_block128_bf16
    x        chain time / the * form's time (above 1: the fusion is ahead), from the better run of each
    wt TB/s  the touched experts' 2 I K weight bytes over the better time of the skinny form
  Before timing, the fused forms are run once and compared bit for bit with each other, and their dequantised h with the chain's.
  python gemm_fp8_block128_grouped_swiglu_bench.py [--quick]"""
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
from gemm_fp8_block128_grouped_bench import balanced  # noqa: E402

SHAPES = ((256, 2048, 7168), (32, 1024, 2048))  # (E, I, K): DeepSeek-V3's routed experts; a smaller layer
MS = (64, 256, 1024, 4096, 32768)             # decode (a mean group of 1/4 ... 4 rows at E = 256) and prefill


def rows_of(E, I, K, Ms, gen):
    kb = K // 128
    b = torch.empty(E, 2 * I, K, dtype=torch.uint8, device="cuda").view(F8)
    for e in range(E):
        b[e] = codes(2 * I, K, gen)
    sb = torch.rand(E, 2 * I // 128, kb, device="cuda", generator=gen) * 1e-3 + 1e-4
    for M in Ms:
        a = codes(M, K, gen)
        sa = torch.rand(M, kb, device="cuda", generator=gen) * 1e-2 + 1e-3
        gate_up = torch.empty(M, 2 * I, dtype=BF, device="cuda")
        hb = torch.empty(M, I, dtype=BF, device="cuda")
        h, hs = torch.empty(M, I, dtype=torch.uint8, device="cuda").view(F8), torch.empty(M, I // 128, device="cuda")
        sizes = balanced(M, E)
        touched = sum(1 for s in sizes if s)
        sets, nsets = [], 1 if touched == E else min(MAX_SETS, E)
        for i in range(nsets):
            shift = i * E // nsets
            sets.append(torch.tensor([0] + sizes[E - shift:] + sizes[:E - shift], device="cuda").cumsum(0).to(torch.int32))

        def fused(form, nxt):
            pkg.gemm_fp8_block128_grouped_swiglu_fp8(a, sa, b, sb, nxt(), h, hs, form=form)

        def chain(nxt=cycle(sets)):
            pkg.gemm_fp8_block128_grouped_bf16(a, sa, b, sb, nxt(), gate_up)
            torch.mul(torch.nn.functional.silu(gate_up[:, :I]), gate_up[:, I:], out=hb)
            pkg.quant_fp8_block128_bf16(hb, h, hs)
        got = []
        for call in (lambda: fused("skinny", lambda: sets[0]), lambda: fused("tile", lambda: sets[0]), lambda: chain(lambda: sets[0])):
            h.view(torch.uint8).zero_()
            hs.zero_()
            call()
            got.append((h.view(torch.uint8).clone(), hs.clone()))
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
        deq = [c.view(F8).float() * s.repeat_interleave(128, dim=1) for c, s in (got[0], got[2])]
        assert bool(torch.isfinite(deq[0]).all())
        # two e4m3 roundings (2^-4 each of its own value) and the chain's bf16 roundings; a code near a scale's amax can move by a step more
        far = float(((deq[0] - deq[1]).abs() / (0.25 * deq[1].abs() + 2.0 ** -7 * got[2][1].repeat_interleave(128, dim=1))).max())
        assert far <= 1.0, far
        del got, deq
        calls = {"skinny": lambda nxt=cycle(sets): fused("skinny", nxt), "tile": lambda nxt=cycle(sets): fused("tile", nxt), "chain": chain}
        runs = [best_of(calls, rounds=2) for _ in range(2)]
        auto = "skinny" if "form skinny" in pkg.manifest.describe_gemm_fp8_block128_grouped_swiglu_fp8(M, E, I, K) else "tile"
        t = {n: min(r[n] for r in runs) * 1e-3 for n in calls}
        cell = lambda n: "%9.1f %9.1f%s" % (runs[0][n] * 1e3, runs[1][n] * 1e3, "*" if n == auto else " ")  # noqa: E731
        print("%6d %4d %5d %5d %4d %4d %s %s %s %6.2f %6.2f %6.2f %5.1f%%" % (
            M, E, I, K, touched, len(sets), cell("skinny"), cell("tile"), cell("chain"), t["chain"] / t["skinny"], t["chain"] / t["tile"],
            touched * 2 * I * K / t["skinny"] * 1e-12, 100 * spread(runs[0][auto], runs[1][auto])), flush=True)
    del b
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    print("gemm_fp8_block128_grouped_swiglu_fp8, both pinned forms (* = the form that form=None runs), beside the chain grouped GEMM -> torch "
          "silu * up -> quant_fp8_block128_bf16 on the same inputs: us per call (launch-inclusive), two runs of every number, the calls "
          "alternating in every round; rows balanced over the experts; tchd = non-empty experts; sets = offset arrays rotating the sizes over the "
          "experts; x = chain / form (better run of each; above 1 the fusion is ahead); wt TB/s = touched 2 I K bytes over the skinny form's "
          "better time; spread = between the * form's two runs")
    print("%6s %4s %5s %5s %4s %4s %9s %9s  %9s %9s  %9s %9s  %6s %6s %6s %6s" % (
        "M_tot", "E", "I", "K", "tchd", "sets", "skinny 1", "skinny 2", "tile 1", "tile 2", "chain 1", "chain 2", "x skny", "x tile", "wtTB/s",
        "spread"))
    for E, I, K in (SHAPES[1:] if args.quick else SHAPES):
        rows_of(E, I, K, (64, 4096) if args.quick else MS, gen)
