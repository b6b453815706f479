"""GPU timing of the sparse multi-head latent attention decode over the paged latent cache held in FP8
(cuda_learn_notes_amd.fa2_decode_paged_mla_sparse_bf16_fp8) beside its bf16 sibling, in the method of
fa_paged_mla_sparse_bench.py: launch-inclusive times from one pair of device events around back-to-back calls after a warm-up, every timed
window >= 0.1 s, best of ROUNDS alternating rounds, the pools rotating over sets that together exceed the 256 MiB Infinity Cache. Everything is
measured TWICE (run 1, run 2, on the same pools) and both are printed.
  (B, T, Hq) x context at page 64, topk 2048, every sequence of length `context`, scale 192^-1/2, the lists of fa_paged_mla_sparse_bench.py.
  Two entries in the one run, alternating, on pools of the same logical content and the same queries, tables and lists:
    fp8    fa2_decode_paged_mla_sparse_bf16_fp8 on the pool of e4m3 codes at kv_scale 2^-8 (576 bytes a token)
    bf16   fa2_decode_paged_mla_sparse_bf16 on those codes dequantised to bf16, exactly (1152 bytes a token)
  fp8/bf16 is a reported measurement, no pass criterion. rd = the latent bytes the row addresses, B T 2048 x 576 resp. x 1152, over its time,
  TB/s, beside hipMemcpyDtoD (read + written bytes over time) from the same run.
  python fa_paged_mla_sparse_fp8_bench.py [--quick]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fa_paged_d256_bench import COPY_BYTES, copy_rate, spread, two_runs  # noqa: E402
from fa_paged_anyg_bench import BF, pkg  # noqa: E402
from fa_decode_paged_bench import rotating  # noqa: E402
from fa_prefill_paged_varlen_bench import cycle  # noqa: E402
from fa_paged_mla_sparse_bench import CONTEXTS, DC, DK, PAGE, QUICK, SCALE, SHAPES, TOPK, sample_lists  # noqa: E402

F8 = torch.float8_e4m3fn
KV_SCALE = 2.0 ** -8


def latent_sets(B, N, gen):
    """Rotating sets of (codes e4m3 [B N / page, page, 576], the same rows in bf16, block_table): randn rows at the scale of the tests
    quantised at KV_SCALE, pages placed by a random permutation. The sets are counted by the bytes of the codes, the smaller pool."""
    mp = N // PAGE

    def make():
        rows = torch.empty(B * mp, PAGE, DK, dtype=BF, device="cuda").normal_(0.0, SCALE, generator=gen)
        codes = (rows.float() * (1.0 / KV_SCALE)).to(F8)
        rows.copy_(codes.float() * KV_SCALE)  # exact: a power-of-two scale
        return codes, rows, torch.randperm(B * mp, generator=gen, device="cuda").view(B, mp).to(torch.int32)
    return rotating(make, B * N * DK)


def row(B, T, Hq, ctx, gen):
    sets = latent_sets(B, ctx, gen)
    q = (torch.randn(B, T, Hq, DK, device="cuda", generator=gen) * SCALE).to(BF)
    idx = sample_lists(B, T, ctx, gen)
    sl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    kvs = torch.tensor([KV_SCALE], dtype=torch.float32, device="cuda")
    o = [torch.empty(B, T, Hq, DC, dtype=BF, device="cuda") for _ in range(2)]
    plan = pkg.fa2_decode_paged_mla_sparse_bf16_fp8_plan(B, T, Hq, TOPK, ctx // PAGE, PAGE)
    assert plan == pkg.fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, TOPK, ctx // PAGE, PAGE)
    ws = [torch.empty(max(plan[2], 16), dtype=torch.uint8, device="cuda") for _ in range(2)]

    def fp8(nxt=cycle(sets)):
        codes, _, bt = nxt()
        pkg.fa2_decode_paged_mla_sparse_bf16_fp8(q, codes, bt, sl, kvs, idx, SCALE, o[0], None, ws[0])

    def bf16(nxt=cycle(sets)):
        _, rows, bt = nxt()
        pkg.fa2_decode_paged_mla_sparse_bf16(q, rows, bt, sl, idx, SCALE, o[1], None, ws[1])

    runs = two_runs({"fp8": fp8, "bf16": bf16})
    assert all(bool(torch.isfinite(x.float()).all()) for x in o)
    if len(sets) == 1:
        assert torch.equal(o[0].view(torch.int16), o[1].view(torch.int16))  # a power-of-two scale: the sibling's bits
    return runs, len(sets), plan


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    copy = [copy_rate() for _ in range(2)]
    print("sparse MLA decode over a paged latent cache, topk %d, page %d: us per call (launch-inclusive), two runs of every number. fp8 = "
          "fa2_decode_paged_mla_sparse_bf16_fp8 on e4m3 codes at kv_scale 2^-8 (576 bytes a token); bf16 = fa2_decode_paged_mla_sparse_bf16 on "
          "the same rows in bf16 (1152 bytes a token), the same lists. fp8/bf16 = the ratio of the times; rd = B T 2048 x the row's bytes over "
          "the time, TB/s" % (TOPK, PAGE))
    if copy[0]:
        print("hipMemcpyDtoD of %d MiB, read + written bytes over time: %.2f and %.2f TB/s (spread %.1f%%)" % (COPY_BYTES >> 20, copy[0], copy[1],
                                                                                                           100 * spread(*copy)))
    else:
        print("hipMemcpyDtoD: the vendor yardstick unit is not built, no copy rate")
    print("%-16s %7s %4s %-7s %9s %9s %9s %9s %10s %10s %8s %8s %8s %8s" % (
        "(B, T, Hq)", "context", "sets", "S x C", "fp8 1", "fp8 2", "bf16 1", "bf16 2", "fp8/bf16 1", "fp8/bf16 2", "rd fp8 1", "rd fp8 2", "rd bf 1",
        "rd bf 2"))
    todo = QUICK if a.quick else [(s, c) for s in SHAPES for c in CONTEXTS]
    for (B, T, Hq), ctx in todo:
        runs, nsets, plan = row(B, T, Hq, ctx, gen)
        us = {k: [r[k] * 1e3 for r in runs] for k in ("fp8", "bf16")}
        rd = {k: [B * T * TOPK * DK * w / (u * 1e-6) * 1e-12 for u in us[k]] for k, w in (("fp8", 1), ("bf16", 2))}
        print("%-16s %7d %4d %-7s %9.1f %9.1f %9.1f %9.1f %10.3f %10.3f %8.2f %8.2f %8.2f %8.2f" % (
            str((B, T, Hq)), ctx, nsets, "%dx%d" % plan[:2], *us["fp8"], *us["bf16"], us["fp8"][0] / us["bf16"][0], us["fp8"][1] / us["bf16"][1],
            *rd["fp8"], *rd["bf16"]), flush=True)
        torch.cuda.empty_cache()
