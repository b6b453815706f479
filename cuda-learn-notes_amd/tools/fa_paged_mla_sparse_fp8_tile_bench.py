"""GPU timing of the sparse multi-head latent attention decode over the paged latent cache in DeepSeek-V3.2's own FP8 row of 656 bytes
(cuda_learn_notes_amd.fa2_decode_paged_mla_sparse_bf16_fp8_tile) beside its two siblings, in the method of
fa_paged_mla_sparse_fp8_bench.py: launch-inclusive times from one pair of device events around back-to-back calls after a warm-up, every
timed window >= 0.1 s, best of ROUNDS alternating rounds, the pools rotating over sets that together exceed the 256 MiB Infinity Cache.
Everything is measured TWICE (run 1, run 2, on the same pools) and both are printed.
  (B, T, Hq) x context at page 64, topk 2048, every sequence of length `context`, scale 192^-1/2, the lists of fa_paged_mla_sparse_bench.py.
  Three entries in the one run, alternating, on the same queries, tables and lists:
    tile   fa2_decode_paged_mla_sparse_bf16_fp8_tile on rows of 656 bytes: codes with per-token tile scales amax / 448, k_pe in bf16
    fp8    fa2_decode_paged_mla_sparse_bf16_fp8 on a pool of e4m3 codes at kv_scale 2^-8 (576 bytes a token)
    bf16   fa2_decode_paged_mla_sparse_bf16 on the tile pool dequantised to bf16 (1152 bytes a token): the new entry's bits
  tile/fp8 and tile/bf16 are reported measurements, no pass criterion. rd = the bytes the row addresses, B T 2048 x 656 / 576 / 1152, over
  its time, TB/s, beside hipMemcpyDtoD (read + written bytes over time) from the same run. Then the append of 4096 tokens (Hq 128, rope
  "half") beside kv_append_paged_mla_bf16_fp8 on the same tokens.
  python fa_paged_mla_sparse_fp8_tile_bench.py [--quick]"""
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

F8, ROW, KV_SCALE = torch.float8_e4m3fn, 656, 2.0 ** -8
NAMES = ("tile", "fp8", "bf16")


def latent_sets(B, N, gen):
    """Rotating sets of (tile pool uint8 [B N / page, page, 656], codes e4m3 [.., 576] at KV_SCALE, the tile pool dequantised to bf16 [.., 576],
    block_table): randn rows at the scale of the tests, each 128-dim tile quantised at its own amax / 448, pages placed by a random
    permutation. The sets are counted by the bytes of the 576-byte pool, the smallest."""
    mp = N // PAGE

    def make():
        rows = torch.empty(B * mp, PAGE, DK, dtype=BF, device="cuda").normal_(0.0, SCALE, generator=gen)
        tile = torch.empty(B * mp, PAGE, ROW, dtype=torch.uint8, device="cuda")
        codes, scales, k_pe = pkg.latent_pool_fp8_tile_views(tile)
        t = rows[..., :DC].float().view(B * mp, PAGE, 4, 128)
        s = t.abs().amax(-1).clamp_min(1e-4) / 448.0
        codes.copy_((t * (1.0 / s)[..., None]).clamp(-448, 448).to(F8).view(B * mp, PAGE, DC))
        scales.copy_(s)
        k_pe.copy_(rows[..., DC:])
        flat = (rows.float() * (1.0 / KV_SCALE)).to(F8)
        rows[..., :DC] = (codes.float() * s.repeat_interleave(128, -1)).to(BF)
        return tile, flat, rows, torch.randperm(B * mp, generator=gen, device="cuda").view(B, mp).to(torch.int32)
    return rotating(make, B * N * DK)


def row(B, T, Hq, ctx, gen):
    sets = latent_sets(B, ctx, gen)
    q = (torch.randn(B, T, Hq, DK, device="cuda", generator=gen) * SCALE).to(BF)
    idx = sample_lists(B, T, ctx, gen)
    sl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
    kvs = torch.tensor([KV_SCALE], dtype=torch.float32, device="cuda")
    o = [torch.empty(B, T, Hq, DC, dtype=BF, device="cuda") for _ in range(3)]
    plan = pkg.fa2_decode_paged_mla_sparse_bf16_fp8_tile_plan(B, T, Hq, TOPK, ctx // PAGE, PAGE)
    assert plan == pkg.fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, TOPK, ctx // PAGE, PAGE)
    ws = [torch.empty(max(plan[2], 16), dtype=torch.uint8, device="cuda") for _ in range(3)]

    def tile(nxt=cycle(sets)):
        pool, _, _, bt = nxt()
        pkg.fa2_decode_paged_mla_sparse_bf16_fp8_tile(q, pool, bt, sl, idx, SCALE, o[0], None, ws[0])

    def fp8(nxt=cycle(sets)):
        _, codes, _, bt = nxt()
        pkg.fa2_decode_paged_mla_sparse_bf16_fp8(q, codes, bt, sl, kvs, idx, SCALE, o[1], None, ws[1])

    def bf16(nxt=cycle(sets)):
        _, _, rows, bt = nxt()
        pkg.fa2_decode_paged_mla_sparse_bf16(q, rows, bt, sl, idx, SCALE, o[2], None, ws[2])

    runs = two_runs({"tile": tile, "fp8": fp8, "bf16": bf16})
    assert all(bool(torch.isfinite(x.float()).all()) for x in o)
    if len(sets) == 1:
        assert torch.equal(o[0].view(torch.int16), o[2].view(torch.int16))  # the bf16 entry's bits on the dequantised pool
    return runs, len(sets), plan


def append_row(gen, tokens=4096, Hq=128):
    """[{name: ms}] x 2 of the two quantising appends on the same tokens: B = 1, the sequence's first `tokens` positions, q rotated along."""
    mp = tokens // PAGE
    c_new = torch.empty(tokens, DC, dtype=BF, device="cuda").normal_(0.0, SCALE, generator=gen)
    k_pe = torch.empty(tokens, DK - DC, dtype=BF, device="cuda").normal_(0.0, SCALE, generator=gen)
    q = torch.empty(tokens, Hq, DK, dtype=BF, device="cuda").normal_(0.0, SCALE, generator=gen)
    q_out = torch.empty_like(q)
    bt = torch.randperm(mp, generator=gen, device="cuda").view(1, mp).to(torch.int32)
    sl = torch.full((1,), tokens, dtype=torch.int32, device="cuda")
    cu = torch.tensor([0, tokens], dtype=torch.int32, device="cuda")
    table = pkg.kv_append_rope_table(tokens, 64).cuda()
    tile_pool = torch.zeros(mp, PAGE, ROW, dtype=torch.uint8, device="cuda")
    flat_pool = torch.zeros(mp, PAGE, DK, dtype=torch.uint8, device="cuda").view(F8)
    kvs = torch.tensor([KV_SCALE], dtype=torch.float32, device="cuda")
    return two_runs({"tile": lambda: pkg.kv_append_paged_mla_bf16_fp8_tile(c_new, k_pe, tile_pool, bt, sl, cu, q, q_out, table, "half", True),
                     "fp8": lambda: pkg.kv_append_paged_mla_bf16_fp8(c_new, k_pe, flat_pool, bt, sl, cu, kvs, q, q_out, table, "half")})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    copy = [copy_rate() for _ in range(2)]
    print("sparse MLA decode over a paged latent cache, topk %d, page %d: us per call (launch-inclusive), two runs of every number. tile = "
          "fa2_decode_paged_mla_sparse_bf16_fp8_tile on rows of 656 bytes (per-token tile scales); fp8 = fa2_decode_paged_mla_sparse_bf16_fp8 on "
          "e4m3 codes at kv_scale 2^-8 (576 bytes a token); bf16 = fa2_decode_paged_mla_sparse_bf16 on the tile pool dequantised (1152 bytes a "
          "token), the same lists. rd = B T 2048 x the row's bytes over the time, TB/s" % (TOPK, PAGE))
    if copy[0]:
        print("hipMemcpyDtoD of %d MiB, read + written bytes over time: %.2f and %.2f TB/s (spread %.1f%%)" % (COPY_BYTES >> 20, copy[0], copy[1],
                                                                                                           100 * spread(*copy)))
    else:
        print("hipMemcpyDtoD: the vendor yardstick unit is not built, no copy rate")
    print("%-16s %7s %4s %-7s" % ("(B, T, Hq)", "context", "sets", "S x C") + "".join(" %8s %8s" % (n + " 1", n + " 2") for n in NAMES)
          + " %10s %10s %11s %11s" % ("tile/fp8 1", "tile/fp8 2", "tile/bf16 1", "tile/bf16 2") + " %9s %9s %9s" % ("rd tile", "rd fp8", "rd bf16")
          + " %9s" % "fp8 sprd")
    todo = QUICK if a.quick else [(s, c) for s in SHAPES for c in CONTEXTS]
    for (B, T, Hq), ctx in todo:
        runs, nsets, plan = row(B, T, Hq, ctx, gen)
        us = {k: [r[k] * 1e3 for r in runs] for k in NAMES}
        rd = {k: B * T * TOPK * w / (min(us[k]) * 1e-6) * 1e-12 for k, w in (("tile", ROW), ("fp8", DK), ("bf16", 2 * DK))}
        print("%-16s %7d %4d %-7s" % (str((B, T, Hq)), ctx, nsets, "%dx%d" % plan[:2]) + "".join(" %8.1f %8.1f" % tuple(us[k]) for k in NAMES)
              + " %10.3f %10.3f %11.3f %11.3f" % (us["tile"][0] / us["fp8"][0], us["tile"][1] / us["fp8"][1], us["tile"][0] / us["bf16"][0],
                                                  us["tile"][1] / us["bf16"][1])
              + " %9.2f %9.2f %9.2f" % (rd["tile"], rd["fp8"], rd["bf16"]) + " %8.1f%%" % (100 * spread(*us["fp8"])), flush=True)
        torch.cuda.empty_cache()
    ap_runs = append_row(gen)
    print("append of 4096 tokens, Hq 128, rope half, us per call: tile (656-byte rows, scale_pow2) %.1f and %.1f; fp8 (576-byte rows, one "
          "kv_scale) %.1f and %.1f; tile/fp8 %.3f and %.3f" % (ap_runs[0]["tile"] * 1e3, ap_runs[1]["tile"] * 1e3, ap_runs[0]["fp8"] * 1e3,
                                                               ap_runs[1]["fp8"] * 1e3, ap_runs[0]["tile"] / ap_runs[0]["fp8"],
                                                               ap_runs[1]["tile"] / ap_runs[1]["fp8"]))
