"""GPU timing of the bf16 paged entries over FP8 (e4m3) pools (cuda_learn_notes_amd.kv_append_paged_varlen_bf16_fp8,
fa2_prefill_paged_varlen_window_sink_bf16_fp8, fa2_decode_paged_multi_window_sink_bf16_fp8) against their bf16 siblings (kv_append_paged_varlen_bf16,
fa2_prefill_paged_varlen_window_sink_bf16, fa2_decode_paged_multi_window_sink_bf16) in the same process on pools of the same logical content (the
FP8 pools are the bf16 pools quantised under per-head scales), in the method of fa_paged_sink_bench.py: launch-inclusive times from one pair of
device events around back-to-back calls after a warm-up, every timed window >= 0.1 s, best of ROUNDS alternating rounds, the pools rotating
over shuffled sets (as many as make the bf16 sets exceed the 256 MiB Infinity Cache together; the FP8 sets are half that). x = bf16 sibling
time / FP8 entry time: above 1 the FP8 entry is faster. The yardstick for a row is the sibling's own spread between two runs of this tool.
  multi     (B, T, context) with Hq 32, Hkv 8, D 128 (G = 4) and the gpt-oss heads Hq 64, Hkv 8, D 64 (G = 8), W in {1024, None}, the
            workspaces preallocated: T G from 4 to 64, contexts 4096 and 16384;
  prefill   three uniform headline shapes and a ragged batch of fa_prefill_paged_varlen_bench.py behind a context of 4096, W in {1024, None},
            and the gpt-oss 4 x 512 prefill at W = 128;
  append    a decode step's append (64 x 1 token) and a prefill's (4 x 512) with the half-split rotation.
W = None is a window past the cache.
  python fa_paged_bf16_fp8_bench.py [--skip prefill multi append]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from fa_decode_paged_bench import paged_from, rotating  # noqa: E402
from fa_paged_bf16_bench import batch_name, offsets  # noqa: E402
from fa_prefill_paged_bench import best_of  # noqa: E402
from fa_prefill_paged_varlen_bench import RAGGED, UNIFORM, cycle  # noqa: E402

BF, F8 = torch.bfloat16, torch.float8_e4m3fn
PAGE = 16
HEADLINE = (32, 8, 128)  # Hq, Hkv, D
GPT_OSS = (64, 8, 64)
WINDOWS = (1024, None)
CTX = 4096
MULTI = [(HEADLINE, 64, 1, 4096), (HEADLINE, 8, 1, 16384), (HEADLINE, 1, 1, 16384), (HEADLINE, 8, 4, 16384), (GPT_OSS, 64, 1, 4096),
         (GPT_OSS, 8, 2, 16384), (GPT_OSS, 8, 8, 16384)]


def scales(Hkv):
    base = [1.0, 2.5, 0.5, 1.75, 0.75, 3.0, 1.25, 0.375]
    ks = torch.tensor([2.0 ** -3 * base[h % 8] for h in range(Hkv)], device="cuda")
    return ks, ks * 2.0


def codes(shape, gen):
    """Random e4m3 bytes of magnitude below 4 (0x48), both signs, as halves (paged_from moves halves; 0 .. 255 are exact there)."""
    c = torch.randint(0, 0x48, shape, device="cuda", generator=gen) + 0x80 * torch.randint(0, 2, shape, device="cuda", generator=gen)
    return c.to(torch.half)


def pools(B, N, Hkv, D, ks, vs, gen):
    """[(bf16 set, FP8 set of the same content and table)]: the FP8 pools hold random codes, the bf16 pools their values code * scale[h] (from
    the CPU's table of the 256 codes: no FP8 arithmetic of torch runs on the GPU here), rounded to bf16."""
    lut = torch.arange(256, dtype=torch.uint8).view(F8).float().cuda()
    per = 2 * B * Hkv * N * D * 2
    dense = rotating(lambda: tuple(codes((B, Hkv, N, D), gen) for _ in range(2)), per)
    out = []
    for (k, v) in dense:
        kp, vp, bt = paged_from(k, v, PAGE, gen)
        k8, v8 = kp.to(torch.uint8), vp.to(torch.uint8)
        value = lambda c, s: (lut[c.long()] * s.view(1, -1, 1, 1)).to(BF)  # noqa: E731
        out.append(((value(k8, ks), value(v8, vs), bt), (k8.view(F8), v8.view(F8), bt)))
    return out


def line(kind, name, ctx, sets, W, base, fp8):
    print("%-8s %-30s %6d %4d %7s %10.1f %10.1f %7.3f" % (kind, name, ctx, sets, "None" if W is None else str(W), base * 1e3, fp8 * 1e3,
                                                          base / fp8), flush=True)


def prefill_row(kind, name, Ts, ctx, shape, windows, gen):
    Hq, Hkv, D = shape
    B, tq = len(Ts), sum(Ts)
    N = -(-(ctx + max(Ts)) // PAGE) * PAGE
    ks, vs = scales(Hkv)
    sets = pools(B, N, Hkv, D, ks, vs, gen)
    q = torch.randn(tq, Hq, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
    sinks = torch.randn(Hq, device="cuda", generator=gen) * 2
    o = {(W, s): torch.empty_like(q) for W in windows for s in (0, 1)}
    sl = torch.tensor([ctx + t for t in Ts], dtype=torch.int32, device="cuda")
    cu = torch.tensor(offsets(Ts), dtype=torch.int32, device="cuda")

    def call(key, nxt):
        W, s = key
        kp, vp, bt = nxt()[s]
        if s:
            pkg.fa2_prefill_paged_varlen_window_sink_bf16_fp8(q, kp, vp, bt, sl, cu, ks, vs, W, sinks, o[key])
        else:
            pkg.fa2_prefill_paged_varlen_window_sink_bf16(q, kp, vp, bt, sl, cu, W, sinks, o[key])
    best = best_of({key: (lambda key=key, nxt=cycle(sets): call(key, nxt)) for key in o})
    for W in windows:
        line(kind, name, ctx, len(sets), W, best[(W, 0)], best[(W, 1)])
    for key in o:
        call(key, lambda: sets[0])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in o.values())
    for W in windows:  # the same logical content: the two agree to what quantising the cache costs
        assert float((o[(W, 0)].float() - o[(W, 1)].float()).abs().max()) < 0.25, W


def multi_row(kind, B, T, ctx, shape, windows, gen):
    Hq, Hkv, D = shape
    n = ctx + T
    N = -(-n // PAGE) * PAGE
    ks, vs = scales(Hkv)
    sets = pools(B, N, Hkv, D, ks, vs, gen)
    q = torch.randn(B, T, Hq, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
    sinks = torch.randn(Hq, device="cuda", generator=gen) * 2
    sl = torch.full((B,), n, dtype=torch.int32, device="cuda")
    plans = {W: pkg.fa2_decode_paged_multi_window_sink_bf16_fp8_plan(B, T, Hq, Hkv, N // PAGE, PAGE, D, W) for W in windows}
    for W in windows:
        assert plans[W] == pkg.fa2_decode_paged_multi_window_sink_bf16_plan(B, T, Hq, Hkv, N // PAGE, PAGE, D, W)
    o = {(W, s): torch.empty_like(q) for W in windows for s in (0, 1)}
    ws = {key: torch.empty(max(plans[key[0]][2], 16), dtype=torch.uint8, device="cuda") for key in o}

    def call(key, nxt):
        W, s = key
        kp, vp, bt = nxt()[s]
        if s:
            pkg.fa2_decode_paged_multi_window_sink_bf16_fp8(q, kp, vp, bt, sl, ks, vs, W, sinks, o[key], None, ws[key])
        else:
            pkg.fa2_decode_paged_multi_window_sink_bf16(q, kp, vp, bt, sl, W, sinks, o[key], None, ws[key])
    best = best_of({key: (lambda key=key, nxt=cycle(sets): call(key, nxt)) for key in o})
    for W in windows:
        line(kind, "%s G=%d D=%d TG=%d S=%d" % ((B, T), Hq // Hkv, D, T * Hq // Hkv, plans[W][0]), ctx, len(sets), W, best[(W, 0)], best[(W, 1)])
    for key in o:
        call(key, lambda: sets[0])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in o.values())
    for W in windows:
        assert float((o[(W, 0)].float() - o[(W, 1)].float()).abs().max()) < 0.25, W


def append_row(name, Ts, ctx, shape, gen):
    Hq, Hkv, D = shape
    B, tq = len(Ts), sum(Ts)
    N = -(-(ctx + max(Ts)) // PAGE) * PAGE
    ks, vs = scales(Hkv)
    sets = pools(B, N, Hkv, D, ks, vs, gen)
    k_new, v_new = (torch.randn(tq, Hkv, D, dtype=torch.half, device="cuda", generator=gen).to(BF) for _ in range(2))
    q = torch.randn(tq, Hq, D, dtype=torch.half, device="cuda", generator=gen).to(BF)
    qo = {s: torch.empty_like(q) for s in (0, 1)}
    sl = torch.tensor([ctx + t for t in Ts], dtype=torch.int32, device="cuda")
    cu = torch.tensor(offsets(Ts), dtype=torch.int32, device="cuda")
    table = pkg.kv_append_rope_table(N, D, device="cuda")

    def call(s, nxt):
        kp, vp, bt = nxt()[s]
        if s:
            pkg.kv_append_paged_varlen_bf16_fp8(k_new, v_new, kp, vp, bt, sl, cu, ks, vs, q, qo[s], table, "half")
        else:
            pkg.kv_append_paged_varlen_bf16(k_new, v_new, kp, vp, bt, sl, cu, q, qo[s], table, "half")
    best = best_of({s: (lambda s=s, nxt=cycle(sets): call(s, nxt)) for s in (0, 1)})
    line("append", name, ctx, len(sets), None, best[0], best[1])
    torch.cuda.synchronize()
    assert torch.equal(qo[0], qo[1])  # the q rows are the sibling's


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip", nargs="*", default=[], choices=["prefill", "multi", "append"])
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    print("bf16 paged entries over FP8 (e4m3) pools against their bf16 siblings, page %d: us per call (launch-inclusive); x = bf16 sibling time / "
          "FP8 entry time (above 1: the FP8 entry is faster); multi: S = splits, TG = query rows per KV head" % PAGE)
    print("%-8s %-30s %6s %4s %7s %10s %10s %7s" % ("entry", "batch", "ctx", "sets", "W", "bf16 us", "fp8 us", "x"))
    if "multi" not in a.skip:
        for (shape, B, T, ctx) in MULTI:
            multi_row("multi", B, T, ctx, shape, WINDOWS, gen)
            torch.cuda.empty_cache()
    if "prefill" not in a.skip:
        for (B, T, _) in (UNIFORM[1], UNIFORM[3], UNIFORM[4]):
            prefill_row("prefill", "%d x T=%d D=128" % (B, T), [T] * B, CTX, HEADLINE, WINDOWS, gen)
            torch.cuda.empty_cache()
        prefill_row("prefill", batch_name(RAGGED[1]) + " D=128", RAGGED[1], CTX, HEADLINE, WINDOWS, gen)
        torch.cuda.empty_cache()
        prefill_row("prefill", "4 x T=512 D=64 gpt-oss", [512] * 4, CTX, GPT_OSS, (128, None), gen)
        torch.cuda.empty_cache()
    if "append" not in a.skip:
        append_row("64 x T=1 gpt-oss", [1] * 64, CTX, GPT_OSS, gen)
        append_row("4 x T=512 gpt-oss", [512] * 4, CTX, GPT_OSS, gen)
        append_row("64 x T=1 D=128", [1] * 64, CTX, HEADLINE, gen)
