"""GPU timing of paged prefill attention (cuda_learn_notes_amd.fa2_prefill_paged, cln_fa2_prefill_paged) against what serves the same problem
without it, all in the same process on the same shuffled pools (paged_from of fa_decode_paged_bench.py: the sequences' pages interleaved, placed by
a random permutation), every sequence with `ctx` tokens in front of its T new ones (len = ctx + T):
  (a) 'multi'  ceil(T / 8) back-to-back fa2_decode_paged_multi calls, 8 tokens each, with prebuilt device length vectors ctx + 8, ctx + 16, ...,
               prebuilt q slices and one workspace: each call streams the whole cache below its length again;
  (b) 'torch'  the torch composition: gather the pages to a dense cache through the table, expand the KV heads to Hq, and
               scaled_dot_product_attention with the explicit boolean mask j < ctx + t + 1 (prebuilt); 'sdpa' is the last step alone on a
               prebuilt dense, expanded cache, 'torch' all three;
  (c) 'dense'  for information, on the rows both serve (G = 1, ctx = 0, T % 256 == 0): fa2_fwd_causal on the dense [B,H,T,D] tensors.
Times are launch-inclusive, from one pair of device events around back-to-back calls after a warm-up (bench_utils.time_region_events), every timed
window >= 0.1 s, best of ROUNDS alternating rounds; the pools rotate over sets that together exceed the 256 MiB Infinity Cache (one set where a
single one already does). TF/s = 4 D Hq B (T ctx + T (T + 1) / 2) flop -- the two products over the visible keys only -- / prefill time.
  python fa_prefill_paged_bench.py [--B 1 4] [--T 64 512 2048] [--ctx 0 4096 16384] [--page 16 64] [--skip torch dense]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from cuda_learn_notes_amd import bench_utils as bu  # noqa: E402
from fa_decode_paged_bench import paged_from, rotating  # noqa: E402

HQ, HKV = 32, 8
BS, TS, CTXS, PAGES = (1, 4), (64, 512, 2048), (0, 4096, 16384), (16, 64)
ROUNDS = 2
MULTI_T = 8


def timed(fn):
    """ms per call: a warm-up, a first estimate, then one event pair around a window of at least 0.1 s."""
    fn()
    torch.cuda.synchronize()
    ms = bu.time_region_events(fn, 2)
    if ms < 2.0:
        bu.prewarm(fn, 0.05)
    return bu.time_region_events(fn, max(3, int(100.0 / max(ms, 1e-3)) + 1))


def best_of(calls):
    best = {n: float("inf") for n in calls}
    for _ in range(ROUNDS):
        for n, f in calls.items():
            best[n] = min(best[n], timed(f))
    torch.cuda.synchronize()
    return best


def gather_dense(kp, vp, bt, G):
    """The pools as dense caches expanded to the query heads: [B, Hkv G, max_pages page, D] each."""
    out = []
    for p in (kp, vp):
        P, Hkv, page, D = p.shape
        d = p[bt.long()].permute(0, 2, 1, 3, 4).reshape(bt.shape[0], Hkv, bt.shape[1] * page, D)
        out.append(d.repeat_interleave(G, dim=1) if G > 1 else d.contiguous())
    return out


def row(B, T, ctx, page, D, Hq, Hkv, gen, skip):
    import torch.nn.functional as F
    N, G = ctx + T, Hq // Hkv
    assert N % page == 0
    per = 2 * B * Hkv * N * D * 2
    dense = rotating(lambda: tuple(torch.randn(B, Hkv, N, D, dtype=torch.half, device="cuda", generator=gen) for _ in range(2)), per)
    pools = [paged_from(k, v, page, gen) for (k, v) in dense]
    q = torch.randn(B, T, Hq, D, dtype=torch.half, device="cuda", generator=gen)
    o = torch.empty_like(q)
    sl = torch.full((B,), N, dtype=torch.int32, device="cuda")
    calls, i = {}, {"prefill": 0, "multi": 0, "torch": 0}

    def pool(name):
        i[name] += 1
        return pools[i[name] % len(pools)]

    def prefill():
        kp, vp, bt = pool("prefill")
        pkg.fa2_prefill_paged(q, kp, vp, bt, sl, o)
    calls["prefill"] = prefill

    chunks = -(-T // MULTI_T)
    qs = [q[:, MULTI_T * c:MULTI_T * (c + 1)].contiguous() for c in range(chunks)]
    os_ = [torch.empty_like(x) for x in qs]
    sls = [torch.full((B,), ctx + min(MULTI_T * (c + 1), T), dtype=torch.int32, device="cuda") for c in range(chunks)]
    need = max(pkg.fa2_decode_paged_multi_plan(B, x.shape[1], Hq, Hkv, N // page, page, D)[2] for x in (qs[0], qs[-1]))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")

    def multi():
        kp, vp, bt = pool("multi")
        for c in range(chunks):
            pkg.fa2_decode_paged_multi(qs[c], kp, vp, bt, sls[c], os_[c], None, ws)
    calls["multi"] = multi

    if "torch" not in skip:
        qt = q.transpose(1, 2)  # [B,Hq,T,D], a view: what a caller of the composition holds
        mask = torch.arange(N, device="cuda")[None, :] < (ctx + 1 + torch.arange(T, device="cuda"))[:, None]  # [T, N]
        ke, ve = gather_dense(*pools[0], G)

        def sdpa():
            F.scaled_dot_product_attention(qt, ke, ve, attn_mask=mask)

        def composed():
            k1, v1 = gather_dense(*pool("torch"), G)
            F.scaled_dot_product_attention(qt, k1, v1, attn_mask=mask)
        calls["sdpa"], calls["torch"] = sdpa, composed

    if "dense" not in skip and G == 1 and ctx == 0 and T % 256 == 0:
        qd = q.transpose(1, 2).contiguous()
        od = torch.empty_like(qd)
        kd, vd = dense[0]

        def causal():
            pkg.fa2_fwd_causal(qd, kd, vd, od)
        calls["dense"] = causal

    best = best_of(calls)
    if "torch" not in skip:  # the composition computes what the entry computes
        ref = F.scaled_dot_product_attention(qt, *gather_dense(*pools[i["prefill"] % len(pools)], G), attn_mask=mask).transpose(1, 2)
        err = (o.float() - ref.float()).abs().max().item()
        assert err < 6e-3, err
    flop = 4.0 * D * Hq * B * (T * ctx + T * (T + 1) / 2.0)
    cell = lambda n: "%10.1f %7.2f" % (best[n] * 1e3, best[n] / best["prefill"]) if n in best else "%10s %7s" % ("-", "-")  # noqa: E731
    print("%-22s %-4d %-2d %3d %11.1f %8.1f %s %s %s %s" % (str((B, T, ctx, D)), page, G, len(pools), best["prefill"] * 1e3,
                                                         flop / best["prefill"] * 1e-9, cell("multi"), cell("sdpa"), cell("torch"), cell("dense")),
          flush=True)
    ok = best["multi"] > best["prefill"] if T >= 64 else True
    return ok and ("torch" not in best or best["torch"] > best["prefill"])


def table(Bs, Ts, ctxs, pages, skip):
    print("paged prefill attention, Hq = %d, Hkv = %d unless the row says G = 1 (then Hq = Hkv = %d): us per call (launch-inclusive, best of %d "
          "rounds); TF/s = 4 D Hq B (T ctx + T (T + 1) / 2) / prefill time; multi = ceil(T / 8) fa2_decode_paged_multi calls; sdpa = torch "
          "scaled_dot_product_attention with the explicit mask on a prebuilt dense, head-expanded cache; torch = gather + expand + that; dense = "
          "fa2_fwd_causal (information only); x = that time / prefill time; sets = rotating pool sets" % (HQ, HKV, HQ, ROUNDS))
    print("%-22s %-4s %-2s %3s %11s %8s %10s %7s %10s %7s %10s %7s %10s %7s" % ("(B, T, ctx, D)", "page", "G", "sets", "prefill us", "TF/s", "multi us",
                                                                            "x", "sdpa us", "x", "torch us", "x", "dense us", "x"))
    gen = torch.Generator(device="cuda").manual_seed(0)
    ok = True
    for page in pages:
        for B in Bs:
            for T in Ts:
                for ctx in ctxs:
                    ok &= row(B, T, ctx, page, 128, HQ, HKV, gen, skip)
                    torch.cuda.empty_cache()
    ok &= row(max(Bs), 512, 4096, 16, 64, HQ, HKV, gen, skip)  # one D = 64 row
    for B in Bs:  # the rows the dense causal kernel serves too
        for T in (t for t in Ts if t % 256 == 0):
            ok &= row(B, T, 0, 64, 128, HQ, HQ, gen, skip)
            torch.cuda.empty_cache()
    print("orderings (prefill faster than multi on every row with T >= 64, and than torch including the gather): %s" % ("hold" if ok else "VIOLATED"))
    return ok


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=list(BS))
    ap.add_argument("--T", type=int, nargs="+", default=list(TS))
    ap.add_argument("--ctx", type=int, nargs="+", default=list(CTXS))
    ap.add_argument("--page", type=int, nargs="+", default=list(PAGES))
    ap.add_argument("--skip", nargs="*", default=[], choices=["torch", "dense"])
    a = ap.parse_args()
    table(a.B, a.T, a.ctx, a.page, a.skip)
