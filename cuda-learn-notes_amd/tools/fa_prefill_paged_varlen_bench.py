"""GPU timing of the packed variable-length paged entries (cuda_learn_notes_amd.fa2_prefill_paged_varlen, kv_append_paged_varlen) against the
fixed-T entries, all in the same process on the same shuffled pools (paged_from of fa_decode_paged_bench.py), in the method of
fa_prefill_paged_bench.py: launch-inclusive times from one pair of device events around back-to-back calls after a warm-up, every timed window
>= 0.1 s, best of ROUNDS alternating rounds, the pools rotating over sets that together exceed the 256 MiB Infinity Cache (one set where a single
one already does).
  uniform   every sequence with the same T: 'varlen' on the packed [B T, Hq, D] tensor against 'fixed' = fa2_prefill_paged on [B, T, Hq, D] --
            the same tiles, the difference is the slot search and the B empty slots per KV head;
  ragged    chunk lengths T_b over a common context ctx (len_b = ctx + T_b): 'varlen' against (a) 'padded' = ONE fixed-T call with T = max T_b on
            the right-aligned [B, max T, Hq, D] tensor (the same lengths: the dead slots see no key) and (b) 'per-seq' = B fixed-T calls, one
            per sequence on prebuilt views; and the append (rope 'half', q rotated) in the same three forms.
  python fa_prefill_paged_varlen_bench.py [--skip uniform ragged]"""
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
from fa_prefill_paged_bench import best_of  # noqa: E402

HQ, HKV, D, PAGE = 32, 8, 128, 16
UNIFORM = [(1, 64, 16384), (1, 512, 4096), (1, 2048, 0), (4, 64, 4096), (4, 512, 4096), (4, 2048, 16384)]  # (B, T, ctx): the headline shapes
RAGGED = [[2048, 512, 64, 17], [512] + [1] * 63]
RAGGED_CTX = (0, 4096)


def pools_for(B, N, gen):
    per = 2 * B * HKV * N * D * 2
    dense = rotating(lambda: tuple(torch.randn(B, HKV, N, D, dtype=torch.half, device="cuda", generator=gen) for _ in range(2)), per)
    return [paged_from(k, v, PAGE, gen) for (k, v) in dense]


def cycle(pools):
    i = [0]

    def nxt():
        i[0] += 1
        return pools[i[0] % len(pools)]
    return nxt


def uniform(gen):
    print("uniform batches, Hq = %d, Hkv = %d, D = %d, page %d: us per call; x = varlen time / fixed time" % (HQ, HKV, D, PAGE))
    print("%-20s %4s %10s %10s %7s" % ("(B, T, ctx)", "sets", "fixed us", "varlen us", "x"))
    for (B, T, ctx) in UNIFORM:
        N = ctx + T
        pools = pools_for(B, N, gen)
        q = torch.randn(B, T, HQ, D, dtype=torch.half, device="cuda", generator=gen)
        qp = q.view(B * T, HQ, D)
        o, op = torch.empty_like(q), torch.empty_like(qp)
        sl = torch.full((B,), N, dtype=torch.int32, device="cuda")
        cu = (torch.arange(B + 1, device="cuda") * T).to(torch.int32)
        pf, pv = cycle(pools), cycle(pools)

        def fixed():
            kp, vp, bt = pf()
            pkg.fa2_prefill_paged(q, kp, vp, bt, sl, o)

        def varlen():
            kp, vp, bt = pv()
            pkg.fa2_prefill_paged_varlen(qp, kp, vp, bt, sl, cu, op)
        best = best_of({"fixed": fixed, "varlen": varlen})
        kp, vp, bt = pools[0]
        pkg.fa2_prefill_paged(q, kp, vp, bt, sl, o)
        pkg.fa2_prefill_paged_varlen(qp, kp, vp, bt, sl, cu, op)
        torch.cuda.synchronize()
        assert torch.equal(o.view(B * T, HQ, D), op)  # the same bits
        print("%-20s %4d %10.1f %10.1f %7.3f" % (str((B, T, ctx)), len(pools), best["fixed"] * 1e3, best["varlen"] * 1e3, best["varlen"] / best["fixed"]),
              flush=True)
        del pools
        torch.cuda.empty_cache()


def ragged(gen):
    print("ragged batches, Hq = %d, Hkv = %d, D = %d, page %d, len_b = ctx + T_b: us per call; padded = one fixed-T call with T = max T_b on the "
          "right-aligned tensor, per-seq = B fixed-T calls; x = that time / varlen time; rows = padded rows / live rows" % (HQ, HKV, D, PAGE))
    print("%-9s %-22s %5s %6s %10s %10s %7s %10s %7s" % ("entry", "T_b", "ctx", "rows", "varlen us", "padded us", "x", "per-seq us", "x"))
    for Ts in RAGGED:
        for ctx in RAGGED_CTX:
            B, Tm, tq = len(Ts), max(Ts), sum(Ts)
            N = -(-(ctx + Tm) // PAGE) * PAGE
            pools = pools_for(B, N, gen)
            lens = [ctx + t for t in Ts]
            sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
            cu_l = [0]
            for t in Ts:
                cu_l.append(cu_l[-1] + t)
            cu = torch.tensor(cu_l, dtype=torch.int32, device="cuda")
            half = lambda *s: torch.randn(*s, dtype=torch.half, device="cuda", generator=gen)  # noqa: E731
            qp, knp, vnp = half(tq, HQ, D), half(tq, HKV, D), half(tq, HKV, D)
            op, qop = torch.empty_like(qp), torch.empty_like(qp)
            qpad, knpad, vnpad = (torch.zeros(B, Tm, x.shape[1], D, dtype=torch.half, device="cuda") for x in (qp, knp, vnp))
            for b, t in enumerate(Ts):  # right-aligned: the live tokens are the last T_b
                for dst, src in ((qpad, qp), (knpad, knp), (vnpad, vnp)):
                    dst[b, Tm - t:] = src[cu_l[b]:cu_l[b + 1]]
            opad, qopad = torch.empty_like(qpad), torch.empty_like(qpad)
            per = [(qp[cu_l[b]:cu_l[b + 1]][None], knp[cu_l[b]:cu_l[b + 1]][None], vnp[cu_l[b]:cu_l[b + 1]][None], sl[b:b + 1],
                    torch.empty(1, Ts[b], HQ, D, dtype=torch.half, device="cuda"), torch.empty(1, Ts[b], HQ, D, dtype=torch.half, device="cuda"))
                   for b in range(B)]
            rope = pkg.kv_append_rope_table(N, D, device="cuda")
            rows = [[bt[b:b + 1].contiguous() for b in range(B)] for (_, _, bt) in pools]
            nxt = {n: cycle(list(zip(pools, rows))) for n in ("v", "p", "s", "av", "ap", "as")}

            def att_varlen():
                (kp, vp, bt), _ = nxt["v"]()
                pkg.fa2_prefill_paged_varlen(qp, kp, vp, bt, sl, cu, op)

            def att_padded():
                (kp, vp, bt), _ = nxt["p"]()
                pkg.fa2_prefill_paged(qpad, kp, vp, bt, sl, opad)

            def att_per_seq():
                (kp, vp, _), r = nxt["s"]()
                for b in range(B):
                    pkg.fa2_prefill_paged(per[b][0], kp, vp, r[b], per[b][3], per[b][4])

            def app_varlen():
                (kp, vp, bt), _ = nxt["av"]()
                pkg.kv_append_paged_varlen(knp, vnp, kp, vp, bt, sl, cu, qp, qop, rope, "half")

            def app_padded():
                (kp, vp, bt), _ = nxt["ap"]()
                pkg.kv_append_paged(knpad, vnpad, kp, vp, bt, sl, qpad, qopad, rope, "half")

            def app_per_seq():
                (kp, vp, _), r = nxt["as"]()
                for b in range(B):
                    pkg.kv_append_paged(per[b][1], per[b][2], kp, vp, r[b], per[b][3], per[b][0], per[b][5], rope, "half")
            name = str(Ts) if len(Ts) <= 4 else "[%d] + [1] x %d" % (Ts[0], len(Ts) - 1)
            for entry_name, calls in (("attention", {"varlen": att_varlen, "padded": att_padded, "per-seq": att_per_seq}),
                                      ("append", {"varlen": app_varlen, "padded": app_padded, "per-seq": app_per_seq})):
                best = best_of(calls)
                print("%-9s %-22s %5d %6.2f %10.1f %10.1f %7.2f %10.1f %7.2f" % (entry_name, name, ctx, B * Tm / float(tq), best["varlen"] * 1e3,
                                                                               best["padded"] * 1e3, best["padded"] / best["varlen"],
                                                                               best["per-seq"] * 1e3, best["per-seq"] / best["varlen"]), flush=True)
            kp, vp, bt = pools[0]  # one pool for both: the appends above have written into the sets
            pkg.fa2_prefill_paged_varlen(qp, kp, vp, bt, sl, cu, op)
            pkg.fa2_prefill_paged(qpad, kp, vp, bt, sl, opad)
            torch.cuda.synchronize()
            for b, t in enumerate(Ts):  # the packed call computes what the padded call computes
                assert torch.equal(op[cu_l[b]:cu_l[b + 1]], opad[b, Tm - t:]), b
            del pools, rows, nxt
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip", nargs="*", default=[], choices=["uniform", "ragged"])
    a = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(0)
    if "uniform" not in a.skip:
        uniform(gen)
    if "ragged" not in a.skip:
        ragged(gen)
