"""GPU timing of multi-token paged decode attention (cuda_learn_notes_amd.fa2_decode_paged_multi, cln_fa2_decode_paged_multi) against the only
way the single-query entry serves the same problem: T back-to-back fa2_decode_paged calls on the same pool with the lengths len - T + 1 ... len.
Both run in the same process on the same shuffled pools (the sequences' pages interleaved, placed by a random permutation).
Times are launch-inclusive (for a split plan: both kernels; for the baseline: all T calls), the pools rotating over sets that together exceed the
256 MiB Infinity Cache (one set where a single one already does) -- the method of fa_decode_paged_bench.py; one pair of device events around
back-to-back calls after a warm-up, every timed window >= 0.1 s, best of 3 alternating rounds. For the first configuration of every (B, len, D)
the baseline is measured REPEATS times on its own (best of 3 each) and printed as min .. max: the run-to-run spread a ratio has to be read against.
Bytes of a call: 2 len B Hkv D 2 -- the K and V rows below the lengths ONCE PER KV HEAD and once per call, whatever T and G are (the baseline
streams T times that; its time is on the same logical problem, so the columns compare as times do).
  python fa_decode_paged_multi_bench.py [--D 64 128] [--len 4096 32768] [--B 1 8 64]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from fa_decode_paged_bench import REPEATS, best_of, paged_from, rotating  # noqa: E402

BS, HKV, GS, DS, TS, LENS, PAGES = (1, 8, 64), 8, (1, 4, 8), (64, 128), (2, 4, 8), (4096, 32768), (16, 128)


def table(Ds, lens, Bs):
    print("multi-token paged decode attention, Hkv = %d: us per call (launch-inclusive); GB/s = 2 len B Hkv D 2 bytes / multi time (K and V once "
          "per KV head and call); 'T x paged' = T fa2_decode_paged calls with the lengths len - T + 1 ... len; x = that time / multi time; "
          "'1 x paged' = one fa2_decode_paged call at len; baseline spread = min .. max of %d separate measurements of 'T x paged'" % (HKV, REPEATS))
    print("%-16s %-4s %-2s %-2s %-14s %10s %9s %12s %7s %11s   %s" % ("(B, len, D)", "page", "G", "T", "plan", "multi us", "GB/s", "T x paged us", "x",
                                                                       "1 x paged us", "T x paged us min .. max"))
    gen = torch.Generator(device="cuda").manual_seed(0)
    for D in Ds:
        for N in lens:
            for B in Bs:
                per = 2 * B * HKV * N * D * 2
                dense = rotating(lambda: tuple(torch.randn(B, HKV, N, D, dtype=torch.half, device="cuda", generator=gen) for _ in range(2)), per)
                first = True
                for page in PAGES:
                    pools = [paged_from(k, v, page, gen) for (k, v) in dense]
                    for G in GS:
                        Hq = HKV * G
                        ws1 = torch.empty(max(pkg.fa2_decode_paged_plan(B, Hq, HKV, N // page, page, D)[2], 16), dtype=torch.uint8, device="cuda")
                        for T in TS:
                            q = torch.randn(B, T, Hq, D, dtype=torch.half, device="cuda", generator=gen)
                            o = torch.empty_like(q)
                            qs = [q[:, t].contiguous() for t in range(T)]
                            os_ = [torch.empty_like(x) for x in qs]
                            sls = [torch.full((B,), N - T + 1 + t, dtype=torch.int32, device="cuda") for t in range(T)]
                            S, C, need = pkg.fa2_decode_paged_multi_plan(B, T, Hq, HKV, N // page, page, D)
                            ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
                            i, j, k1 = [0], [0], [0]

                            def multi():
                                kp, vp, bt = pools[i[0] % len(pools)]
                                i[0] += 1
                                pkg.fa2_decode_paged_multi(q, kp, vp, bt, sls[-1], o, None, ws)

                            def t_paged():
                                kp, vp, bt = pools[j[0] % len(pools)]
                                j[0] += 1
                                for t in range(T):
                                    pkg.fa2_decode_paged(qs[t], kp, vp, bt, sls[t], os_[t], None, ws1)

                            def one_paged():
                                kp, vp, bt = pools[k1[0] % len(pools)]
                                k1[0] += 1
                                pkg.fa2_decode_paged(qs[-1], kp, vp, bt, sls[-1], os_[-1], None, ws1)

                            best = best_of({"multi": multi, "t_paged": t_paged, "one": one_paged})
                            spread = ""
                            if first:
                                runs = [best["t_paged"]] + [best_of({"t_paged": t_paged})["t_paged"] for _ in range(REPEATS - 1)]
                                spread = "%.2f .. %.2f (+%.1f%%)" % (min(runs) * 1e3, max(runs) * 1e3, 100.0 * (max(runs) / min(runs) - 1.0))
                                first = False
                            live = 2.0 * B * N * HKV * D * 2
                            print("%-16s %-4d %-2d %-2d %-14s %10.2f %9.1f %12.2f %7.3f %11.2f   %s" % (
                                str((B, N, D)), page, G, T, "S=%d C=%d" % (S, C), best["multi"] * 1e3, live / best["multi"] * 1e-6,
                                best["t_paged"] * 1e3, best["t_paged"] / best["multi"], best["one"] * 1e3, spread), flush=True)
                    del pools
                del dense
                torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, nargs="+", default=list(DS))
    ap.add_argument("--len", type=int, nargs="+", default=list(LENS))
    ap.add_argument("--B", type=int, nargs="+", default=list(BS))
    a = ap.parse_args()
    table(a.D, a.len, a.B)
