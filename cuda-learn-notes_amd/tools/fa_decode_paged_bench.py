"""GPU timing of paged decode attention with grouped query heads (cuda_learn_notes_amd.fa2_decode_paged, cln_fa2_decode_paged) against the only
way fa2_decode serves the same logical problem: a dense cache [B,Hq,len,D] with K and V expanded to the query head count (at G = 1: the dense
cache itself). Both run in the same process on the same data; the pages of the pool are shuffled, the sequences' pages interleaved.
Times are launch-inclusive (for a split plan: both kernels), the caches rotating over sets that together exceed the 256 MiB Infinity Cache (one set
where a single one already does) -- the method of fa_decode_bench.py; one pair of device events around back-to-back calls after a warm-up, every
timed window >= 0.1 s, best of 3 alternating rounds. The G = 1 dense row is measured REPEATS times on its own (best of 3 each) and printed as
min .. max: the run-to-run spread a paged / dense ratio has to be read against.
Bytes of a call: 2 sum_b len_b Hkv D 2 -- the K and V rows below the lengths, ONCE PER KV HEAD, for every row of the table (the
expanded dense call streams G times that; its GB/s column is on the same logical bytes, so the columns compare as times do).
  python fa_decode_paged_bench.py"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from cuda_learn_notes_amd import bench_utils as bu  # noqa: E402

BS, HKV, GS, DS, LENS, PAGES = (1, 8, 64), 8, (1, 4, 8), (64, 128), (4096, 32768), (16, 128)
ROTATE_BYTES = 640 << 20
MAX_SETS = 40
REPEATS = 5


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


def rotating(make, per_bytes):
    """`make()` called for as many sets as exceed the Infinity Cache together (one where a single set already does)."""
    n = max(1, min(MAX_SETS, -(-ROTATE_BYTES // per_bytes)))
    return [make() for _ in range(n)]


def paged_from(kd, vd, page, gen):
    """(k_pages, v_pages, block_table) holding dense kd, vd [B,Hkv,N,D]: P = B N / page pages placed by a random permutation of the interleaved
    order (page i of sequence 0, of sequence 1, ..., page i + 1 of sequence 0, ...)."""
    B, Hkv, N, D = kd.shape
    mp = N // page
    perm = torch.randperm(B * mp, generator=gen, device="cuda")  # slot of the (i, b)-th page
    kp, vp = (torch.empty(B * mp, Hkv, page, D, dtype=torch.half, device="cuda") for _ in range(2))
    for dst, src in ((kp, kd), (vp, vd)):
        dst[perm] = src.view(B, Hkv, mp, page, D).permute(2, 0, 1, 3, 4).reshape(B * mp, Hkv, page, D)
    bt = perm.view(mp, B).t().contiguous().to(torch.int32)
    return kp, vp, bt


def table():
    print("paged decode attention, Hkv = %d: us per call (launch-inclusive); GB/s = 2 len B Hkv D 2 bytes / time (K and V once per KV head); "
          "'expanded' = fa2_decode on the dense cache with K, V expanded to Hq heads (G = 1: the dense cache); x = expanded time / paged time; "
          "dense G=1 spread = min .. max of %d separate measurements" % (HKV, REPEATS))
    print("%-16s %-4s %-2s %-14s %10s %9s %12s %7s   %s" % ("(B, len, D)", "page", "G", "plan", "paged us", "GB/s", "expanded us", "x", "dense G=1 us min .. max"))
    gen = torch.Generator(device="cuda").manual_seed(0)
    for D in DS:
        for N in LENS:
            for B in BS:
                per = 2 * B * HKV * N * D * 2
                dense = rotating(lambda: tuple(torch.randn(B, HKV, N, D, dtype=torch.half, device="cuda", generator=gen) for _ in range(2)), per)
                sl = torch.full((B,), N, dtype=torch.int32, device="cuda")
                spread = None
                for page in PAGES:
                    pools = [paged_from(k, v, page, gen) for (k, v) in dense]
                    for G in GS:
                        Hq = HKV * G
                        q = torch.randn(B, Hq, D, dtype=torch.half, device="cuda", generator=gen)
                        o = torch.empty_like(q)
                        S, C, need = pkg.fa2_decode_paged_plan(B, Hq, HKV, N // page, page, D)
                        ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
                        exp = dense if G == 1 else [tuple(t.repeat_interleave(G, dim=1) for t in kv) for kv in dense]
                        wsd = torch.empty(max(pkg.fa2_decode_plan(B, Hq, N, D)[2], 16), dtype=torch.uint8, device="cuda")
                        i, j = [0], [0]

                        def paged():
                            kp, vp, bt = pools[i[0] % len(pools)]
                            i[0] += 1
                            pkg.fa2_decode_paged(q, kp, vp, bt, sl, o, None, ws)

                        def expanded():
                            k, v = exp[j[0] % len(exp)]
                            j[0] += 1
                            pkg.fa2_decode(q, k, v, sl, o, None, wsd)

                        best = best_of({"paged": paged, "expanded": expanded})
                        if G == 1 and spread is None:
                            runs = [best["expanded"]] + [best_of({"expanded": expanded})["expanded"] for _ in range(REPEATS - 1)]
                            spread = (min(runs), max(runs))
                        live = 2.0 * B * N * HKV * D * 2
                        print("%-16s %-4d %-2d %-14s %10.2f %9.1f %12.2f %7.3f   %s" % (
                            str((B, N, D)), page, G, "S=%d C=%d" % (S, C), best["paged"] * 1e3, live / best["paged"] * 1e-6, best["expanded"] * 1e3,
                            best["expanded"] / best["paged"],
                            "%.2f .. %.2f (+%.1f%%)" % (spread[0] * 1e3, spread[1] * 1e3, 100.0 * (spread[1] / spread[0] - 1.0)) if G == 1 else ""), flush=True)
                        del exp
                    del pools
                del dense
                torch.cuda.empty_cache()


if __name__ == "__main__":
    table()
