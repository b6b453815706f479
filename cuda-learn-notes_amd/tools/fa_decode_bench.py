"""GPU timing of decode attention (cuda_learn_notes_amd.fa2_decode, cln_fa2_decode) against torch scaled_dot_product_attention fp16 with a
length-1 query on the same caches, and the measured error of the kernel against the bound of its tests.
Times are launch-inclusive (for a split plan: both kernels), K / V rotating over sets that together exceed the 256 MiB Infinity Cache -- the
method of the bandwidth rows; device events around back-to-back calls after a warm-up, every timed window >= 0.1 s, best of 3 alternating
rounds. Live bytes of a call: 2 sum_b len_b H D 2 (the K and V rows below the lengths; q, O and the workspace are not counted). SDPA has no
per-sequence lengths: it runs the equal-length rows only.
  python fa_decode_bench.py              the table, then the accuracy figures
  python fa_decode_bench.py --accuracy   the accuracy figures only"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from cuda_learn_notes_amd import bench_utils as bu  # noqa: E402

SHAPES = [(1, 32, 8192, 128), (8, 32, 4096, 128), (64, 32, 2048, 128), (1, 32, 32768, 64), (32, 8, 1024, 64)]
ROTATE_BYTES = 640 << 20
COPY_CEILING_TBS = 6.29  # hipMemcpyDtoD on this chip


def timed(fn):
    bu.prewarm(fn, 0.1)
    ms = bu.time_region_events(fn, 5)
    return bu.time_region_events(fn, max(10, int(100.0 / max(ms, 1e-3)) + 1))


def ragged_lengths(B, N):
    """One ragged batch per shape: lengths spread evenly over (0, N], the longest equal to N (B = 1: three quarters of N)."""
    return [N * (b + 1) // B for b in range(B)] if B > 1 else [3 * N // 4]


def table():
    sdpa = torch.nn.functional.scaled_dot_product_attention
    print("decode attention: ms per call (launch-inclusive), live TB/s = 2 sum(len) H D 2 bytes / time; copy ceiling %.2f TB/s; SDPA = torch fp16 "
          "scaled_dot_product_attention, query length 1" % COPY_CEILING_TBS)
    print("%-22s %-8s %-12s %9s %8s %7s %9s %9s" % ("(B, H, len, D)", "lengths", "plan", "ms", "TB/s", "of copy", "sdpa ms", "ours/sdpa"))
    for (B, H, N, D) in SHAPES:
        torch.manual_seed(0)
        per = 2 * B * H * N * D * 2
        nsets = max(2, min(40, -(-ROTATE_BYTES // per)))
        sets = [(torch.randn(B, H, N, D, dtype=torch.half, device="cuda"), torch.randn(B, H, N, D, dtype=torch.half, device="cuda")) for _ in range(nsets)]
        q = torch.randn(B, H, D, dtype=torch.half, device="cuda")
        q4 = q.view(B, H, 1, D)
        o = torch.empty_like(q)
        S, C, need = pkg.fa2_decode_plan(B, H, N, D)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
        for kind, lens in (("equal", [N] * B), ("ragged", ragged_lengths(B, N))):
            sl = torch.tensor(lens, dtype=torch.int32, device="cuda")
            i, j = [0], [0]

            def ours():
                k, v = sets[i[0] % nsets]
                i[0] += 1
                pkg.fa2_decode(q, k, v, sl, o, None, ws)

            def theirs():
                k, v = sets[j[0] % nsets]
                j[0] += 1
                sdpa(q4, k, v)

            calls = {"ours": ours}
            if kind == "equal":
                calls["sdpa"] = theirs
            best = {n: float("inf") for n in calls}
            for _ in range(3):
                for n, f in calls.items():
                    best[n] = min(best[n], timed(f))
            torch.cuda.synchronize()
            live = 2.0 * sum(lens) * H * D * 2
            tbs = live / best["ours"] * 1e-9
            sd = best.get("sdpa")
            print("%-22s %-8s %-12s %9.4f %8.3f %6.1f%% %9s %9s" % (
                str((B, H, N, D)), kind, "S=%d C=%d" % (S, C), best["ours"], tbs, 100.0 * tbs / COPY_CEILING_TBS,
                "%.4f" % sd if sd else "-", "%.3f" % (best["ours"] / sd) if sd else "-"), flush=True)
        del sets
        torch.cuda.empty_cache()


def accuracy():
    """Worst error / bound of the test rules (tests/decode_reference.py: fa_tol for O, 2^-10 max(1, max|LSE|) for LSE) per head dim, over the
    shapes and boundary lengths of tests/test_gpu_fa2_decode.py on seeds those tests do not use."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import decode_reference as dr
    import test_gpu_fa2_decode as t
    print("accuracy against the fp64 reference: worst error / bound over the test shapes and boundary lengths, seed 9 (the tests use 0 and 1)")
    for D in t.DS:
        worst_o = worst_l = 0.0
        for (B, H, Nmax) in t.SHAPES:
            q, k, v = t.problem(B, H, Nmax, D, seed=9)
            qd, kd, vd = (x.cuda() for x in (q, k, v))
            for n in t.lengths_for(B, H, Nmax, D):
                o, lse = t.run(qd, kd, vd, [n] * B)
                ro, rl = dr.ref_decode(q, k, v, [n] * B)
                worst_o = max(worst_o, (o.double() - ro).abs().max().item() / dr.fa_tol(ro))
                worst_l = max(worst_l, (lse.double() - rl).abs().max().item() / dr.lse_tol(rl))
        print("D=%-4d O: worst error / fa_tol = %.4f    LSE: worst error / (2^-10 max(1, max|LSE|)) = %.5f" % (D, worst_o, worst_l), flush=True)


if __name__ == "__main__":
    if "--accuracy" not in sys.argv:
        table()
    accuracy()
