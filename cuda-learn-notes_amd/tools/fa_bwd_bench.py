"""GPU timing of the attention backward (cuda_learn_notes_amd.fa2_bwd, cln_fa2_bwd / cln_fa2_bwd_causal) and of forward + backward through
fa2_attention, against torch scaled_dot_product_attention fp16 forward + backward and backward alone, causal and not.
FLOPs: backward 10 B H N^2 D, forward 4 B H N^2 D (both halved when causal). The per-kernel split (dQ / dK-dV): run the script under
rocprofv3 --kernel-trace --stats and read fa2_bwd_dq_kernel / fa2_bwd_dkdv_kernel in its stats file.
Device events around back-to-back launches after a warm-up; every timed window is >= 0.1 s; best of 3 alternating rounds.
  python fa_bwd_bench.py               the table
  python fa_bwd_bench.py --calibrate   the observed ratios max|X - X64| / max|X_sdpa - X64| of the test tolerance rule (seeds the tests do not use)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from cuda_learn_notes_amd import bench_utils as bu  # noqa: E402

SHAPES = [(4, 8, 2048, 64), (2, 32, 4096, 64), (2, 32, 4096, 128), (1, 32, 8192, 128)]


def timed(fn):
    bu.prewarm(fn, 0.1)
    ms = bu.time_region_events(fn, 5)
    iters = max(10, int(100.0 / max(ms, 1e-3)) + 1)
    return bu.time_region_events(fn, iters)


def sdpa_backend():
    try:
        from torch.nn.attention import SDPBackend, sdpa_kernel
    except ImportError:
        return "unknown"
    q = torch.randn(1, 8, 256, 64, dtype=torch.half, device="cuda", requires_grad=True)
    for b in (SDPBackend.FLASH_ATTENTION, SDPBackend.EFFICIENT_ATTENTION, SDPBackend.MATH):
        try:
            with sdpa_kernel([b]):
                torch.nn.functional.scaled_dot_product_attention(q, q, q, is_causal=True).sum().backward()
            return b.name  # the first backend in torch's own priority order that runs here
        except RuntimeError:
            continue
    return "none"


def table():
    sdpa = torch.nn.functional.scaled_dot_product_attention
    print("SDPA backend (first of torch's priority order that runs fp16 fwd+bwd here): %s" % sdpa_backend())
    print("bwd FLOPs = 10 B H N^2 D, fwd 4 B H N^2 D, halved when causal; times in ms (best of 3 alternating rounds)")
    print("%-20s %-6s %9s %7s %9s %7s %9s %7s %9s %7s %8s %8s" % ("shape", "causal", "bwd", "TF", "fwd+bwd", "TF", "sdpa_bwd", "TF",
                                                                 "sdpa_f+b", "TF", "bwd/sdpa", "fb/sdpa"))
    for shape in SHAPES:
        B, H, N, D = shape
        for causal in (False, True):
            torch.manual_seed(0)
            q, k, v, do = (torch.randn(B, H, N, D, dtype=torch.half, device="cuda") for _ in range(4))
            o = torch.empty_like(q)
            lse = torch.empty(B, H, N, dtype=torch.float32, device="cuda")
            pkg.fa2_fwd_lse(q, k, v, o, lse, causal=causal)
            dq, dk, dv = (torch.empty_like(q) for _ in range(3))
            delta = torch.empty_like(lse)
            qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
            so = sdpa(qa, ka, va, is_causal=causal)

            def ours_fb():
                qa.grad = ka.grad = va.grad = None
                pkg.fa2_attention(qa, ka, va, causal=causal).backward(do)

            def sdpa_fb():
                qa.grad = ka.grad = va.grad = None
                sdpa(qa, ka, va, is_causal=causal).backward(do)

            def sdpa_b():
                qa.grad = ka.grad = va.grad = None
                torch.autograd.backward(so, do, retain_graph=True)

            calls = {"bwd": lambda: pkg.fa2_bwd(q, k, v, o, do, lse, dq, dk, dv, delta=delta, causal=causal), "fb": ours_fb,
                     "sb": sdpa_b, "sfb": sdpa_fb}
            best = {n: float("inf") for n in calls}
            for _ in range(3):
                for n, f in calls.items():
                    best[n] = min(best[n], timed(f))
            torch.cuda.synchronize()
            c = 0.5 if causal else 1.0
            fb, ff = c * 10.0 * B * H * N * N * D, c * 4.0 * B * H * N * N * D
            print("%-20s %-6s %9.4f %7.1f %9.4f %7.1f %9.4f %7.1f %9.4f %7.1f %8.3f %8.3f" % (
                str(shape), causal, best["bwd"], fb / best["bwd"] * 1e-9, best["fb"], (fb + ff) / best["fb"] * 1e-9, best["sb"],
                fb / best["sb"] * 1e-9, best["sfb"], (fb + ff) / best["sfb"] * 1e-9, best["bwd"] / best["sb"], best["fb"] / best["sfb"]), flush=True)


def calibrate():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_fa2_bwd as t
    print("ratio r_X = max|X - X64| / max|X_sdpa - X64|, and e_X = max|X - X64| / max|X64| (2^-10 = %.2e); seeds 500.. (tests use others)" % 2.0 ** -10)
    worst = {}
    for i, (B, H, N, D, amp) in enumerate([(1, 8, 256, 64, 1), (1, 8, 512, 128, 1), (2, 3, 2048, 64, 1), (1, 8, 2048, 128, 1), (1, 8, 1024, 64, 4),
                                           (1, 8, 1024, 128, 4)]):
        for causal in (False, True):
            q, k, v, do = t.qkv(B, H, N, D, seed=500 + i, k_scale=amp)
            o, lse = t.fwd(q, k, v, causal)
            got = t.bwd(q, k, v, o, do, lse, causal)[:3]
            ref = t.ref64(q, k, v, do, causal)[2:]
            sd = t.sdpa_grads(q, k, v, do, causal)
            row = []
            for nm, x, x64, xs in zip(("dQ", "dK", "dV"), got, ref, sd):
                err = (t.flat(x) - x64).abs().max().item()
                es = (xs - x64).abs().max().item()
                r, e = err / es, err / x64.abs().max().item()
                worst[nm] = max(worst.get(nm, (0, 0)), (r, e))
                row.append("%s r=%.2f e=%.2e" % (nm, r, e))
            print("%-22s causal=%-5s %s" % (str((B, H, N, D)) + ("x%d" % amp if amp != 1 else ""), causal, "  ".join(row)), flush=True)
    print("worst (r, e): " + "  ".join("%s (%.2f, %.2e)" % (k, *v) for k, v in worst.items()))


if __name__ == "__main__":
    calibrate() if "--calibrate" in sys.argv else table()
