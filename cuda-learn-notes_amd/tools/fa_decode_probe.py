"""GPU sweep behind the split plan of decode attention (cln_fa2_decode_plan, csrc/flash_attn_decode.hip): every shape is timed with the keys of
a head cut into S = 1, 2, 4, ... chunks through the probe library's cln_fa2_decode_variant (explicit S and C), next to the plan's own pick.
The plan's three constants -- the number of workgroups worth reaching, the smallest chunk worth a workgroup, the cap on S -- are read off this
table. Launch-inclusive times (both kernels of a split call), K / V rotating over sets that together exceed the 256 MiB Infinity Cache, all
lengths equal to Nmax; device events around back-to-back calls, windows >= 0.1 s after a warm-up, best of 2 rounds.
  python fa_decode_probe.py"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from cuda_learn_notes_amd import _loader  # noqa: E402
from cuda_learn_notes_amd import bench_utils as bu  # noqa: E402

SHAPES = [(1, 32, 8192, 128), (8, 32, 4096, 128), (64, 32, 2048, 128), (1, 32, 32768, 64), (32, 8, 1024, 64),
          (1, 8, 4096, 128), (1, 8, 65536, 128), (4, 32, 1024, 128), (16, 32, 2048, 128), (2, 8, 512, 64), (1, 1, 65536, 64), (32, 32, 512, 128)]
SPLITS = (1, 2, 4, 8, 16, 32, 64, 128)
ROTATE_BYTES = 640 << 20


def key_step(D):
    return 4 * 4 * (64 * 8 // D)


def variant_fn():
    fn = _loader.load_so("libcln_amd_probe.so").cln_fa2_decode_variant
    fn.argtypes = [ctypes.c_void_p] * 7 + [ctypes.c_longlong] + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def cache_sets(B, H, N, D):
    per = 2 * B * H * N * D * 2
    n = max(2, min(40, -(-ROTATE_BYTES // per)))
    return [(torch.randn(B, H, N, D, dtype=torch.half, device="cuda"), torch.randn(B, H, N, D, dtype=torch.half, device="cuda")) for _ in range(n)]


def timed(fn):
    bu.prewarm(fn, 0.05)
    ms = bu.time_region_events(fn, 5)
    return bu.time_region_events(fn, max(10, int(100.0 / max(ms, 1e-3)) + 1))


def main():
    fn = variant_fn()
    stream = torch.cuda.current_stream().cuda_stream
    print("decode attention, explicit split plans: us per call (launch-inclusive), live GB/s = 2 B H N D 2 bytes / time; * = the plan's pick")
    for (B, H, N, D) in SHAPES:
        torch.manual_seed(0)
        sets = cache_sets(B, H, N, D)
        q = torch.randn(B, H, D, dtype=torch.half, device="cuda")
        o = torch.empty_like(q)
        lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
        pS, pC, _ = pkg.fa2_decode_plan(B, H, N, D)
        step = key_step(D)
        cands = []
        for want in SPLITS:
            C = -(-(-(-N // want)) // step) * step
            S = -(-N // C)
            if (S, C) not in cands:
                cands.append((S, C))
        if (pS, pC) not in cands:
            cands.append((pS, pC))
        ws = torch.empty(max(B * H * max(s for s, _ in cands) * (D + 2) * 4, 16), dtype=torch.uint8, device="cuda")
        best = {c: float("inf") for c in cands}
        for _ in range(2):
            for (S, C) in cands:
                i = [0]

                def call():
                    k, v = sets[i[0] % len(sets)]
                    i[0] += 1
                    rc = fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), lens.data_ptr(), o.data_ptr(), None, ws.data_ptr(), ws.numel(), B, H, N, D, S, C, stream)
                    assert rc == 0, rc
                best[(S, C)] = min(best[(S, C)], timed(call))
        torch.cuda.synchronize()
        live = 2.0 * B * H * N * D * 2
        fastest = min(best.values())
        for (S, C) in cands:
            ms = best[(S, C)]
            print("%-22s S=%-4d C=%-6d workgroups=%-7d %9.2f us %8.1f GB/s  %5.2fx fastest %s" % (
                str((B, H, N, D)), S, C, B * H * S, ms * 1e3, live / ms * 1e-6, ms / fastest, "*" if (S, C) == (pS, pC) else ""), flush=True)
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
