"""GPU timing of the two MFMA attention entries over an FP8 (e4m3fn) paged KV cache -- cuda_learn_notes_amd.fa2_decode_paged_multi_fp8 and
fa2_prefill_paged_fp8 -- each against its fp16 entry on an fp16 pool of the same logical content (the dequantised values, which fp16 holds
exactly), in the same process; and of fa2_decode_paged_multi_fp8 at T = 1 against the single-query VALU entry fa2_decode_paged_fp8 on the same
FP8 pool. The method is that of fa_decode_paged_fp8_bench.py: shuffled pools with the sequences interleaved, launch-inclusive times (for a
split plan: both kernels), the pools rotate over sets whose FP8 bytes alone reach 640 MiB (past the 256 MiB Infinity Cache), one pair of device
events around back-to-back calls after a warm-up, every timed window >= 0.1 s, best of 3 alternating rounds. ratio = fp16 time / FP8 time; the
byte ratio of the K / V stream is 2.
  python fa_paged_fp8_attn_bench.py [--quick] [--skip multi|prefill] [--fp16-lib OTHER.so]
--quick: D = 128 at (B, context) = (8, 4096), (8, 32768), (64, 16384) and D = 64 at (64, 16384) for the multi-token table; the prefill table is
the same six shapes either way.
--fp16-lib OTHER.so: a third table -- the two fp16 entries cln_fa2_decode_paged_multi and cln_fa2_prefill_paged of this build against the same
C entries of another build of their compile units (say the parent commit's: the two .hip files compiled with the flags of _build.py and linked
into a shared object), both called through ctypes with the same arguments, alternating in one process: what a change to the shared kernel
bodies did to the fp16 entries."""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fa_decode_paged_fp8_bench as fb  # noqa: E402  (best_of, pool_pair, code_values: one method for the three FP8 tables)

HKV, PAGE, F8 = fb.HKV, 16, fb.F8
GS, TS = (1, 4, 8), (1, 4, 8)
FULL = [(D, N, B) for D in (64, 128) for N in (4096, 16384, 32768) for B in (8, 64)]
QUICK = [(128, 4096, 8), (128, 32768, 8), (128, 16384, 64), (64, 16384, 64)]
PREFILL = [(1, 64, 16384), (1, 512, 4096), (1, 2048, 0), (4, 64, 4096), (4, 512, 4096), (4, 2048, 16384)]  # (B, T, context): INTEGRATION 13


def make_sets(B, N, D, scales, lut, gen):
    mp = N // PAGE
    per8 = 2 * B * HKV * N * D
    nsets = max(1, min(fb.MAX_SETS, -(-fb.ROTATE_BYTES // per8)))
    sets = []
    for _ in range(nsets):
        bt = torch.randperm(B * mp, generator=gen, device="cuda").view(mp, B).t().contiguous().to(torch.int32)
        sets.append(fb.pool_pair(B * mp, PAGE, D, scales, lut, gen) + (bt,))
    return sets, per8


def multi_table(shapes):
    print("multi-token paged decode attention, FP8 cache against fp16 cache, Hkv = %d, page %d: us per call (launch-inclusive); GB/s = 2 len B Hkv D "
          "(1 | 2) bytes / time; ratio = fp16 us / fp8 us (byte ratio 2); at T = 1 also fa2_decode_paged_fp8 (VALU) on the same pool and "
          "valu/mfma = its us / the multi-token FP8 us" % (HKV, PAGE))
    print("%-18s %-2s %-2s %-14s %9s %9s %9s %9s %7s %10s %9s" % ("(B, len, D)", "G", "T", "plan", "fp8 us", "GB/s", "fp16 us", "GB/s", "ratio",
                                                                   "valu8 us", "valu/mfma"))
    gen = torch.Generator(device="cuda").manual_seed(0)
    lut = fb.code_values()
    scales = torch.tensor([0.5 * (1.0 + 0.25 * h) for h in range(HKV)], device="cuda")
    for (D, N, B) in shapes:
        mp = N // PAGE
        sl = torch.full((B,), N, dtype=torch.int32, device="cuda")
        sets, per8 = make_sets(B, N, D, scales, lut, gen)
        nsets = len(sets)
        for G in GS:
            Hq = HKV * G
            for T in TS:
                q = torch.randn(B, T, Hq, D, dtype=torch.half, device="cuda", generator=gen)
                o8, o16 = torch.empty_like(q), torch.empty_like(q)
                p8, p16 = pkg.fa2_decode_paged_multi_fp8_plan(B, T, Hq, HKV, mp, PAGE, D), pkg.fa2_decode_paged_multi_plan(B, T, Hq, HKV, mp, PAGE, D)
                assert p8 == p16
                ws8, ws16 = (torch.empty(max(p8[2], 16), dtype=torch.uint8, device="cuda") for _ in range(2))
                i, j, k = [0], [0], [0]

                def fp8():
                    k8, v8, _, _, bt = sets[i[0] % nsets]
                    i[0] += 1
                    pkg.fa2_decode_paged_multi_fp8(q, k8, v8, bt, sl, scales, scales, o8, None, ws8)

                def fp16():
                    _, _, k16, v16, bt = sets[j[0] % nsets]
                    j[0] += 1
                    pkg.fa2_decode_paged_multi(q, k16, v16, bt, sl, o16, None, ws16)

                calls = {"fp8": fp8, "fp16": fp16}
                if T == 1:
                    q1, o1 = q.view(B, Hq, D), torch.empty(B, Hq, D, dtype=torch.half, device="cuda")
                    ws1 = torch.empty(max(pkg.fa2_decode_paged_fp8_plan(B, Hq, HKV, mp, PAGE, D)[2], 16), dtype=torch.uint8, device="cuda")

                    def valu8():
                        k8, v8, _, _, bt = sets[k[0] % nsets]
                        k[0] += 1
                        pkg.fa2_decode_paged_fp8(q1, k8, v8, bt, sl, scales, scales, o1, None, ws1)

                    calls["valu8"] = valu8
                best = fb.best_of(calls)
                tail = "%10.2f %9.3f" % (best["valu8"] * 1e3, best["valu8"] / best["fp8"]) if T == 1 else "%10s %9s" % ("-", "-")
                print("%-18s %-2d %-2d %-14s %9.2f %9.1f %9.2f %9.1f %7.3f %s" % (
                    str((B, N, D)), G, T, "S=%d C=%d" % p8[:2], best["fp8"] * 1e3, per8 / best["fp8"] * 1e-6, best["fp16"] * 1e3,
                    2 * per8 / best["fp16"] * 1e-6, best["fp16"] / best["fp8"], tail), flush=True)
        del sets
        torch.cuda.empty_cache()


def prefill_table():
    G, D = 4, 128
    Hq = HKV * G
    print("paged prefill attention, FP8 cache against fp16 cache, Hq / Hkv = %d / %d, D = %d, page %d: us per call (launch-inclusive); TF/s = "
          "4 D Hq B (T ctx + T (T + 1) / 2) / time; ratio = fp16 us / fp8 us" % (Hq, HKV, D, PAGE))
    print("%-18s %9s %8s %9s %8s %7s" % ("(B, T, context)", "fp8 us", "TF/s", "fp16 us", "TF/s", "ratio"))
    gen = torch.Generator(device="cuda").manual_seed(2)
    lut = fb.code_values()
    scales = torch.tensor([0.5 * (1.0 + 0.25 * h) for h in range(HKV)], device="cuda")
    for (B, T, ctx) in PREFILL:
        N = -(-(ctx + T) // PAGE) * PAGE
        sl = torch.full((B,), ctx + T, dtype=torch.int32, device="cuda")
        sets, _ = make_sets(B, N, D, scales, lut, gen)
        nsets = len(sets)
        q = torch.randn(B, T, Hq, D, dtype=torch.half, device="cuda", generator=gen)
        o8, o16 = torch.empty_like(q), torch.empty_like(q)
        i, j = [0], [0]

        def fp8():
            k8, v8, _, _, bt = sets[i[0] % nsets]
            i[0] += 1
            pkg.fa2_prefill_paged_fp8(q, k8, v8, bt, sl, scales, scales, o8)

        def fp16():
            _, _, k16, v16, bt = sets[j[0] % nsets]
            j[0] += 1
            pkg.fa2_prefill_paged(q, k16, v16, bt, sl, o16)

        best = fb.best_of({"fp8": fp8, "fp16": fp16})
        flops = 4.0 * D * Hq * B * (T * ctx + T * (T + 1) / 2)
        print("%-18s %9.2f %8.1f %9.2f %8.1f %7.3f" % (str((B, T, ctx)), best["fp8"] * 1e3, flops / best["fp8"] * 1e-9, best["fp16"] * 1e3,
                                                        flops / best["fp16"] * 1e-9, best["fp16"] / best["fp8"]), flush=True)
        del sets
        torch.cuda.empty_cache()


def fp16_against(other_path):
    """cln_fa2_decode_paged_multi and cln_fa2_prefill_paged: this build ('this') against the library at other_path ('other'), fp16 pools rotating
    over >= 640 MiB, the same pointers and arguments for both."""
    from cuda_learn_notes_amd import _loader, host
    libs = {"this": ctypes.CDLL(_loader.so_path("libcln_amd.so")), "other": ctypes.CDLL(os.path.abspath(other_path))}
    vp, ci, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    for lib in libs.values():
        lib.cln_fa2_decode_paged_multi.argtypes, lib.cln_fa2_decode_paged_multi.restype = [vp] * 8 + [ll] + [ci] * 8 + [vp], ci
        lib.cln_fa2_prefill_paged.argtypes, lib.cln_fa2_prefill_paged.restype = [vp] * 7 + [ci] * 8 + [vp], ci
    gen = torch.Generator(device="cuda").manual_seed(3)

    def fp16_sets(B, N, D):
        mp = N // PAGE
        per = 4 * B * HKV * N * D
        nsets = max(1, min(fb.MAX_SETS, -(-fb.ROTATE_BYTES // per)))
        out = []
        for _ in range(nsets):
            bt = torch.randperm(B * mp, generator=gen, device="cuda").view(mp, B).t().contiguous().to(torch.int32)
            k, v = (torch.randn(B * mp, HKV, PAGE, D, dtype=torch.half, device="cuda", generator=gen) for _ in range(2))
            out.append((k, v, bt))
        return out

    def pair(make_call):
        calls = {}
        for name, lib in libs.items():
            calls[name] = make_call(lib)
        for f in calls.values():  # every call returns 0 before anything is timed
            f()
        torch.cuda.synchronize()
        return fb.best_of(calls)

    print("fp16 entries, this build against %s: us per call (launch-inclusive), ratio = other us / this us (> 1: this build is faster)"
          % os.path.basename(other_path))
    print("%-26s %-18s %-2s %-2s %10s %10s %7s" % ("entry", "(B, len, D)", "G", "T", "this us", "other us", "ratio"))
    for (D, N, B) in [(128, 4096, 8), (128, 16384, 64), (64, 4096, 8), (64, 16384, 64)]:
        mp = N // PAGE
        sl = torch.full((B,), N, dtype=torch.int32, device="cuda")
        sets = fp16_sets(B, N, D)
        for G in GS:
            Hq = HKV * G
            for T in (1, 4, 8):
                q = torch.randn(B, T, Hq, D, dtype=torch.half, device="cuda", generator=gen)
                o = torch.empty_like(q)
                need = pkg.fa2_decode_paged_multi_plan(B, T, Hq, HKV, mp, PAGE, D)[2]
                ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")

                def make_call(lib):
                    i = [0]

                    def call():
                        k, v, bt = sets[i[0] % len(sets)]
                        i[0] += 1
                        rc = lib.cln_fa2_decode_paged_multi(q.data_ptr(), k.data_ptr(), v.data_ptr(), bt.data_ptr(), sl.data_ptr(), o.data_ptr(), None,
                                                            ws.data_ptr(), ws.numel(), B, T, Hq, HKV, B * mp, mp, PAGE, D, host._stream())
                        assert rc == 0, rc
                    return call

                best = pair(make_call)
                print("%-26s %-18s %-2d %-2d %10.2f %10.2f %7.3f" % ("fa2_decode_paged_multi", str((B, N, D)), G, T, best["this"] * 1e3,
                                                                    best["other"] * 1e3, best["other"] / best["this"]), flush=True)
        del sets
        torch.cuda.empty_cache()
    G, D = 4, 128
    Hq = HKV * G
    for (B, T, ctx) in PREFILL:
        N = -(-(ctx + T) // PAGE) * PAGE
        mp = N // PAGE
        sl = torch.full((B,), ctx + T, dtype=torch.int32, device="cuda")
        sets = fp16_sets(B, N, D)
        q = torch.randn(B, T, Hq, D, dtype=torch.half, device="cuda", generator=gen)
        o = torch.empty_like(q)

        def make_call(lib):
            i = [0]

            def call():
                k, v, bt = sets[i[0] % len(sets)]
                i[0] += 1
                rc = lib.cln_fa2_prefill_paged(q.data_ptr(), k.data_ptr(), v.data_ptr(), bt.data_ptr(), sl.data_ptr(), o.data_ptr(), None, B, T, Hq,
                                               HKV, B * mp, mp, PAGE, D, host._stream())
                assert rc == 0, rc
            return call

        best = pair(make_call)
        print("%-26s %-18s %-2d %-2s %10.2f %10.2f %7.3f" % ("fa2_prefill_paged", str((B, T, ctx)) + " ctx", G, "-", best["this"] * 1e3,
                                                            best["other"] * 1e3, best["other"] / best["this"]), flush=True)
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    skip = [a for a in sys.argv[sys.argv.index("--skip") + 1:] if not a.startswith("--") and not a.endswith(".so")] if "--skip" in sys.argv else []
    if "multi" not in skip:
        multi_table(QUICK if "--quick" in sys.argv else FULL)
    if "prefill" not in skip:
        prefill_table()
    if "--fp16-lib" in sys.argv:
        fp16_against(sys.argv[sys.argv.index("--fp16-lib") + 1])
