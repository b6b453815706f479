"""GPU timing of the paged KV-cache append with fused RoPE (cuda_learn_notes_amd.kv_append_paged, cln_kv_append_paged) against what a caller
writes without it -- the torch composition: positions, page and row indices computed on the device, q and k rotated with torch ops in fp32, two
index_put_ -- and against torch.Tensor.copy_ of the bytes the entry writes (the K, V and q rows), the floor of any kernel that moves them.
All three run in the same process on the same pool (pages placed by a random permutation, Hq / Hkv = 32 / 8, D = 128, page 16, CTX tokens of
context in front of the new ones). Times are launch-inclusive: one pair of device events around back-to-back calls after a warm-up, every timed
window >= 0.1 s, best of 3 alternating rounds (fa_decode_paged_bench.timed). The new rows and q rotate over SETS input sets with different
lengths, so consecutive calls write different rows; they stay cache-resident, as they are behind the projection GEMM that produces them.
The composition is given every token live (it does no clamping) and no lengths on the host.
  python kv_append_paged_bench.py [--rows decode verify prefill] [--rope none half interleaved]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as entry  # noqa: E402

pkg = entry.load_package()
from fa_decode_paged_bench import best_of  # noqa: E402

HQ, HKV, D, PAGE, CTX, SETS = 32, 8, 128, 16, 2048, 4
ROWS = {"decode": [(8, 1), (64, 1), (256, 1)], "verify": [(8, 8), (64, 8), (256, 8)], "prefill": [(4, 512)]}  # (B, T)
ROPES = ("none", "half", "interleaved")


def torch_append(k_new, v_new, kp, vp, bt, sl, q, q_out, table, rope, ar, heads):
    """The composition on the device: nothing is read on the host. Every token is taken as live."""
    T = k_new.shape[1]
    pos = (sl[:, None] - T + ar[None, :]).long()  # [B,T]
    k = k_new
    if rope != "none":
        cs = table[pos]  # [B,T,D]
        c, s = cs[:, :, None, :D // 2], cs[:, :, None, D // 2:]

        def rot(x):
            x = x.float()
            x1, x2 = (x[..., :D // 2], x[..., D // 2:]) if rope == "half" else (x[..., 0::2], x[..., 1::2])
            a, b = x1 * c - x2 * s, x1 * s + x2 * c
            return (torch.cat((a, b), dim=-1) if rope == "half" else torch.stack((a, b), dim=-1).flatten(-2)).half()

        k = rot(k_new)
        q_out.copy_(rot(q))
    pg = bt.gather(1, pos // PAGE).long()
    idx = (pg[:, :, None], heads[None, None, :], (pos % PAGE)[:, :, None])
    kp.index_put_(idx, k)
    vp.index_put_(idx, v_new)


def table(rows, ropes):
    print("paged KV append, Hq / Hkv = %d / %d, D = %d, page %d, %d tokens of context: us per call (launch-inclusive); 'torch' = the composition of "
          "torch ops (rotate, indices on the device, two index_put_); 'copy_' = torch.Tensor.copy_ of the bytes the entry writes; x = torch / entry"
          % (HQ, HKV, D, PAGE, CTX))
    print("%-8s %-4s %-4s %-12s %10s %10s %10s %8s %10s" % ("row", "B", "T", "rope", "bytes", "entry us", "torch us", "x", "copy_ us"))
    gen = torch.Generator(device="cuda").manual_seed(0)
    rope_table = pkg.kv_append_rope_table(CTX + 1024, D, device="cuda")
    heads = torch.arange(HKV, device="cuda")
    for name in rows:
        for (B, T) in ROWS[name]:
            mp = -(-(CTX + T + SETS) // PAGE)
            P = B * mp
            kp, vp = (torch.randn(P, HKV, PAGE, D, dtype=torch.half, device="cuda", generator=gen) for _ in range(2))
            bt = torch.randperm(P, generator=gen, device="cuda").view(mp, B).t().contiguous().to(torch.int32)
            sets = [(torch.randn(B, T, HKV, D, dtype=torch.half, device="cuda", generator=gen),
                     torch.randn(B, T, HKV, D, dtype=torch.half, device="cuda", generator=gen),
                     torch.randn(B, T, HQ, D, dtype=torch.half, device="cuda", generator=gen),
                     torch.full((B,), CTX + T + i, dtype=torch.int32, device="cuda")) for i in range(SETS)]
            q_out = torch.empty(B, T, HQ, D, dtype=torch.half, device="cuda")
            ar = torch.arange(T, device="cuda", dtype=torch.int32)
            for rope in ropes:
                nbytes = B * T * (2 * HKV + (HQ if rope != "none" else 0)) * D * 2
                src, dst = (torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(2))
                i, j = [0], [0]

                def ours():
                    kn, vn, q, sl = sets[i[0] % SETS]
                    i[0] += 1
                    if rope == "none":
                        pkg.kv_append_paged(kn, vn, kp, vp, bt, sl)
                    else:
                        pkg.kv_append_paged(kn, vn, kp, vp, bt, sl, q, q_out, rope_table, rope)

                def composed():
                    kn, vn, q, sl = sets[j[0] % SETS]
                    j[0] += 1
                    torch_append(kn, vn, kp, vp, bt, sl, q, q_out, rope_table, rope, ar, heads)

                best = best_of({"entry": ours, "torch": composed, "copy": lambda: dst.copy_(src)})
                print("%-8s %-4d %-4d %-12s %10d %10.2f %10.2f %8.2f %10.2f" % (name, B, T, rope, nbytes, best["entry"] * 1e3, best["torch"] * 1e3,
                                                                             best["torch"] / best["entry"], best["copy"] * 1e3), flush=True)
            del kp, vp, sets
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", nargs="+", default=list(ROWS), choices=list(ROWS))
    ap.add_argument("--rope", nargs="+", default=list(ROPES), choices=list(ROPES))
    a = ap.parse_args()
    table(a.rows, a.rope)
