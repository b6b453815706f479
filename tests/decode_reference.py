"""References for the decode attention tests (tests/test_fa2_decode_surface.py proves them, tests/test_gpu_fa2_decode.py uses them): the fp64
single-query attention over a KV cache with per-sequence lengths clamped as the kernels clamp them, a Python mirror of the split plan of
csrc/flash_attn_decode.hip, and the tolerance rule of the plain attention names. A plain module: nothing here is collected."""
import torch

TOL_AMPLIFIED_KEYS = 6e-3

# the constants of csrc/flash_attn_decode.hip / flash_attn_decode.cuh
TARGET_WORKGROUPS = 1024
MIN_CHUNK = 256
MAX_SPLITS = 64


def key_step(D):
    """Keys per workgroup step: 4 waves x 4 loads x (64 lanes / (D / 8) lanes per row)."""
    return 4 * 4 * (64 * 8 // D)


def plan(B, H, Nmax, D):
    """(splits, chunk, workspace_bytes) as cln_fa2_decode_plan computes them."""
    step, bh = key_step(D), B * H
    want = 1
    if bh < TARGET_WORKGROUPS and Nmax > MIN_CHUNK:
        want = min(-(-TARGET_WORKGROUPS // bh), Nmax // MIN_CHUNK, MAX_SPLITS)
    chunk = -(-(-(-Nmax // want)) // step) * step
    splits = -(-Nmax // chunk)
    return splits, chunk, workspace_bytes(B, H, splits, D)


def workspace_bytes(B, H, splits, D):
    """fp32 O partials [B H][S][D] and (m, l) pairs [B H][S][2]; nothing for one split."""
    return B * H * splits * (D + 2) * 4 if splits > 1 else 0


def ref_decode(q, k, v, lens):
    """fp64 (O [B,H,D], LSE [B,H]) of O[b,h] = sum_{j < len_b} softmax_j(q . K_j / sqrt(D)) V_j with len_b = clamp(lens[b], 0, Nmax);
    len_b = 0 gives O = 0 and LSE = -inf. q: [B,H,D]; k, v: [B,H,Nmax,D]; lens: B integers."""
    B, H, Nmax, D = k.shape
    qd, kd, vd = q.double().cpu(), k.double().cpu(), v.double().cpu()
    O = torch.zeros(B, H, D, dtype=torch.float64)
    L = torch.full((B, H), float("-inf"), dtype=torch.float64)
    for b in range(B):
        n = min(max(int(lens[b]), 0), Nmax)
        if n == 0:
            continue
        s = torch.einsum("hd,hjd->hj", qd[b], kd[b, :, :n]) / D ** 0.5
        L[b] = torch.logsumexp(s, dim=-1)
        O[b] = torch.einsum("hj,hjd->hd", torch.exp(s - L[b][:, None]), vd[b, :, :n])
    return O, L


def fa_tol(ref):
    """The scale rule of the plain attention names (tests/fa_reference.py): 2^-9 max|O_ref| + 4e-4, never more than 6e-3."""
    return min(2.0 ** -9 * float(ref.abs().max()) + 4e-4, TOL_AMPLIFIED_KEYS)


def lse_tol(ref):
    """The first clause of check_lse (tests/fa_reference.py): 2^-10 max(1, max|LSE_ref|) over the finite entries."""
    fin = ref[torch.isfinite(ref)]
    return 2.0 ** -10 * max(1.0, float(fin.abs().max()) if fin.numel() else 0.0)
