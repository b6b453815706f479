"""Helper of the tests of the fused gate/up + SiLU-mul + quantise grouped FP8 GEMM (tests/test_gpu_gemm_fp8_block128_grouped_swiglu.py; DESIGN
4.4.30). A plain module: nothing here is collected. Built on gemm_fp8_block128_reference (gr) and fp8_kv_reference (fk).

For one expert with b [2I,K] (rows 0 ... I-1 gate, I ... 2I-1 up) and sb [2I/128,K/128]:  G, U = gr.ref on the two halves (fp64, with
their S = sum |terms|), h_ref = G / (1 + exp(-G)) * U in fp64. The kernel keeps G and U in fp32 and rounds nothing to bf16, so

    eG = (128 + 2 K / 128) 2^-23 S_G, eU likewise                    gr.bound without its bf16 term
    E_h = 1.1 eG (|U| + eU) + |silu(G)| eU + 2^-19 |h_ref|           |silu'| <= 1.1; the last term: the approximate exp and reciprocal and
                                                                     the two products, for |G| up to a few units
    bound = 2^-4 |h_ref| + 2^-10 h_scale + 2 E_h                     fk.bound's shape: half an e4m3 ulp of a normal code, half a subnormal
                                                                     step, and an fp32 error that carries a value across a rounding
                                                                     boundary adds no more than itself (hence 2 E_h)

on |code * h_scale - h_ref| with code and h_scale as the kernel returned them, dequantised in fp64; and the scale itself obeys
|448 h_scale - max(amax_block |h_ref|, 1e-4)| <= max_block E_h + 2^-22 amax (one fp32 division). Cases are made on the CPU, once per process,
and never modified."""
import functools

import torch

import gemm_fp8_block128_reference as gr

BLK = gr.BLK


def ref(a, sa, b, sb, K):
    """(h_ref, E_h) in fp64, both [M,I], of one expert."""
    I = b.shape[0] // 2
    (G, SG), (U, SU) = gr.ref(a, sa, b[:I], sb[:I // BLK]), gr.ref(a, sa, b[I:], sb[I // BLK:])
    c = (128 + 2 * K // BLK) * 2.0 ** -23
    eG, eU, silu = c * SG, c * SU, G / (1.0 + torch.exp(-G))
    h = silu * U
    return h, 1.1 * eG * (U.abs() + eU) + silu.abs() * eU + 2.0 ** -19 * h.abs()


def bound(h, Eh, h_scale):
    """h_scale [M,I/128] as the kernel returned it."""
    return 2.0 ** -4 * h.abs() + 2.0 ** -10 * h_scale.double().repeat_interleave(BLK, dim=1) + 2.0 * Eh


def scale_slack(h, Eh, h_scale):
    """(|448 h_scale - max(amax, 1e-4)|, its allowance), both [M,I/128]."""
    M, I = h.shape
    amax = h.abs().view(M, I // BLK, BLK).amax(dim=-1)
    return (448.0 * h_scale.double() - amax.clamp_min(1e-4)).abs(), Eh.view(M, I // BLK, BLK).amax(dim=-1) + 2.0 ** -22 * amax


@functools.lru_cache(maxsize=None)
def exact(M, I, K):
    """a, sa, b [2I,K], sb of one expert and hf fp32 [M,I]: activation and gate codes are integers in 1 ... 4 with scales 2^0 ... 2^2, so
    G >= K >= 128 is an integer below 2^24 (exact in fp32 in any order) and SiLU returns it; up codes are integers in -4 ... 4 with scales
    2^-2 ... 2^2, so U is exact; hf = fl32(G U) is one IEEE product."""
    g = torch.Generator().manual_seed(7 * M + 11 * I + 13 * K)
    kb, nb = K // BLK, I // BLK
    a = torch.randint(1, 5, (M, K), generator=g).float().to(gr.F8)
    b = torch.cat([torch.randint(1, 5, (I, K), generator=g), torch.randint(-4, 5, (I, K), generator=g)]).float().to(gr.F8)
    sa = 2.0 ** torch.randint(0, 3, (M, kb), generator=g).float()
    sb = 2.0 ** torch.cat([torch.randint(0, 3, (nb, kb), generator=g), torch.randint(-2, 3, (nb, kb), generator=g)]).float()
    G, U = gr.ref(a, sa, b[:I], sb[:nb])[0], gr.ref(a, sa, b[I:], sb[nb:])[0]
    return a, sa, b, sb, G.float() * U.float()
