"""Helper of the tests of the block-scaled FP8 GEMM and its quantiser (tests/test_gpu_gemm_fp8_block128.py,
tests/test_gemm_fp8_block128_surface.py). A plain module: nothing here is collected.

    out[m, n] = bf16( sum_kb sa[m, kb] sb[n // 128, kb] sum_{k in kb} a[m, k] b[n, k] )

a e4m3fn [M,K] with sa fp32 [M,K/128]; b e4m3fn [N,K] with sb fp32 [ceil(N/128),K/128]. ref() is that sum in fp64 together with
S = sum_kb sa sb sum_k |a| |b|; the bound of the GPU test is 2^-8 |ref| + (128 + 2 K / 128) 2^-23 S: one bf16 rounding, any summation order of
128 products (2^-23 each so that a truncating adder is covered), the fp32 scale-and-add chain. Cases are made on the CPU, once per process,
and never modified."""
import functools

import torch

import fp8_kv_reference as fk

BF, F8, F32 = torch.bfloat16, fk.F8, torch.float32
BLK = 128
SHAPES = ((1, 8, 128), (17, 264, 384), (64, 128, 256), (65, 136, 256), (129, 392, 1024), (300, 576, 512))


def quant_a(x, pow2=False):
    """(codes e4m3fn [M,K], scales fp32 [M,K/128]) of bf16 x [M,K] in the kernel's fp32 operations: a = max(amax, 1e-4), scale = a / 448, with
    pow2 the smallest power of two >= scale on the bits, codes = e4m3fn rne of clamp(x (1 / scale), +-448)."""
    M, K = x.shape
    xb = x.float().view(M, K // BLK, BLK)
    s = xb.abs().amax(dim=-1).clamp_min(torch.tensor(1e-4, dtype=F32)) / torch.tensor(448.0, dtype=F32)
    if pow2:
        b = s.view(torch.int32)
        s = torch.where((b & 0x007FFFFF) != 0, (b & 0x7F800000) + 0x00800000, b).view(F32)
    return fk.quantize(xb, s[:, :, None]).view(M, K), s.contiguous()


def quant_b(w):
    """(codes e4m3fn [N,K], scales fp32 [ceil(N/128),K/128]) of a float weight [N,K]: 128 x 128 blocks (the last block of N may be partial),
    scale = amax / 448."""
    N, K = w.shape
    nb = -(-N // BLK)
    wp = torch.zeros(nb * BLK, K, dtype=F32)
    wp[:N] = w.float()
    blocks = wp.view(nb, BLK, K // BLK, BLK)
    s = blocks.abs().amax(dim=(1, 3)) / torch.tensor(448.0, dtype=F32)
    codes = fk.quantize(blocks, s[:, None, :, None]).view(nb * BLK, K)[:N].contiguous()
    return codes, s.contiguous()


def ref(a, sa, b, sb):
    """(ref, S) in fp64, both [M,N]."""
    (M, K), N = a.shape, b.shape[0]
    kb = K // BLK
    ad, bd = a.double().view(M, kb, BLK), b.double().view(N, kb, BLK)
    sbn = sb.double().repeat_interleave(BLK, dim=0)[:N]  # [N, kb]
    out, S = torch.zeros(M, N, dtype=torch.float64), torch.zeros(M, N, dtype=torch.float64)
    for i in range(kb):
        s = sa[:, i].double()[:, None] * sbn[:, i][None, :]
        out += s * (ad[:, i] @ bd[:, i].T)
        S += s * (ad[:, i].abs() @ bd[:, i].abs().T)
    return out, S


def bound(r, S, K):
    return 2.0 ** -8 * r.abs() + (128 + 2 * K // BLK) * 2.0 ** -23 * S


@functools.lru_cache(maxsize=None)
def gaussian(M, N, K):
    """x bf16 [M,K] randn, its quantisation, 0.05 randn weights quantised, and the fp64 reference: every scale distinct, none a power of two."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    x = torch.randn(M, K, generator=g).to(BF)
    a, sa = quant_a(x)
    b, sb = quant_b(0.05 * torch.randn(N, K, generator=g))
    return x, a, sa, b, sb, ref(a, sa, b, sb)


@functools.lru_cache(maxsize=None)
def exact(M, N, K):
    """Integer codes in -4 ... 4 and scales 2^-2 ... 2^2: every partial sum is a multiple of 2^-4 below 2^24, so fp32 is exact in any order and
    the answer is ref rounded once to bf16."""
    g = torch.Generator().manual_seed(7 * M + 11 * N + 13 * K)
    kb, nb = K // BLK, -(-N // BLK)
    a = torch.randint(-4, 5, (M, K), generator=g).float().to(F8)
    b = torch.randint(-4, 5, (N, K), generator=g).float().to(F8)
    sa = 2.0 ** torch.randint(-2, 3, (M, kb), generator=g).float()
    sb = 2.0 ** torch.randint(-2, 3, (nb, kb), generator=g).float()
    return a, sa, b, sb, ref(a, sa, b, sb)[0].float().to(BF)


def one_hot(side, step, off):
    """(16, 16, 128), unit scales: row i of the one-hot operand is 1 at k_i = (step i + off) % 128 and 0 elsewhere, the other operand is dense
    with d[r, k] = (7 k + 3 r) % 31 - 15 (integers, exact in e4m3, neighbours in k and r differ): out[m, n] is the single byte d[., k_i]. A
    lane group that takes another K slice, a row in another lane or a byte order that differs between the operands moves the answer."""
    k = (step * torch.arange(16) + off) % BLK
    hot = torch.zeros(16, BLK)
    hot[torch.arange(16), k] = 1.0
    dense = ((7 * torch.arange(BLK)[None, :] + 3 * torch.arange(16)[:, None]) % 31 - 15).float()
    a, b = (hot, dense) if side == "a" else (dense, hot)
    want = dense[:, k].T if side == "a" else dense[:, k]  # [m, n]
    return a.to(F8), torch.ones(16, 1), b.to(F8), torch.ones(1, 1), want.to(BF)
