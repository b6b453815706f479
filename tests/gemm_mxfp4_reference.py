"""Helper of the tests of the MXFP4-weight GEMMs and their MXFP8 quantiser (tests/test_gpu_gemm_mxfp4.py, tests/test_gemm_mxfp4_surface.py;
DESIGN 4.4.32). A plain module: nothing here is collected.

    out[m, n] = bf16( bias[n] + sum_kb 2^(sa[m, kb] - 127) 2^(sb[n, kb] - 127) sum_{k in kb} e4m3(a[m, k]) e2m1(b[n, k]) ),  kb over K / 32

a e4m3fn [M,K] with sa e8m0 [M,K/32]; b uint8 [N,K/2] (element 2 i in the low nibble of byte i) with sb uint8 [N,K/32]. ref() is that sum in
fp64 together with S = sum scales |a| |b|; the bound of the GPU test is 2^-8 |ref| + (128 + K / 128) 2^-23 S: one bf16 rounding, any
summation order of 128 products (2^-23 each so that a truncating adder is covered), the chain through the C operand. Cases are made on the
CPU, once per process, and never modified."""
import functools

import torch

BF, F8, E8, F32, F64 = torch.bfloat16, torch.float8_e4m3fn, torch.float8_e8m0fnu, torch.float32, torch.float64
MX = 32
E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], dtype=F64)  # by code
SHAPES = ((1, 8, 32), (17, 264, 96), (64, 128, 160), (65, 136, 416), (129, 392, 416))


def e8m0(s):
    """2^(byte - 127) in fp64 of e8m0 bytes (uint8 or float8_e8m0fnu)."""
    return torch.pow(torch.tensor(2.0, dtype=F64), s.view(torch.uint8).double() - 127.0)


def pack(codes):
    """uint8 [N,K/2] of e2m1 codes uint8 [N,K]: element 2 i in the low nibble of byte i."""
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def unpack(b):
    """fp64 [N,K] values of packed e2m1 bytes [N,K/2]."""
    b = b.view(torch.uint8)
    return E2M1[torch.stack((b & 15, b >> 4), dim=-1).flatten(-2).long()]


def quant_a(x):
    """(codes e4m3fn [M,K], scale bytes e8m0 [M,K/32]) of bf16 x in the kernel's integer and fp32 operations: E = the exponent field of
    fp32(amax), byte = clamp(E - 8, 0, 254), code = e4m3fn rne of clamp(x 2^(127 - byte), +-448)."""
    M, K = x.shape
    xb = x.float().view(M, K // MX, MX)
    sc = (((xb.abs().amax(dim=-1).view(torch.int32) >> 23) & 0xFF) - 8).clamp(0, 254)
    inv = torch.where(sc < 254, (254 - sc) << 23, torch.full_like(sc, 0x00400000)).view(F32)
    codes = (xb * inv[:, :, None]).clamp(-448.0, 448.0).to(F8).view(M, K)
    return codes, sc.to(torch.uint8).view(E8).contiguous()


def quant_b(w):
    """(packed e2m1 uint8 [N,K/2], scale bytes uint8 [N,K/32]) of a float weight: per 32 elements byte = floor(log2 amax) - 2 + 127, the
    nearest e2m1 value of w 2^(127 - byte) (saturating at 6)."""
    N, K = w.shape
    wb = w.double().view(N, K // MX, MX)
    sc = (torch.floor(torch.log2(wb.abs().amax(dim=-1).clamp_min(2.0 ** -100))) - 2 + 127).clamp(0, 254)
    y = wb * torch.pow(torch.tensor(2.0, dtype=F64), 127 - sc)[:, :, None]
    codes = (y.abs()[..., None] - E2M1[:8]).abs().argmin(dim=-1) + 8 * (y < 0)
    return pack(codes.view(N, K).to(torch.uint8)), sc.to(torch.uint8).contiguous()


def ref(a, sa, b, sb, bias=None):
    """(ref, S) in fp64, both [M,N]; the scales are powers of two, so applying them per element is the definition's sum exactly."""
    A = a.double() * e8m0(sa).repeat_interleave(MX, dim=1)
    B = unpack(b) * e8m0(sb).repeat_interleave(MX, dim=1)
    out = A @ B.T
    return (out if bias is None else out + bias.double()[None, :]), A.abs() @ B.abs().T


def bound(r, S, K):
    return 2.0 ** -8 * r.abs() + (128 + K / 128) * 2.0 ** -23 * S


@functools.lru_cache(maxsize=None)
def gaussian(M, N, K, seed=0):
    """x bf16 [M,K] randn, its MXFP8 quantisation, 0.05 randn weights in MXFP4, a bf16 bias, and the fp64 reference WITHOUT the bias."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + seed)
    x = torch.randn(M, K, generator=g).to(BF)
    a, sa = quant_a(x)
    b, sb = quant_b(0.05 * torch.randn(N, K, generator=g))
    return x, a, sa, b, sb, torch.randn(N, generator=g).to(BF), ref(a, sa, b, sb)


@functools.lru_cache(maxsize=None)
def exact(M, N, K):
    """Integer a in -4 ... 4, every e2m1 value in b, scales 2^-2 ... 2^2 drawn per block, an integer bias: every partial sum is a multiple of
    2^-5 below 2^24, so fp32 is exact in any order and the answer is ref rounded once to bf16."""
    g = torch.Generator().manual_seed(7 * M + 11 * N + 13 * K)
    a = torch.randint(-4, 5, (M, K), generator=g).float().to(F8)
    b = pack(torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8))
    sa = torch.randint(125, 130, (M, K // MX), generator=g, dtype=torch.uint8).view(E8)
    sb = torch.randint(125, 130, (N, K // MX), generator=g, dtype=torch.uint8)
    bias = torch.randint(-8, 9, (N,), generator=g).to(BF)
    return a, sa, b, sb, bias, ref(a, sa, b, sb, bias)[0].to(BF)


def one_hot(side, step, off):
    """(16, 16, 128): row i of the one-hot operand is 1 at k_i = (step i + off) % 128, the other operand is dense and differs between
    neighbours in k and in the row (b: the seven non-zero e2m1 magnitudes with alternating signs; a: integers), and every (row, block) scale
    is a distinct power of two (sa 2^(4 m + kb - 32), sb 2^(2 (4 n + kb) - 63)): out[m, n] is one element times one scale of each side,
    exact in bf16. A swapped nibble, lane group, row, scale byte or sa / sb moves the answer."""
    r, k = torch.arange(16)[:, None], torch.arange(128)[None, :]
    ki = (step * torch.arange(16) + off) % 128
    if side == "a":
        a = torch.zeros(16, 128)
        a[torch.arange(16), ki] = 1.0
        codes = 1 + (3 * k + 5 * r) % 7 + 8 * ((k + r) & 1)
    else:
        a = ((7 * k + 3 * r) % 31 - 15).float()
        codes = torch.zeros(16, 128, dtype=torch.int64)
        codes[torch.arange(16), ki] = 2
    b = pack(codes.to(torch.uint8))
    kb = torch.arange(4)[None, :]
    sa = (127 + 4 * r + kb - 32).to(torch.uint8).view(E8)
    sb = (127 + 2 * (4 * r + kb) - 63).to(torch.uint8)
    return a.to(F8), sa, b, sb, ref(a.to(F8), sa, b, sb)[0].to(BF)


def quant_rows(M, K):
    """bf16 x [M,K] for the quantiser: scaled randn rows, then row 0 = (an all-zero block, a block with amax exactly 2^6, a block whose amax
    500 saturates after scaling) and the last row's first block a subnormal amax (2^-130)."""
    g = torch.Generator().manual_seed(M + K)
    x = (torch.randn(M, K, generator=g) * 2.0 ** (torch.rand(M, 1, generator=g) * 16 - 8)).to(BF)
    x[0, :32] = 0
    x[0, 32:64] = x[0, 32:64].clamp(-60, 60)
    x[0, 40] = -64.0
    x[0, 64:96] = x[0, 64:96].clamp(-400, 400)
    x[0, 70] = 500.0
    x[-1, :32] = 0
    x[-1, 3], x[-1, 4] = 2.0 ** -130, -(2.0 ** -131)
    return x
