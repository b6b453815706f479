"""Helpers of the tests of multi-head latent attention over a paged latent cache held in FP8 (tests/test_paged_mla_fp8_surface.py,
tests/test_gpu_paged_mla_fp8.py): the fp64 reference and the bf16 emulation of
cuda_learn_notes_amd.fa2_decode_paged_mla_bf16_fp8, the builder of pools of codes, and the cases of the GPU test. Built from fp8_kv_reference
(quantize, dequantize, bound, NAN_BYTE) and paged_mla_reference; nothing is free-standing.

The pool is e4m3fn [P, page, 576]; kv_scale is ONE fp32 number for the whole pool: value = e4m3(code) * kv_scale.
  fp64 reference   paged_mla_reference.decode on dequantize(pool, kv_scale, float64).
  emulation        paged_mla_reference.emul_rows' six steps on the CODES taken as bf16 values (every e4m3 value is one), which is what the kernel's
                   LDS image holds: scores from the bf16 q and the codes in fp64, cast to fp32 and multiplied there by the fp32 number
                   fp32(fp32(scale * log2 e) * kv_scale); P = exp2 of the scores minus the row's final maximum; P rounded to bf16; P V over the
                   codes accumulated in fp64; divided by the fp32 row sum of the unrounded P; times kv_scale in fp32; O rounded once to bf16.
With kv_scale a power of two every product with it is exact, and both equal paged_mla_reference.decode on the pool dequantised to bf16, bit for
bit (asserted by the surface test). The criteria are the family's, no new tolerance: O within paged_bf16_reference.o_bound(emul, ref), LSE
within decode_reference.lse_tol, -inf rows and zero rows exactly.

A plain module: nothing here is collected. Cases are made on the CPU, once per process, and never modified."""
import functools

import torch

import fp8_kv_reference as f8
import multi_decode_reference as mr
import paged_mla_reference as ml
import paged_softcap_reference as cr

BF, F8 = torch.bfloat16, f8.F8
DC, DR, DK, SCALE = ml.DC, ml.DR, ml.DK, ml.SCALE
NAN_BYTE = f8.NAN_BYTE
NEG_INF = ml.NEG_INF
KV_SCALES = (2.0 ** -8, 0.003)  # a power of two (every product with it exact) and one that is not


def scale_t(kv_scale):
    """kv_scale as the fp32 [1] tensor the entries take."""
    return torch.tensor([kv_scale], dtype=torch.float32)


def quantize(x, kv_scale):
    """fp8_kv_reference.quantize with the one scale of the pool."""
    return f8.quantize(x, scale_t(kv_scale))


def dequantize(codes, kv_scale, dtype=torch.float32):
    return f8.dequantize(codes, scale_t(kv_scale), dtype)


# ---------------------------------------------------------------------------------------------------- reference and emulation

def emul_rows(q, codes, vis, scale, kv_scale, dv, on_scores=1, on_o=1):
    """O_emul fp64 [R, dv] holding bf16 values: queries q [R, dk] (bf16) over rows of codes [N, dk] (bf16 values), query r seeing the first vis[r]
    keys. on_scores / on_o: how many times kv_scale multiplies the scores / O (1 and 1: the kernel; anything else: a mistake the surface test
    shows the bound can see)."""
    R = q.shape[0]
    out = torch.zeros(R, dv, dtype=torch.float64)
    top = int(max(vis)) if len(vis) else 0
    if top == 0:
        return out
    vist = torch.tensor(list(vis), dtype=torch.int64)
    live = vist > 0
    kvs = torch.tensor(kv_scale, dtype=torch.float32)
    mult = torch.tensor(cr.f32(scale) * ml.LOG2E, dtype=torch.float32)
    for _ in range(on_scores):
        mult = mult * kvs                                                                                        # fp32(fp32(scale log2e) kv_scale)
    s = (q.double() @ codes[:top].double().T).float() * mult                                                     # 1
    s = s.masked_fill(torch.arange(top)[None, :] >= vist[:, None], NEG_INF)[live]
    p = torch.exp2(s - s.max(dim=-1, keepdim=True).values)                                                       # 2
    lsum = p.sum(dim=-1, dtype=torch.float32)                                                                    # 5: of the unrounded P
    o = (p.bfloat16().double() @ codes[:top, :dv].double() / lsum.double()[:, None]).float()                    # 3, 4, 5
    for _ in range(on_o):
        o = o * kvs                                                                                              # in fp32, in front of the rounding
    out[live] = o.bfloat16().double()                                                                            # 6
    return out


def decode(q, pool, block_table, lens, kv_scale, scale, dv=DC, on_scores=1, on_o=1):
    """(O [B,T,Hq,dv], LSE [B,T,Hq], O_emul [B,T,Hq,dv]), all fp64: q bf16 [B,T,Hq,dk], pool e4m3fn [P,page,dk], kv_scale a Python float (taken
    as fp32). O and LSE are paged_mla_reference.decode's on the pool dequantised in float64; the emulation is emul_rows above."""
    B, T, Hq, dk = q.shape
    Nmax = block_table.shape[1] * pool.shape[1]
    O, L, _ = ml.decode(q, dequantize(pool, kv_scale, torch.float64), block_table, lens, scale, dv)
    dense = ml.gather(pool.to(BF), block_table, lens)  # the codes as bf16 values; a dead page is never followed
    vis = mr.visible(lens, T, Nmax)
    E = torch.zeros(B, T, Hq, dv, dtype=torch.float64)
    for b in range(B):
        vb = vis[b * T:(b + 1) * T]
        if max(vb) == 0:
            continue
        for h in range(Hq):
            E[b, :, h] = emul_rows(q[b, :, h], dense[b], vb, scale, kv_scale, dv, on_scores, on_o)
    return O, L, E


# ---------------------------------------------------------------------------------------------------- pools of codes

def make_pool(codes, page, lens, seed=0):
    """(pool e4m3fn [P,page,dk], block_table int32 [B,max_pages]) of dense rows of codes [B,Nmax,dk], as paged_mla_reference.make_pool builds
    its pools -- the same pages in the same places for the same seed -- but every page no live entry names holds 0x7f, the e4m3 NaN."""
    import paged_decode_reference as pr
    c = f8.bits(codes)
    kp, _, bt = pr.make_pool(c[:, None], c[:, None, :, :1], page, lens, seed=seed, fill=NAN_BYTE)
    return kp[:, 0].contiguous().view(F8), bt


def zero_dead_pages(pool, block_table, lens):
    """A copy of the pool whose pages no live table entry names hold zeros."""
    page = pool.shape[1]
    live = set()
    for b in range(block_table.shape[0]):
        n = min(max(int(lens[b]), 0), block_table.shape[1] * page)
        live.update(int(block_table[b, i]) for i in range(-(-n // page)))
    out = f8.bits(pool).clone()
    for pg in range(pool.shape[0]):
        if pg not in live:
            out[pg] = 0
    return out.view(F8)


# ---------------------------------------------------------------------------------------------------- the cases of the GPU test

ONE_TH = [(1, 1), (1, 16), (1, 17), (3, 5), (1, 64), (2, 128), (8, 3)]
SPLIT_TH = ml.SPLIT_TH
ONE_PAGES = (16, 64)


@functools.lru_cache(maxsize=None)
def one_case(T, Hq, page, kv_scale):
    """case 1: (q [8,T,Hq,576], lens, (pool of codes, block_table)): paged_mla_reference.one_case's q, lengths and dense rows, quantised on the
    CPU at kv_scale; one split."""
    q, lens, _ = ml.one_case(T, Hq, page)
    codes = quantize(ml._dense(len(lens), ml.ONE_NMAX), kv_scale)
    return q, lens, make_pool(codes, page, lens, seed=T + Hq)


@functools.lru_cache(maxsize=None)
def split_case(T, Hq, kv_scale):
    """case 2: (q [5,T,Hq,576], lens, (pool of codes, block_table)): paged_mla_reference.split_case quantised; Nmax 1024 at page 16."""
    q, lens, _ = ml.split_case(T, Hq)
    codes = quantize(ml._dense(len(lens), ml.SPLIT_PAGE * ml.SPLIT_MAX_PAGES), kv_scale)
    return q, lens, make_pool(codes, ml.SPLIT_PAGE, lens, seed=Hq)


def parity_cases():
    """Every parity case of the GPU file as (what, q, lens, (pool, block_table), kv_scale)."""
    for kv_scale in KV_SCALES:
        for (T, Hq) in ONE_TH:
            for page in ONE_PAGES:
                yield ("one", T, Hq, page, kv_scale), *one_case(T, Hq, page, kv_scale), kv_scale
        for (T, Hq) in SPLIT_TH:
            yield ("split", T, Hq, ml.SPLIT_PAGE, kv_scale), *split_case(T, Hq, kv_scale), kv_scale


def all_finite_codes():
    """The 254 finite e4m3fn codes as uint8, subnormals and -0 included: every byte but 0x7f and 0xff."""
    return torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def scale_case(T, Hq, split, kv_scale, scale):
    """paged_mla_reference.scale_case over the pool of codes at kv_scale."""
    q, lens, pool = split_case(T, Hq, kv_scale) if split else one_case(T, Hq, 16, kv_scale)
    q = ml.times(q, ml.Q_MULT)
    return q, lens, pool, decode(q, *pool, lens, kv_scale, scale), decode(q, *pool, lens, kv_scale, SCALE)
