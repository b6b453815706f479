"""The cases of the plain FlashAttention-2 forward tests (tests/test_fa2_plain_edges_surface.py proves the table on the CPU,
tests/test_gpu_fa2_plain_edges.py and tests/test_gpu_fa2_plain_large.py run it): for each of the kernels behind the 28
flash_attn_mma_stages_* names (fa2_plan, csrc/flash_attn.hip) the smallest shapes with one tile, an odd tile count and more than one row
block, head counts that are and are not multiples of 8 (the two block-id -> head maps), the N = 8192 cases, the tensors past 2^32 bytes,
and the input builders. A plain module: nothing here is collected."""
import torch

import fa_reference as far

SPLIT_KV = "flash_attn_mma_stages_split_kv"
SQKV = "flash_attn_mma_stages_split_q_shared_qkv"
TQKV = "flash_attn_mma_stages_split_q_tiling_qkv"
VT = "flash_attn_mma_stages_split_q_shared_kv_swizzle_qkv"  # takes V as [B, H, D, N]

# kind -> what the describe text starts with; "v2/NW" also names the `NW=` of the text
PREFIX = {"splitkv": "fa2_fwd_splitkv<", "v2/2": "fa2_fwd_v2<", "v2/4": "fa2_fwd_v2<", "v2/8": "fa2_fwd_v2<", "m16x": "fa2_fwd_m16x<",
          "m16": "fa2_fwd_m16<", "m16x64r": "fa2_fwd_m16x64r<", "pair2": "fa2_fwd_pair2<", "dw4": "fa2_fwd_dw4<"}


def _rows(kind, name, *shapes):
    return [(kind, name) + s for s in shapes]


# (kind, name, B, H, N, D)
TABLE = (
    _rows("splitkv", SPLIT_KV, (1, 3, 32, 32), (2, 3, 160, 64), (1, 5, 416, 96), (1, 8, 416, 128))
    + _rows("v2/2", SQKV, (1, 3, 64, 32), (1, 8, 192, 64), (2, 3, 320, 96), (1, 5, 192, 128))
    + _rows("v2/4", SQKV, (1, 3, 128, 32), (2, 3, 384, 64), (1, 8, 768, 64), (1, 8, 384, 96), (1, 5, 384, 128), (1, 3, 128, 256), (1, 8, 384, 256))
    + _rows("v2/8", SQKV, (1, 257, 256, 32), (1, 264, 256, 32), (1, 129, 256, 96))
    + _rows("m16x", SQKV, (1, 43, 768, 64), (1, 48, 768, 64), (1, 5, 768, 128), (1, 8, 256, 128))
    + _rows("m16", SQKV, (1, 5, 768, 256), (1, 8, 256, 256))
    + _rows("m16x64r", SQKV, (1, 256, 512, 64), (1, 451, 512, 64), (1, 256, 1536, 64))
    + _rows("pair2", TQKV, (1, 3, 128, 320), (1, 8, 384, 384), (2, 3, 640, 512), (1, 5, 128, 512))
    + _rows("dw4", TQKV, (1, 3, 64, 640), (1, 8, 192, 768), (2, 3, 320, 1024), (1, 5, 64, 1024))
    + _rows("v2/2", VT, (1, 3, 192, 32), (2, 3, 320, 96))
    + _rows("m16x", VT, (1, 48, 768, 64), (1, 5, 768, 128))
    + _rows("m16x64r", VT, (1, 256, 512, 64))
    + _rows("v2/4", VT, (1, 3, 384, 256), (1, 8, 256, 256))
)
KINDS = tuple(PREFIX)
HEAD_DIMS = (32, 64, 96, 128, 256, 320, 384, 512, 640, 768, 1024)


def row_id(row):
    kind, name, B, H, N, D = row
    return "%s%s-%dx%dx%dx%d" % (kind.replace("/", "nw"), "-vt" if name == VT else "", B, H, N, D)


def reaches(text, row):
    """Does the describe text say that `row` runs the kernel it is listed under?"""
    kind, name, B, H, N, D = row
    ok = text.startswith(PREFIX[kind] + "D=%d," % D) and ((",V^T" in text) == (name == VT))
    if kind.startswith("v2/"):
        ok = ok and ("NW=%s," % kind[3:]) in text
    return ok


# ---- N = 8192: (kind, name, B, H, N, D)
LONG = [("v2/4", SQKV, 1, 2, 8192, 32), ("v2/4", SQKV, 1, 2, 8192, 96), ("m16x", SQKV, 1, 2, 8192, 128), ("m16x", VT, 1, 2, 8192, 128),
        ("m16", SQKV, 1, 2, 8192, 256), ("pair2", TQKV, 1, 2, 8192, 512), ("dw4", TQKV, 1, 2, 8192, 1024)]
LONG_BLOCKS = (0, 4032, 8192 - 128)  # first rows of the three blocks of 128 query rows that get an fp64 reference

# ---- tensors past 2^32 bytes: head 2^32 / (2 N D) and at least 8 heads after it lie beyond the 4 GiB line
LARGE = [("dw4", TQKV, 1, 2056, 1024, 1024), ("pair2", TQKV, 1, 4104, 1024, 512), ("m16x64r", SQKV, 1, 65544, 512, 64),
         ("m16x", SQKV, 1, 16392, 1024, 128), ("v2/8", SQKV, 1, 262152, 256, 32)]
PERIOD = 7  # head h of a large case holds the data of head h mod 7


def wrap_shifts(N, D):
    """By how many heads an access to a [H, N, D] fp16 tensor moves when its byte offset wraps at 2^32 or its element offset at 2^31 or
    2^32: {what: heads}. Every shift must be a whole number of heads (the position inside the head then stays), which holds when N D is a
    power of two below 2^31."""
    per = N * D
    out = {}
    for what, span in (("2^32 bytes", 2 ** 32 // 2), ("2^31 elements", 2 ** 31), ("2^32 elements", 2 ** 32)):
        assert span % per == 0, (what, N, D)
        out[what] = span // per
    return out


# ---- tolerances: the project's rules, unchanged


def tol_rule(name, D):
    """fa_tol for the plain names at D <= 128 (fp16 pre-scaled Q), fa_tol_f32 for the kernels that scale the scores in fp32: D >= 256,
    split_kv and the *_acc_f32 names."""
    return far.fa_tol_f32 if D >= 256 or name == SPLIT_KV or "_acc_f32" in name else far.fa_tol


def ref_heads(oracle, q, k, v):
    """oracle.attention_fp64 per flattened head, [B H, N, D] fp64, a few heads at a time so that the scores stay below 2^25 elements."""
    B, H, N, D = q.shape
    qf, kf, vf = (t.reshape(B * H, N, D) for t in (q, k, v))
    step = max(1, 2 ** 25 // (N * N))
    return torch.cat([oracle.attention_fp64(qf[i:i + step], kf[i:i + step], vf[i:i + step]) for i in range(0, B * H, step)])


def head_errors(o, ref, rule):
    """(error, bound, error / bound) of the worst flattened head, each head held to the rule of its own max|O_ref|. o: [B, H, N, D] or
    [n, N, D]; ref: fp64 [n, N, D]."""
    got = o.reshape(ref.shape).double().cpu()
    err = (got - ref).abs().amax(dim=(1, 2))
    bound = torch.tensor([rule(r) for r in ref], dtype=torch.float64)
    worst = int((err / bound).argmax())
    return err[worst].item(), bound[worst].item(), (err / bound).max().item()


# ---- inputs (all on the CPU, fp16)


def gauss(B, H, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, H, N, D, generator=g).half() for _ in range(3)]


def spiked(B, H, N, D, seed):
    """The recipe of test_pingpong_kernels_deferred_max_and_rescale in every head: key norms growing along N (a creeping maximum), one late
    dominant key for row 5 (a forced rescale with a non-trivial alpha) and one early spike for a later row (everything after it ~ -inf)."""
    q, k, v = gauss(B, H, N, D, seed)
    n = B * H
    k = (k.float() * torch.linspace(0.2, 1.6, N).view(1, 1, N, 1)).half()
    qf, kf = q.view(n, N, D), k.view(n, N, D)
    heads = torch.arange(n)
    kf[heads, N - 3 - heads % 5] = qf[:, 5] * 3.0
    kf[heads, 2 + heads % 3] = qf[:, (3 * N) // 10] * 5.0
    return q, k, v


def onehot(B, H, N, D, seed):
    """(q, k, v, V[pi]) with far.onehot_problem(N, D, causal=False) per head, stacked to [B, H, N, D]."""
    heads = [far.onehot_problem(N, D, False, seed + h) for h in range(B * H)]
    q, k, v = (torch.stack([hd[i] for hd in heads]).view(B, H, N, D) for i in range(3))
    vp = torch.stack([hd[2][hd[4]] for hd in heads]).view(B, H, N, D)
    return q, k, v, vp


def onehot_facts(N, D, seed):
    """Of one head of the one-hot problem, in fp64: (gap in nats, dimensions the key code spans, largest off-target mass, largest
    (|O64 - V[pi]| - (2^-10 |V[pi]| + 1e-5)) -- negative when the fp64 softmax itself is inside the bound, largest target score)."""
    q, k, v, _, pi = far.onehot_problem(N, D, False, seed)
    bits = (N - 1).bit_length()
    r = D // bits
    s = q.double() @ k.double().T / D ** 0.5
    lse = torch.logsumexp(s, dim=-1)
    target = s[torch.arange(N), pi]
    o = torch.softmax(s, dim=-1) @ v.double()
    vp = v[pi].double()
    over = ((o - vp).abs() - (2.0 ** -10 * vp.abs() + 1e-5)).max().item()
    other = s.clone()
    other[torch.arange(N), pi] = float("-inf")
    return (target - other.amax(-1)).min().item(), r * bits, (-torch.expm1(target - lse)).max().item(), over, target.max().item()


def derangement(n, seed):
    """A seeded permutation of range(n) without a fixed point."""
    g = torch.Generator().manual_seed(seed)
    while True:
        p = torch.randperm(n, generator=g)
        if not bool((p == torch.arange(n)).any()):
            return p
