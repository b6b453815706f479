"""Helper of the tests of the MoE token path (tests/test_gpu_moe_path.py, tests/test_moe_surface.py): the torch / fp64
references of route, sort and combine. A plain module: nothing here is collected. Cases are made on the CPU, once per process, never modified.

Route inputs sit on a grid so that the fp64 keys of a row are at least GAP = 2^-8 apart (route_case asserts it): softmax logits are a
permutation of distinct multiples of 2^-5 in [-8, 8) (exact in bf16); sigmoid logits are multiples of 2^-5 in [-0.5, 0.5), so s lies in
[0.378, 0.623), and the bias is a permutation of multiples of 2^-2, so two keys differ by at least 0.25 - 0.245.

weight_bound: every fp32 operation of the kernel is within 2^-24 relative (an add, a multiply, an IEEE divide) or 2^-23 (v_exp_f32, 1 ulp);
exp(x) is v_exp_f32(x log2 e), whose rounded product moves the result by |x| 2^-24 relative. A term (exp, or sigmoid = exp, add, divide) is
therefore within (5 + |x|) 2^-24, the sum of n terms adds n 2^-24, and term / sum * scale adds 3 more: in all w 2^-24 (2 (5 + xmax) + n + 3)
with xmax the largest |argument of exp| in the row's tensor and n = k (renormalize) or E."""
import functools

import torch

BF, F32, F64, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int32
GAP = 2.0 ** -8


@functools.lru_cache(maxsize=None)
def route_case(T, E, k, scoring, tie=False):
    """(logits fp32 [T,E] with bf16-exact values, bias fp32 [E] or None, fp64 keys, fp64 s or None)."""
    g = torch.Generator().manual_seed(131 * T + 7 * E + k + (scoring == "sigmoid"))
    if tie:
        logits = torch.full((T, E), 0.25)
        bias = torch.full((E,), 0.5) if scoring == "sigmoid" else None
    elif scoring == "softmax":
        logits = torch.stack([(torch.randperm(512, generator=g)[:E] - 256).float() / 32 for _ in range(T)])
        bias = None
    else:
        logits = (torch.randint(0, 32, (T, E), generator=g) - 16).float() / 32
        bias = torch.randperm(E, generator=g).float() / 4
    s = torch.sigmoid(logits.double()) if scoring == "sigmoid" else None
    keys = logits.double() if scoring == "softmax" else s + bias.double()
    if not tie:
        srt = torch.sort(keys, dim=1).values
        assert E == 1 or float((srt[:, 1:] - srt[:, :-1]).min()) >= GAP
    return logits, bias, keys, s


def route_ref(logits, keys, s, k, renormalize, scale):
    """(ids int32 [T,k], weights fp64 [T,k], bound fp64 [T,k]): a stable descending sort of the fp64 keys; the weights in fp64."""
    ids = torch.sort(-keys, dim=1, stable=True).indices[:, :k]
    E = keys.shape[1]
    if s is None:
        p = torch.exp(logits.double() - logits.double().amax(dim=1, keepdim=True))
        xmax = float((logits.amax(dim=1) - logits.amin(dim=1)).max())
        den = p.gather(1, ids).sum(dim=1, keepdim=True) if renormalize else p.sum(dim=1, keepdim=True)
        n = k if renormalize else E
    else:
        p, xmax, n = s, float(logits.abs().max()), k
        den = p.gather(1, ids).sum(dim=1, keepdim=True) if renormalize else torch.ones(keys.shape[0], 1, dtype=F64)
    w = scale * p.gather(1, ids) / den
    return ids.to(I32), w, w * 2.0 ** -24 * (2 * (5 + xmax) + n + 3)


@functools.lru_cache(maxsize=None)
def sort_ids(n, E, pattern):
    g = torch.Generator().manual_seed(n + 31 * E)
    if pattern == "uniform":
        return torch.randint(0, E, (n,), generator=g, dtype=I32)
    if pattern == "one":
        return torch.full((n,), E - 1, dtype=I32)
    ids = torch.randint(0, E, (n,), generator=g, dtype=I32)
    ids = torch.where(ids % 3 == 1, ids - 1, ids)  # experts 1, 4, 7 ... are empty
    drop = torch.rand(n, generator=g)
    return torch.where(drop < 0.2, torch.full_like(ids, -1), torch.where(drop > 0.9, torch.full_like(ids, E + 3), ids))


def sort_ref(ids, E):
    """(expert_offsets [E+1], src [n], pos [n]) of flat ids by a stable CPU sort; dropped slots (id outside [0,E)) go behind the live rows."""
    ids = ids.flatten().long()
    n, live = ids.numel(), (ids >= 0) & (ids < E)
    order = torch.sort(torch.where(live, ids, torch.full_like(ids, E)), stable=True).indices
    m = int(live.sum())
    src = torch.full((n,), -1, dtype=I32)
    src[:m] = order[:m].to(I32)
    pos = torch.full((n,), -1, dtype=I32)
    pos[order[:m]] = torch.arange(m, dtype=I32)
    off = torch.zeros(E + 1, dtype=I32)
    off[1:] = torch.cumsum(torch.bincount(ids[live], minlength=E), 0).to(I32)
    return off, src, pos


def combine_ref(y, pos, w, residual):
    """(out fp64 [T,N], sum_j |w y| fp64 [T,N]); a pos outside [0, M) contributes nothing."""
    M, live = y.shape[0], (pos >= 0) & (pos < y.shape[0])
    terms = torch.where(live, w.double(), torch.zeros((), dtype=F64))[:, :, None] * y.double()[pos.long().clamp(0, M - 1)]
    out = terms.sum(dim=1)
    return (out if residual is None else out + residual.double()), terms.abs().sum(dim=1)
