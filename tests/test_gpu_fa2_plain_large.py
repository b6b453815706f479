"""GPU: the plain FlashAttention-2 forward over q, k, v and o of more than 2^32 bytes each, one case per kernel kind that forms
`(size_t)head_i * N * D` (fa2_fwd_dw4, fa2_fwd_pair2, fa2_fwd_m16x64r, fa2_fwd_m16x at D = 128, fa2_fwd_v2 with 8 waves): the cases
fc.LARGE of tests/fa_plain_cases.py, whose plan and wrap images tests/test_fa2_plain_edges_surface.py proves on the CPU. No other test of
this family has a tensor past a few hundred MiB, so a head offset formed in 32 bits would pass them all.

The inputs are periodic in the head: head h holds the data of head h mod 7 (seven Gaussian heads, tiled on the device), and O starts as
NaN. The check needs no reference and no tolerance: O[h] must equal O[h mod 7] on every bit for every h, compared on the device, and no
element may be NaN. A byte or element offset that wraps at 32 bits moves an access by a power-of-two number of heads, never a multiple
of 7, and stays inside the allocation: a wrapped load reads another residue's data, a wrapped store leaves NaN behind. Heads 0..6 are
then held to the fp64 oracle by the rule of the name (fa_tol / fa_tol_f32 of tests/fa_reference.py, per head). Each case needs about
17 GiB and frees it; the module is skipped only on a device with less than 24 GiB in all."""
import pytest
import torch

import fa_plain_cases as fc

pytestmark = pytest.mark.gpu

MIN_TOTAL_MEMORY = 24 << 30


@pytest.fixture(scope="module")
def fa(built, dev):
    total = torch.cuda.get_device_properties(dev).total_memory
    if total < MIN_TOTAL_MEMORY:
        pytest.skip("a device of %d bytes in all cannot hold four tensors of 4 GiB" % total)
    yield built.flash_attn_lib()
    torch.cuda.empty_cache()


def tiled(base, H):
    """[H, N, D] on the device with head h = base[h mod 7]."""
    return base.repeat((H + fc.PERIOD - 1) // fc.PERIOD, 1, 1)[:H].contiguous()


def large_case(fa, dev, oracle, row):
    kind, name, B, H, N, D = row
    what, rule = fc.row_id(row), fc.tol_rule(name, D)
    q7, k7, v7 = fc.gauss(1, fc.PERIOD, N, D, seed=700 + N + D)
    q, k, v = (tiled(t[0].to(dev), H).view(1, H, N, D) for t in (q7, k7, v7))
    o = torch.full_like(q, float("nan"))
    assert all(t.numel() * 2 > 2 ** 32 and t.is_contiguous() for t in (q, k, v, o))
    getattr(fa, name)(q, k, v, o, 2)
    torch.cuda.synchronize()
    o = o.view(H, N, D)
    step = max(fc.PERIOD, 2 ** 28 // (N * D))  # heads per comparison: at most 2^28 elements at a time
    bad = nan = 0
    for h0 in range(0, H, step):
        part = o[h0:h0 + step]
        idx = torch.arange(h0, h0 + part.shape[0], device=dev) % fc.PERIOD
        nan += int(torch.isnan(part).sum())
        bad += int((part.view(torch.int16) != o[:fc.PERIOD].view(torch.int16)[idx]).flatten(1).any(dim=1).sum())
    line = 2 ** 32 // (2 * N * D)
    print("%-40s %d heads, %d beyond byte 2^32 (from head %d): %d differ from head h mod 7, %d NaN" % (what, H, H - line, line, bad, nan))
    assert nan == 0 and bad == 0, (what, bad, nan)
    err, bound, ratio = fc.head_errors(o[:fc.PERIOD], fc.ref_heads(oracle, q7, k7, v7), rule)
    print("%-40s heads 0..6    %.3e / %.3e = %.3f" % (what, err, bound, ratio))
    assert ratio <= 1.0, (what, err, bound)
    del q, k, v, o
    torch.cuda.empty_cache()


def test_dw4_d1024_past_4_gib(fa, dev, oracle):
    large_case(fa, dev, oracle, fc.LARGE[0])


def test_pair2_d512_past_4_gib(fa, dev, oracle):
    large_case(fa, dev, oracle, fc.LARGE[1])


def test_m16x64r_d64_past_4_gib(fa, dev, oracle):
    large_case(fa, dev, oracle, fc.LARGE[2])


def test_m16x_d128_past_4_gib(fa, dev, oracle):
    large_case(fa, dev, oracle, fc.LARGE[3])


def test_v2_8_waves_d32_past_4_gib(fa, dev, oracle):
    large_case(fa, dev, oracle, fc.LARGE[4])
