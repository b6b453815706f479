"""GPU: every entry of the paged KV-cache path -- 23 attention entries, the *_anyg_* and *_softcap_anyg_* ones at G = 3, whose kernels divide
by the group where their siblings shift, and 5 append entries -- over pools of more than 2^32 elements (2^33 bytes). The pool offset
((pg Hkv + kvh) page + row) D + off of PagedKV::elem (csrc/flash_attn_decode_common.cuh, flash_attn_decode_paged_fp8.cuh, paged_bf16.cuh) and of
the `row` of the five append kernels is formed in 64 bits by casts that no other test holds up: the largest pool elsewhere is a few MiB.

One pair of byte buffers of 8 GiB + 64 KiB + 16 backs every pool view (tests/paged_large_pool.py: the view starts 16 bytes in, so its base is
16-byte but not 32-byte aligned); they are allocated once per module with torch.empty and never filled or moved: a case writes its named pages
and its poison pages only, kilobytes to a few MiB. The module is skipped only on a device with less than 24 GiB in all.

The oracle adds no tolerance. A case from the family's own builders runs on its small pool and is held to the family's fp64 reference by the
family's check (tests/paged_all_entries.py); its live pages are then copied on the device to the named pages of the large view -- on both sides
of element 2^31, 2^32 (2^33 in an e4m3 pool) and at the end of the pool --, the table is remapped, and the entry runs again: O and LSE must keep
every bit, which page placement never changes (test_page_placement_does_not_change_a_bit and its siblings). A wrapped offset reads NaN poison
(tests/test_paged_large_pool_plan.py). The append entries start both pools from poison: afterwards every named page of the large view equals its
page of the small pool byte for byte, every poison page still holds poison, and q_out has the small run's bits. Not covered: q / o / k_new past
2^31 elements, B max_pages past 2^31, rope tables past 4 GiB."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paged_all_entries as ae  # noqa: E402
import paged_large_pool as lp  # noqa: E402

pytestmark = pytest.mark.gpu

DS = list(lp.DS)
ATTN = [e.name for e in ae.ATTN]
DECODE = [e.name for e in ae.ATTN if e.plan]
APPEND = [e.name for e in ae.APPEND]
MIN_TOTAL_MEMORY = 24 << 30


@pytest.fixture(scope="module")
def buffers(built, dev):
    total = torch.cuda.get_device_properties(dev).total_memory
    if total < MIN_TOTAL_MEMORY:
        pytest.skip("a device of %d bytes in all cannot hold two pools of 8 GiB" % total)
    bufs = [torch.empty(lp.BUF_BYTES, dtype=torch.uint8, device=dev) for _ in range(2)]  # a failed allocation is an error
    assert all(b.data_ptr() % 32 == 0 for b in bufs)
    yield bufs
    bufs.clear()
    torch.cuda.empty_cache()


class Large:
    """The [P, Hkv, page, D] views of the two buffers for one pool type, and their pages as byte rows."""

    def __init__(self, bufs, Hkv, D, dtype):
        self.dtype, self.s = dtype, torch.empty(0, dtype=dtype).element_size()
        self.E = Hkv * ae.PAGE * D
        self.PB, self.P = self.E * self.s, lp.pages(self.E, self.s)
        assert lp.BASE + self.P * self.PB <= lp.BUF_BYTES == bufs[0].numel() == bufs[1].numel()
        self.bufs = bufs
        self.k, self.v = (b[lp.BASE:lp.BASE + self.P * self.PB].view(dtype).view(self.P, Hkv, ae.PAGE, D) for b in bufs)
        for t in (self.k, self.v):
            assert t.is_contiguous() and t.data_ptr() % 32 == 16 and t.numel() > 2 ** 32 and t.numel() * self.s > 2 ** 33

    def page(self, which, n):
        assert 0 <= n < self.P
        return self.bufs[which][lp.BASE + n * self.PB:lp.BASE + (n + 1) * self.PB]

    def poison(self, pages):
        for n in pages:
            for w in (0, 1):
                if self.s == 1:
                    self.page(w, n).fill_(ae.poison_bits(self.dtype))
                else:
                    self.page(w, n).view(torch.int16).fill_(ae.poison_bits(self.dtype))

    def read(self, which, pages):
        """[len(pages), PB] uint8 on the CPU."""
        return torch.stack([self.page(which, n) for n in pages]).cpu()

    def still_poison(self, pages):
        want = torch.empty(self.PB, dtype=torch.uint8)
        if self.s == 1:
            want.fill_(ae.poison_bits(self.dtype))
        else:
            want.view(torch.int16).fill_(ae.poison_bits(self.dtype))
        return all(bool((self.read(w, pages) == want).all()) for w in (0, 1))


def relocate(big, d, c, plan, first=()):
    """The device tensors d of case c with its live pages copied to the named pages of the large view and the table remapped; the dead entries
    point at a poison page. first: (b, i) entries that get named pages of `plan["must"]` before the others are handed out. Returns (d', the
    (small page, large page) pairs)."""
    live = ae.live_entries(c["bt"], c["lens"])
    assert len(live) == len(plan["named"])
    rest = [n for n in plan["named"] if n not in plan.get("must", ())]
    order = list(plan.get("must", ()))[:len(first)] + rest
    order += [n for n in plan["named"] if n not in order]
    entries = list(first) + [x for x in live if x not in first]
    big.poison(plan["poison"])
    bt = torch.full_like(c["bt"], plan["dead"])
    small_k, small_v = (d[n].view(torch.uint8).view(-1, big.PB) for n in ("kp", "vp"))
    pairs = []
    for (b, i), n in zip(entries, order):
        j = int(c["bt"][b, i])
        big.page(0, n).copy_(small_k[j])
        big.page(1, n).copy_(small_v[j])
        bt[b, i] = n
        pairs.append((j, n))
    assert int(bt.max()) < big.P and int(bt.min()) >= 0 and len({n for _, n in pairs}) == len(pairs)
    out = dict(d)
    out.update(kp=big.k, vp=big.v, bt=bt.to(d["bt"].device))
    return out, pairs


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def attention_case(buffers, dev, name, D, T, split):
    c = ae.attn_case(name, D, T, split)
    e = c["e"]
    what = "%s D=%d T=%d%s" % (name, D, T, " split" if split else "")
    if split:
        assert ae.plan_of(c)[0] > 1, what
    d = ae.to_dev(c, dev)
    o, lse = ae.run(e, d, c["W"])
    ae.check_small(c, o.cpu(), lse.cpu(), what)
    big = Large(buffers, c["Hkv"], D, ae.pool_type(e))
    plan = lp.plan(big.E, big.s, len(ae.live_entries(c["bt"], c["lens"])), seed=D + T)
    d2, pairs = relocate(big, d, c, plan)
    o2, lse2 = ae.run(e, d2, c["W"])
    top = max(n for _, n in pairs)
    print("%s: %d live pages in a pool of %d, highest page %d, last element offset %d, last byte %d"
          % ((what, len(pairs), big.P, top) + lp.last_offset(top, big.E, big.s)))
    assert top == big.P - 1
    assert bool(torch.isfinite(o2.float()).all()) and not bool(torch.isnan(lse2).any()), what
    assert torch.equal(bits(o2), bits(o)) and torch.equal(bits(lse2), bits(lse)), what
    assert big.still_poison(plan["poison"][:4])


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name", ATTN)
def test_attention_keeps_every_bit_when_its_pages_move_past_two_to_the_32(built, dev, buffers, name, D):
    for T in ((1, 3) if ae.BY_NAME[name].form in ("multi", "prefill") else (1,)):
        attention_case(buffers, dev, name, D, T, False)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name", DECODE)
def test_decode_with_several_splits_over_256_high_pages(built, dev, buffers, name, D):
    attention_case(buffers, dev, name, D, 1, True)


def append_plan(big, c):
    """The plan of an append case: the 8 pages that receive rows are P - 1 and, for every boundary, the page at it and the nearest named page
    below it, as far as 8 go."""
    plan = lp.plan(big.E, big.s, len(ae.live_entries(c["bt"], c["lens"])), seed=c["D"])
    must = [big.P - 1]
    for b in lp.boundaries(big.E, big.s):
        must += [b, max(n for n in plan["named"] if n < b)]
    assert all(n in plan["named"] for n in must)
    plan["must"] = must[:len(c["receivers"])]
    return plan


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name", APPEND)
def test_append_writes_the_named_pages_and_nothing_else(built, dev, buffers, name, D):
    c = ae.append_case(name, D)
    e = c["e"]
    big = Large(buffers, ae.APPEND_HKV, D, ae.pool_type(e))
    plan = append_plan(big, c)
    for rope in ae.ROPES:
        what = "%s D=%d rope=%s" % (name, D, rope)
        d = ae.to_dev(c, dev)  # fresh poisoned small pools
        qo = None if rope == "none" else torch.full_like(d["q"], float("nan"))
        ae.call_append(e, d, rope, qo)
        big.poison(plan["named"])
        d2, pairs = relocate(big, ae.to_dev(c, dev), c, plan, first=c["receivers"])  # copies poisoned pages: the named pages start as poison
        qo2 = None if rope == "none" else torch.full_like(d["q"], float("nan"))
        ae.call_append(e, d2, rope, qo2)
        torch.cuda.synchronize()
        small = [d[n].view(torch.uint8).view(-1, big.PB).cpu() for n in ("kp", "vp")]
        start = c["kp"].view(torch.uint8).view(-1, big.PB)
        written = {n for (j, n) in pairs if not torch.equal(small[0][j], start[j])}
        # rows went to every page that should receive some: among them page P - 1 and, for every boundary, the page at it and one below it
        assert len(written) == len(c["receivers"]) and set(plan["must"]) <= written, (what, sorted(written), plan["must"])
        for w in (0, 1):
            got = big.read(w, [n for _, n in pairs])
            assert torch.equal(got, small[w][[j for j, _ in pairs]]), (what, "KV"[w])
        assert big.still_poison(plan["poison"]), what
        if qo is not None:
            assert bool(torch.isfinite(qo.float()).all()) and torch.equal(bits(qo2), bits(qo)), what
        top = max(written)
        print("%s: rows written to pages %s; last element offset %d, last byte %d" % ((what, sorted(written)) + lp.last_offset(top, big.E, big.s)))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("pair", [("kv_append_paged", "fa2_decode_paged_multi"),
                                  ("kv_append_paged_varlen_bf16_fp8", "fa2_decode_paged_multi_window_sink_bf16_fp8")], ids=["fp16", "bf16-e4m3"])
def test_append_then_decode_on_the_large_view_is_the_small_pools_step(built, dev, buffers, pair, D):
    """One serving step: the K / V rows of the T = 3 newest tokens of every sequence are appended (rotated), then the decode entry attends."""
    a, c = ae.BY_NAME[pair[0]], ae.attn_case(pair[1], D, 3, False)
    e = c["e"]
    g = torch.Generator().manual_seed(D)
    dt = ae.elem_type(e)
    lead = (c["B"] * 3,) if a.varlen else (c["B"], 3)
    new = dict(k_new=torch.randn(*lead, c["Hkv"], D, generator=g).to(dt), v_new=torch.randn(*lead, c["Hkv"], D, generator=g).to(dt),
               rope_table=ae.pkg().kv_append_rope_table(256, D))
    big = Large(buffers, c["Hkv"], D, ae.pool_type(e))
    plan = lp.plan(big.E, big.s, len(ae.live_entries(c["bt"], c["lens"])), seed=D)

    def step(d):
        d = dict(d, **{n: t.to(dev) for n, t in new.items()})
        d["q"] = d["q"].view(*lead, c["Hq"], D)
        if a.varlen:
            d["cu"] = torch.arange(0, 3 * c["B"] + 1, 3, dtype=torch.int32, device=dev)
        qo = torch.full_like(d["q"], float("nan"))
        ae.call_append(a, d, "half", qo)
        d["q"] = qo.view(c["B"], 3, c["Hq"], D)
        return ae.run(e, d, c["W"])

    d = ae.to_dev(c, dev)
    o, lse = step(d)
    d2, pairs = relocate(big, ae.to_dev(c, dev), c, plan)
    o2, lse2 = step(d2)
    assert bool(torch.isfinite(o.float()).all()) and not bool(torch.isnan(lse).any())
    assert torch.equal(bits(o2), bits(o)) and torch.equal(bits(lse2), bits(lse))
    for w, n in ((0, "kp"), (1, "vp")):
        assert torch.equal(big.read(w, [p for _, p in pairs]), d[n].view(torch.uint8).view(-1, big.PB).cpu()[[j for j, _ in pairs]])
    assert big.still_poison(plan["poison"])
