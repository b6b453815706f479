"""GPU: every entry of the multi-head latent attention path that addresses the paged latent cache -- fa2_decode_paged_mla_bf16, _bf16_fp8 and
_sparse_bf16, kv_append_paged_mla_bf16 and _bf16_fp8, kv_gather_paged_mla_bf16 and _bf16_fp8 -- over a pool of more than 2^32 elements (bf16:
more than 2^33 bytes). The pool offset ((pg << page_shift) + row) 576 + col is formed in 64 bits by casts that no other test holds up
(kv.elem of csrc/flash_attn_decode_paged_mla_bf16.cuh, the hand-written forms of the e4m3 and the sparse decode, the `row` of the two append
and the two gather kernels): the largest latent pool elsewhere is a few MiB.

One byte buffer of 8 GiB + 64 KiB + 16 backs the pool view [P, 16, 576] of either type (tests/paged_mla_large_pool.py: the view starts 16 bytes
in, so its base is 16-byte but not 32-byte aligned); it is allocated once per module with torch.empty and never filled or moved: a case writes
its named pages and its poison pages only. The module is skipped only on a device with less than 16 GiB in all.

The oracle adds no tolerance. A case from the family's own builders runs on its small pool and is held to the family's reference by the
family's check; its live pages are then copied on the device to the named pages of the large view -- on both sides of element 2^31, 2^32 (2^33 in
an e4m3 pool) and at the end of the pool --, the table is remapped, the dead entries point at a poison page, and the entry runs again: O and LSE
keep every bit and are finite. A wrapped offset reads NaN poison (tests/test_paged_mla_large_pool_plan.py). Every case runs under both orders of
the plan: a page of 9216 elements lets the page at the highest boundary and the page at the boundary below it be named only in turn. The append
entries start both pools from poison: afterwards every named page of the large view equals its page of the small pool byte for byte, every
poison page still holds poison, and q_out has the small run's bits. The gather entries: `out` has the small run's bits.

Not covered: q / out / c_new past 2^31 elements; B max_pages past 2^31; the packed kv of the prefill past 2^31 elements -- its
(size_t)r Hq 256 needs a 4 GiB operand and a long prefill, and is left out on purpose."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp8_kv_reference as f8  # noqa: E402
import paged_all_entries as ae  # noqa: E402
import paged_mla_fp8_reference as mf  # noqa: E402
import paged_mla_large_pool as mlp  # noqa: E402
import paged_mla_reference as ml  # noqa: E402
import paged_mla_sparse_reference as sp  # noqa: E402
import test_gpu_mla_prefill as gp  # noqa: E402
import test_gpu_paged_mla as gm  # noqa: E402
import test_gpu_paged_mla_fp8 as gf  # noqa: E402
import test_gpu_paged_sink_attention as sk  # noqa: E402

pytestmark = pytest.mark.gpu

BF, F8 = torch.bfloat16, f8.F8
DC, DR, DK, SCALE, PAGE = ml.DC, ml.DR, ml.DK, ml.SCALE, mlp.PAGE
KVS = mf.KV_SCALES[1]
O_FILL, L_FILL, Q_FILL = sk.O_FILL, sk.L_FILL, 0x3C5A
MIN_TOTAL_MEMORY = 16 << 30
ORDERS = (False, True)  # paged_mla_large_pool.plan's top_first
MODES = ("none", "half", "interleaved")
bits, fbits, check = sk.bits, sk.fbits, sk.check
RATIOS = {}
DEV = "cuda"


def note(group, ratio):
    RATIOS[group] = max(RATIOS.get(group, 0.0), ratio)


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def i32(x):
    return torch.tensor(list(x), dtype=torch.int32, device=DEV)


@pytest.fixture(scope="module")
def buffer(built, dev):
    total = torch.cuda.get_device_properties(dev).total_memory
    print("total device memory: %d bytes" % total)
    if total < MIN_TOTAL_MEMORY:
        pytest.skip("a device of %d bytes in all cannot hold a pool of 8 GiB" % total)
    bufs = [torch.empty(mlp.BUF_BYTES, dtype=torch.uint8, device=dev)]  # a failed allocation is an error
    assert bufs[0].data_ptr() % 32 == 0
    yield bufs
    bufs.clear()
    torch.cuda.empty_cache()


class Large:
    """The [P, 16, 576] view of the buffer for one pool type, and its pages as byte rows."""

    def __init__(self, bufs, dtype):
        self.dtype, self.s = dtype, torch.empty(0, dtype=dtype).element_size()
        self.E = mlp.E
        self.PB, self.P = self.E * self.s, mlp.pages(self.E, self.s)
        self.buf = bufs[0]
        assert mlp.BASE + self.P * self.PB <= mlp.BUF_BYTES == self.buf.numel() < mlp.BASE + (self.P + 1) * self.PB
        self.pool = self.buf[mlp.BASE:mlp.BASE + self.P * self.PB].view(dtype).view(self.P, PAGE, DK)
        assert self.pool.is_contiguous() and self.pool.data_ptr() % 32 == 16 and self.pool.numel() > 2 ** 32
        assert self.pool.numel() * self.s > 2 ** 33 or self.s == 1

    def page(self, n):
        assert 0 <= n < self.P
        return self.buf[mlp.BASE + n * self.PB:mlp.BASE + (n + 1) * self.PB]

    def poison(self, pages):
        for n in pages:
            if self.s == 1:
                self.page(n).fill_(ae.poison_bits(self.dtype))
            else:
                self.page(n).view(torch.int16).fill_(ae.poison_bits(self.dtype))

    def read(self, pages):
        """[len(pages), PB] uint8 on the CPU."""
        return torch.stack([self.page(n) for n in pages]).cpu()

    def still_poison(self, pages):
        want = torch.empty(self.PB, dtype=torch.uint8)
        if self.s == 1:
            want.fill_(ae.poison_bits(self.dtype))
        else:
            want.view(torch.int16).fill_(ae.poison_bits(self.dtype))
        return bool((self.read(pages) == want).all())


def relocate(big, small, bt, lens, plan, first=()):
    """The live pages of the small pool (on the device) copied to the named pages of the large view and the table remapped; the dead entries
    point at a poison page. first: the live (b, i) entries that get the pages plan["must"] -- P - 1 and the pages at and below every boundary
    -- before the others are handed out. Returns (the table on the device, the (small page, large page) pairs, the pages `first` got)."""
    live = ae.live_entries(bt, lens, PAGE)
    assert len(live) == len(plan["named"]) and all(x in live for x in first)
    must = plan["must"][:len(first)] if first else []
    order = must + [n for n in plan["named"] if n not in must]
    entries = list(first) + [x for x in live if x not in set(first)]
    big.poison(plan["poison"])
    out = torch.full_like(bt, plan["dead"])
    rows = small.view(torch.uint8).view(-1, big.PB)
    pairs = []
    for (b, i), n in zip(entries, order):
        j = int(bt[b, i])
        big.page(n).copy_(rows[j])
        out[b, i] = n
        pairs.append((j, n))
    assert int(out.max()) < big.P and int(out.min()) >= 0 and len({n for _, n in pairs}) == len(pairs) == len(live)
    return out.to(DEV), pairs, {n for (_, n), x in zip(pairs, entries) if x in set(first)}


def report(what, big, plan, pages):
    top = max(pages)
    elem, byte = mlp.last_offset(top, big.E, big.s)
    print("%s: %d pages in a pool of %d, highest page %d, last element offset %d, last byte %d" % (what, len(pages), big.P, top, elem, byte))
    assert top == big.P - 1 and (byte > 2 ** 33 if big.s == 2 else elem > 2 ** 33)


# ---------------------------------------------------------------------------------------------------- decode

def run_decode(family, q, pool, bt, lens, idx=None):
    """(o, lse) on the device; q, pool, bt are on the device already."""
    c = pkg()
    B, T, Hq, _ = q.shape
    o = torch.full((B, T, Hq, DC), O_FILL, dtype=torch.int16, device=DEV).view(BF)
    lse = torch.full((B, T, Hq), L_FILL, dtype=torch.int32, device=DEV).view(torch.float32)
    if family == "sparse":
        need = c.fa2_decode_paged_mla_sparse_bf16_plan(B, T, Hq, idx.shape[2], bt.shape[1], PAGE)
        ws = torch.empty(max(need[2], 16), dtype=torch.uint8, device=DEV)
        c.fa2_decode_paged_mla_sparse_bf16(q, pool, bt, i32(lens), idx, SCALE, o, lse, ws)
    elif family == "fp8":
        need = c.fa2_decode_paged_mla_bf16_fp8_plan(B, T, Hq, bt.shape[1], PAGE)
        ws = torch.empty(max(need[2], 16), dtype=torch.uint8, device=DEV)
        c.fa2_decode_paged_mla_bf16_fp8(q, pool, bt, i32(lens), mf.scale_t(KVS).to(DEV), SCALE, o, lse, ws)
    else:
        need = c.fa2_decode_paged_mla_bf16_plan(B, T, Hq, bt.shape[1], PAGE)
        ws = torch.empty(max(need[2], 16), dtype=torch.uint8, device=DEV)
        c.fa2_decode_paged_mla_bf16(q, pool, bt, i32(lens), SCALE, o, lse, ws)
    torch.cuda.synchronize()
    return o, lse, need[0]


def decode_case(family, T, Hq, split):
    """(q, lens, pool, bt, idx or None, the reference) from the family's own builders, page 16."""
    if family == "sparse":
        q, lens, (pool, bt) = sp.split_case(T, Hq) if split else sp.one_case(T, Hq, PAGE)
        idx = sp.split_indices(T, Hq, False) if split else sp.one_indices(T, Hq, PAGE, 200)
        return q, lens, pool, bt, idx, sp.decode_sparse(q, pool, bt, lens, idx, SCALE)
    if family == "fp8":
        q, lens, (pool, bt) = mf.split_case(T, Hq, KVS) if split else mf.one_case(T, Hq, PAGE, KVS)
        return q, lens, pool, bt, None, mf.decode(q, pool, bt, lens, KVS, SCALE)
    q, lens, (pool, bt) = ml.split_case(T, Hq) if split else ml.one_case(T, Hq, PAGE)
    return q, lens, pool, bt, None, ml.decode(q, pool, bt, lens, SCALE)


def listed_entries(idx, bt, lens, T):
    """The live (b, i) table entries whose page holds a position that some valid slot lists, in table order."""
    vis = sp.visible(lens, T, bt.shape[1] * PAGE)
    seen = set()
    for b in range(len(lens)):
        for t in range(T):
            seen.update((b, p // PAGE) for _, p in sp.valid_slots(idx[b, t], vis[b][t]))
    return sorted(seen)


DECODE_CASES = [(1, 16, False), (3, 5, False), (2, 40, True)]
SPARSE_CASES = [(3, 5, False), (2, 40, True)]


@pytest.mark.parametrize("case", [(f, *c) for f in ("bf16", "fp8") for c in DECODE_CASES] + [("sparse", *c) for c in SPARSE_CASES],
                         ids=lambda c: "%s-T%dxHq%d%s" % (c[0], c[1], c[2], "-split" if c[3] else ""))
def test_decode_keeps_every_bit_when_its_pages_move_past_two_to_the_32(built, dev, buffer, case):
    family, T, Hq, split = case
    q, lens, pool, bt, idx, ref = decode_case(family, T, Hq, split)
    what = "mla %s decode T=%d Hq=%d%s" % (family, T, Hq, " split" if split else "")
    qd, pd = q.to(DEV), pool.to(DEV)
    xd = None if idx is None else idx.to(DEV)
    o, lse, S = run_decode(family, qd, pd, bt.to(DEV), lens, xd)
    assert (S > 1) == split, (what, S)
    note(family, check(o.cpu(), lse.cpu(), *ref, what + ", small pool"))
    big = Large(buffer, F8 if family == "fp8" else BF)
    live = ae.live_entries(bt, lens, PAGE)
    first = listed_entries(idx, bt, lens, T) if family == "sparse" else live
    for top_first in ORDERS:
        plan = mlp.plan(big.E, big.s, len(live), seed=T + Hq, top_first=top_first)
        assert len(first) >= len(plan["must"])  # the high pages go to entries the kernel reads
        bt2, pairs, got = relocate(big, pd, bt, lens, plan, first=first[:len(plan["must"])])
        assert got == set(plan["must"])
        o2, lse2, _ = run_decode(family, qd, big.pool, bt2, lens, xd)
        report("%s, %s" % (what, "top first" if top_first else "low first"), big, plan, [n for _, n in pairs])
        assert bool(torch.isfinite(o2.float()).all()) and not bool(torch.isnan(lse2).any()), what
        assert torch.equal(bits(o2), bits(o)) and torch.equal(fbits(lse2), fbits(lse)), what
        assert big.still_poison(plan["poison"][:4] + plan["poison"][-4:])


# ---------------------------------------------------------------------------------------------------- append

def append_problem(fp8):
    """The family's _append_problem with a pool that starts as poison."""
    lens, pool, bt, cu, c_new, k_pe, q = (gf if fp8 else gm)._append_problem()
    return lens, ae.poisoned(tuple(pool.shape), F8 if fp8 else BF), bt, cu, c_new, k_pe, q


def call_append(fp8, dv, pool, bt, lens, cu, rope, with_q=True):
    """dv: the new rows and q on the device. Returns q_out."""
    c_new, k_pe, q, table = dv
    qo = torch.full(q.shape, Q_FILL, dtype=torch.int16, device=DEV).view(BF) if with_q else None
    tb = None if rope == "none" else table
    if fp8:
        pkg().kv_append_paged_mla_bf16_fp8(c_new, k_pe, pool, bt, i32(lens), i32(cu), mf.scale_t(KVS).to(DEV), q if with_q else None, qo, tb, rope)
    else:
        pkg().kv_append_paged_mla_bf16(c_new, k_pe, pool, bt, i32(lens), i32(cu), q if with_q else None, qo, tb, rope)
    torch.cuda.synchronize()
    return qo


def receivers(lens, T_new):
    """The (b, i) table entries whose page receives a row: the last T_b positions of every sequence."""
    out = []
    for b, (n, t) in enumerate(zip(lens, T_new)):
        out += [(b, i) for i in sorted({p // PAGE for p in range(n - t, n)})]
    return out


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_append_writes_the_named_pages_and_nothing_else(built, dev, buffer, fp8):
    lens, pool, bt, cu, c_new, k_pe, q = append_problem(fp8)
    table = pkg().kv_append_rope_table(gm.APPEND_NMAX, DR)
    dv = tuple(t.to(DEV) for t in (c_new, k_pe, q, table))
    recv = receivers(lens, gm.APPEND_T)
    big = Large(buffer, F8 if fp8 else BF)
    live = ae.live_entries(bt, lens, PAGE)
    start = pool.view(torch.uint8).view(-1, big.PB)
    for mode, rope in enumerate(MODES):
        for top_first in ORDERS:
            what = "mla %s append rope=%s, %s" % ("e4m3" if fp8 else "bf16", rope, "top first" if top_first else "low first")
            plan = mlp.plan(big.E, big.s, len(live), seed=mode, top_first=top_first)
            assert len(recv) >= len(plan["must"]), (len(recv), plan["must"])
            small = pool.to(DEV)
            qo = call_append(fp8, dv, small, bt.to(DEV), lens, cu, rope)
            big.poison(plan["named"])
            bt2, pairs, got = relocate(big, pool.to(DEV), bt, lens, plan, first=recv[:len(plan["must"])])  # copies poisoned pages
            qo2 = call_append(fp8, dv, big.pool, bt2, lens, cu, rope)
            after = small.view(torch.uint8).view(-1, big.PB).cpu()
            written = {n for (j, n) in pairs if not torch.equal(after[j], start[j])}
            # rows went to every page that should receive some: among them P - 1 and, for every boundary, a page at or above it and one below
            assert len(written) == len(recv) and got == set(plan["must"]) <= written, (what, sorted(written), plan["must"])
            assert torch.equal(big.read([n for _, n in pairs]), after[[j for j, _ in pairs]]), what
            assert big.still_poison(plan["poison"]), what
            seq = slice(cu[0], cu[-1])
            assert bool(torch.isfinite(qo[seq].float()).all()) and torch.equal(bits(qo2), bits(qo)), what
            report(what + ": rows written to pages %s" % sorted(written), big, plan, sorted(written))


# ---------------------------------------------------------------------------------------------------- gather

def gather_problem(fp8):
    """(pool, bt, lens, [(starts, counts)]): the families' gather problems; every row read lies inside its sequence or past the table."""
    if fp8:
        _, lens, (pool, bt) = mf.split_case(1, 16, KVS)
        return pool, bt, lens, [(None, list(lens)), ([900, 17, 250, 0, 0], [100, 100, 7, 100, 0])]
    pool, bt = gp._gather_problem(PAGE)
    return pool, bt, gp.GATHER_LENS, [(None, [100, 30, 256]), ([0, 7, 64], [100, 30, 256 - 64 + 20])]


def call_gather(fp8, pool, bt, cu, total, starts):
    out = torch.full((total, DK), Q_FILL, dtype=torch.int16, device=DEV).view(BF)
    st = None if starts is None else i32(starts)
    if fp8:
        pkg().kv_gather_paged_mla_bf16_fp8(pool, bt, i32(cu), mf.scale_t(KVS).to(DEV), out, st)
    else:
        pkg().kv_gather_paged_mla_bf16(pool, bt, i32(cu), out, st)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_gather_reads_the_named_pages(built, dev, buffer, fp8):
    pool, bt, lens, rounds = gather_problem(fp8)
    big = Large(buffer, F8 if fp8 else BF)
    live = ae.live_entries(bt, lens, PAGE)
    pd = pool.to(DEV)
    Nmax = bt.shape[1] * PAGE
    for k, (starts, counts) in enumerate(rounds):
        st = starts or [0] * len(counts)
        assert all(s0 + n <= max(ln, s0) or s0 + n > Nmax for s0, n, ln in zip(st, counts, lens))
        read = sorted({(b, p // PAGE) for b, (s0, n) in enumerate(zip(st, counts)) for p in range(s0, min(s0 + n, lens[b]))})
        assert all(x in live for x in read)
        cu = [2]
        for n in counts:
            cu.append(cu[-1] + n)
        total = cu[-1] + 3
        out = call_gather(fp8, pd, bt.to(DEV), cu, total, starts)
        for top_first in ORDERS:
            what = "mla %s gather starts=%s, %s" % ("e4m3" if fp8 else "bf16", starts, "top first" if top_first else "low first")
            plan = mlp.plan(big.E, big.s, len(live), seed=k, top_first=top_first)
            assert len(read) >= len(plan["must"])
            bt2, pairs, got = relocate(big, pd, bt, lens, plan, first=read[:len(plan["must"])])
            out2 = call_gather(fp8, big.pool, bt2, cu, total, starts)
            # taken from named pages on both sides of every boundary and from P - 1
            assert got == set(plan["must"]) and all(any(n >= b_ for n in got) and any(n < b_ for n in got) for b_ in mlp.boundaries(big.E, big.s))
            seq = out2[cu[0]:cu[-1]]
            assert bool(torch.isfinite(seq.float()).all()) and torch.equal(bits(out2), bits(out)), what
            assert big.still_poison(plan["poison"][:4] + plan["poison"][-4:])
            report(what, big, plan, sorted(got))


# ---------------------------------------------------------------------------------------------------- chain

@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "e4m3"])
def test_append_then_decode_on_the_large_view_is_the_small_pools_step(built, dev, buffer, fp8):
    """One serving step on the (2, 40) several-splits problem: the rows of the two newest tokens of every sequence are appended (rope half),
    then the decode entry attends with the rotated q."""
    T, Hq = 2, 40
    q4, lens, (pool, bt) = mf.split_case(T, Hq, KVS) if fp8 else ml.split_case(T, Hq)
    B = len(lens)
    g = torch.Generator().manual_seed(5)
    cu = list(range(0, T * B + 1, T))
    c_new, k_pe = ((torch.randn(T * B, d, generator=g) * SCALE).to(BF) for d in (DC, DR))
    table = pkg().kv_append_rope_table(bt.shape[1] * PAGE, DR)
    dv = tuple(t.to(DEV) for t in (c_new, k_pe, q4.reshape(T * B, Hq, DK).contiguous(), table))
    big = Large(buffer, F8 if fp8 else BF)
    live = ae.live_entries(bt, lens, PAGE)
    family = "fp8" if fp8 else "bf16"

    def step(pl, btd):
        qo = call_append(fp8, dv, pl, btd, lens, cu, "half")
        return run_decode(family, qo.view(B, T, Hq, DK), pl, btd, lens)[:2]

    small = pool.to(DEV)
    o, lse = step(small, bt.to(DEV))
    after = small.view(torch.uint8).view(-1, big.PB).cpu()
    assert not torch.equal(after, pool.view(torch.uint8).view(-1, big.PB))
    assert bool(torch.isfinite(o.float()).all()) and not bool(torch.isnan(lse).any())
    recv = receivers(lens, [T if n >= T else n for n in lens])
    for top_first in ORDERS:
        plan = mlp.plan(big.E, big.s, len(live), seed=9, top_first=top_first)
        bt2, pairs, got = relocate(big, pool.to(DEV), bt, lens, plan, first=recv[:len(plan["must"])])
        o2, lse2 = step(big.pool, bt2)
        assert torch.equal(bits(o2), bits(o)) and torch.equal(fbits(lse2), fbits(lse)), top_first
        assert torch.equal(big.read([n for _, n in pairs]), after[[j for j, _ in pairs]])
        assert big.still_poison(plan["poison"])
        report("mla %s chain append + decode, %s" % (family, "top first" if top_first else "low first"), big, plan, [n for _, n in pairs])


def test_zz_summary_of_error_over_bound(built, dev):
    """The largest O err / bound of the small-pool runs per family. Not an assertion of its own -- every case asserted err <= bound where it
    ran; the large-pool runs are held by bit equality."""
    for group, r in sorted(RATIOS.items()):
        print("RATIOS %-28s %.4f" % (group, r))
    assert all(r <= 1.0 for r in RATIOS.values())
