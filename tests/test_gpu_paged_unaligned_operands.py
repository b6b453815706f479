"""GPU: every entry of the paged KV-cache path with the operands its host check admits at 4-byte alignment actually AT 4-byte alignment
(data_ptr() % 16 == 4): block_table, seqlens, cu_q, k_scale, v_scale, sinks, the rope table of the append entries and the lse of the prefill
entries (csrc/paged_entry.h: append_args, prefill_args; fa2d::check_pointers for the decode entries, whose lse stays at 16 bytes and is not
shifted here). The surface tests show that the host accepts such pointers; here the kernels load through them: scalar dword loads everywhere
but the rope table, which the append kernels read as 16-byte vectors of a type that promises 4-byte alignment only (kva::f4u).

Each shifted operand is a copy at base + 4 bytes of a 16-byte aligned buffer. A run with all of them shifted, and one run per operand shifted
alone, must give the bits of the aligned run: O and LSE, or the pools and q_out after an append. A shifted lse lies inside a larger filled
buffer whose words on either side keep their fill. One case per entry from tests/paged_all_entries.py -- 23 attention entries, the *_anyg_* and
*_softcap_anyg_* ones at G = 3 -- and a several-splits case of the six sink decode entries, whose combine kernel reads sinks and seqlens."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paged_all_entries as ae  # noqa: E402

pytestmark = pytest.mark.gpu

DS = [64, 128]
LSE_FILL = 0x4B1DF00D


def shifted(t):
    """A contiguous copy of the int32 / fp32 tensor t at 4 bytes past a 16-byte boundary."""
    assert t.element_size() == 4
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    s = buf[1:1 + t.numel()].view(t.shape)
    s.copy_(t)
    assert s.data_ptr() % 16 == 4 and s.is_contiguous()
    return s


def shifted_lse(shape, dev):
    """(lse at base + 4 bytes, the whole buffer) filled with LSE_FILL."""
    n = 1
    for x in shape:
        n *= x
    buf = torch.full((n + 8,), LSE_FILL, dtype=torch.int32, device=dev)
    lse = buf[1:1 + n].view(torch.float32).view(shape)
    assert lse.data_ptr() % 16 == 4 and lse.is_contiguous()
    return lse, buf


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def attention(dev, name, D, T, split):
    c = ae.attn_case(name, D, T, split)
    e = c["e"]
    what = "%s D=%d T=%d%s" % (name, D, T, " split" if split else "")
    if split:
        assert ae.plan_of(c)[0] > 1, what
    d = ae.to_dev(c, dev)
    assert all(d[n].data_ptr() % 16 == 0 for n in d)
    o, lse = ae.run(e, d, c["W"])
    ae.check_small(c, o.cpu(), lse.cpu(), what)
    names = ae.aligned4(e)
    assert set(names) >= {"bt", "sl"}
    for which in [names] + [[n] for n in names]:
        d2 = dict(d)
        for n in which:
            if n != "lse":
                d2[n] = shifted(d[n])
        o2, lse2 = ae.outputs(d2)
        buf = None
        if "lse" in which:
            lse2, buf = shifted_lse(lse.shape, dev)
        assert o2.data_ptr() % 16 == 0
        ae.call(e, d2, c["W"], o2, lse2)
        torch.cuda.synchronize()
        assert torch.equal(bits(o2), bits(o)) and torch.equal(bits(lse2), bits(lse)), (what, which)
        if buf is not None:
            assert bool((buf[:1] == LSE_FILL).all()) and bool((buf[1 + lse.numel():] == LSE_FILL).all()), (what, which)
    return len(names)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name", [e.name for e in ae.ATTN])
def test_attention_with_operands_at_4_byte_alignment(built, dev, name, D):
    e = ae.BY_NAME[name]
    assert ("lse" in ae.aligned4(e)) == (not e.plan)  # the prefill entries only
    attention(dev, name, D, 3, False)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name", [e.name for e in ae.ATTN if e.plan and e.sink])  # the sink pair and its any-G and soft-cap forms (G = 3)
def test_sink_decode_with_several_splits_reads_sinks_and_lengths_in_the_combine(built, dev, name, D):
    attention(dev, name, D, 1, True)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("name", [e.name for e in ae.APPEND])
def test_append_with_operands_at_4_byte_alignment(built, dev, name, D):
    c = ae.append_case(name, D)
    e = c["e"]
    for rope in ae.ROPES:
        names = [n for n in ae.aligned4(e) if rope != "none" or n != "rope_table"]

        def run(which):
            d = ae.to_dev(c, dev)  # fresh poisoned pools
            assert all(d[n].data_ptr() % 16 == 0 for n in d)
            for n in which:
                d[n] = shifted(d[n])
            qo = None if rope == "none" else torch.full_like(d["q"], float("nan"))
            ae.call_append(e, d, rope, qo)
            torch.cuda.synchronize()
            return d["kp"].view(torch.uint8).cpu(), d["vp"].view(torch.uint8).cpu(), (None if qo is None else bits(qo).cpu())

        kp, vp, qo = run([])
        assert not torch.equal(kp, c["kp"].view(torch.uint8)) and not torch.equal(vp, c["vp"].view(torch.uint8))  # rows were written
        if qo is not None:
            assert bool(torch.isfinite(qo.view(ae.elem_type(e)).float()).all())
        for which in [names] + [[n] for n in names]:
            k2, v2, q2 = run(which)
            assert torch.equal(k2, kp) and torch.equal(v2, vp), (name, D, rope, which)
            assert qo is None or torch.equal(q2, qo), (name, D, rope, which)
