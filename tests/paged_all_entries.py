"""Every entry of the paged KV-cache path behind one calling convention, for the tests that run ALL of them (tests/test_gpu_paged_large_pool.py,
tests/test_gpu_paged_unaligned_operands.py): the 23 attention entries (fa2_decode_paged*, fa2_prefill_paged*) and the 5 append entries
(kv_append_paged*), one small case per entry from the builders the families' own tests use (paged_decode_reference.make_pool,
fp8_kv_reference.make_pool, paged_bf16_fp8_reference.quantize_pools, paged_sink_reference.sinks_mixed), and the check of a result against the
family's fp64 reference with the family's own check function and bound -- no tolerance is defined here:
    fp16 pools        the check() of tests/test_gpu_fa2_decode_paged.py, ..._multi.py, test_gpu_fa2_prefill_paged.py, ..._varlen.py
    fp16 over e4m3    the check() of tests/test_gpu_fa2_decode_paged_fp8.py and fp8_paged_attn_cases.Entry.check
    bf16 (over e4m3)  paged_sink_reference (paged_bf16_fp8_reference) .prefill / .decode, held by the check() of
                      tests/test_gpu_paged_sink_attention.py; an entry without sinks is that reference with sinks of -inf, one without a window
                      that reference with W = None, which is how paged_bf16_fp8_reference already treats sinks = None. The *_anyg_* entries run
                      with G = Hq / Hkv = 3, which their power-of-two siblings refuse, against the same references (both index the KV head as
                      h // G).
    *_softcap_anyg_*  paged_softcap_reference.prefill / .decode with the scale and the cap of its sensitive cases (scale_for(D), CAP = 2, q x 4:
                      most scores sit past the cap), held by the same check(), as tests/test_gpu_paged_softcap_attention.py does.
The 4-byte operand sets are those of csrc/paged_entry.h (prefill_args, append_args) and fa2d::check_pointers: everything behind q and the pools
in a decode entry; that and lse in a prefill entry; every int32 / fp32 input of an append entry, the rope table among them. They agree with the
`for i in (...)  # ... 4-byte alignment` lists of the surface tests. A plain module: nothing here is collected."""
import collections
import functools

import torch

import fp8_kv_reference as f8
import fp8_paged_attn_cases as cs
import paged_bf16_fp8_reference as b8
import paged_decode_reference as pr
import paged_sink_reference as sr
import paged_softcap_reference as cr
import test_gpu_fa2_decode_paged as t_dec
import test_gpu_fa2_decode_paged_fp8 as t_dec8
import test_gpu_fa2_decode_paged_multi as t_multi
import test_gpu_fa2_prefill_paged as t_pre
import test_gpu_fa2_prefill_paged_varlen as t_var
import test_gpu_paged_sink_attention as t_sink

BF, HALF, F8 = torch.bfloat16, torch.float16, f8.F8
PAGE = 16
NEG_INF = float("-inf")

# form: "single" q [B,Hq,D]; "multi" / "prefill" q [B,T,Hq,D]; "varlen" q packed [total_q,Hq,D] with cu_q. plan: a decode entry (splits, workspace).
# anyg: any Hq / Hkv in 1 ... 16 (the case takes ANYG); softcap: softmax_scale and softcap follow the sinks
Attn = collections.namedtuple("Attn", "name bf16 fp8 form window sink plan anyg softcap", defaults=(False, False))
ATTN = [
    Attn("fa2_decode_paged", False, False, "single", False, False, True),
    Attn("fa2_decode_paged_multi", False, False, "multi", False, False, True),
    Attn("fa2_prefill_paged", False, False, "prefill", False, False, False),
    Attn("fa2_prefill_paged_varlen", False, False, "varlen", False, False, False),
    Attn("fa2_decode_paged_fp8", False, True, "single", False, False, True),
    Attn("fa2_decode_paged_multi_fp8", False, True, "multi", False, False, True),
    Attn("fa2_prefill_paged_fp8", False, True, "prefill", False, False, False),
    Attn("fa2_prefill_paged_varlen_bf16", True, False, "varlen", False, False, False),
    Attn("fa2_decode_paged_multi_bf16", True, False, "multi", False, False, True),
    Attn("fa2_prefill_paged_varlen_window_bf16", True, False, "varlen", True, False, False),
    Attn("fa2_decode_paged_multi_window_bf16", True, False, "multi", True, False, True),
    Attn("fa2_prefill_paged_varlen_window_sink_bf16", True, False, "varlen", True, True, False),
    Attn("fa2_decode_paged_multi_window_sink_bf16", True, False, "multi", True, True, True),
    Attn("fa2_prefill_paged_varlen_window_sink_bf16_fp8", True, True, "varlen", True, True, False),
    Attn("fa2_decode_paged_multi_window_sink_bf16_fp8", True, True, "multi", True, True, True),
    Attn("fa2_prefill_paged_varlen_window_sink_anyg_bf16", True, False, "varlen", True, True, False, True),
    Attn("fa2_decode_paged_multi_window_sink_anyg_bf16", True, False, "multi", True, True, True, True),
    Attn("fa2_prefill_paged_varlen_window_sink_anyg_bf16_fp8", True, True, "varlen", True, True, False, True),
    Attn("fa2_decode_paged_multi_window_sink_anyg_bf16_fp8", True, True, "multi", True, True, True, True),
    Attn("fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16", True, False, "varlen", True, True, False, True, True),
    Attn("fa2_decode_paged_multi_window_sink_softcap_anyg_bf16", True, False, "multi", True, True, True, True, True),
    Attn("fa2_prefill_paged_varlen_window_sink_softcap_anyg_bf16_fp8", True, True, "varlen", True, True, False, True, True),
    Attn("fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8", True, True, "multi", True, True, True, True, True),
]
Append = collections.namedtuple("Append", "name bf16 fp8 varlen")
APPEND = [
    Append("kv_append_paged", False, False, False),
    Append("kv_append_paged_fp8", False, True, False),
    Append("kv_append_paged_varlen", False, False, True),
    Append("kv_append_paged_varlen_bf16", True, False, True),
    Append("kv_append_paged_varlen_bf16_fp8", True, True, True),
]
BY_NAME = {e.name: e for e in ATTN + APPEND}
ROPES = ("none", "half", "interleaved")
VARLEN_T = [7, 2]
WINDOW, SPLIT_WINDOW = 65, 5000  # the split case's window covers its 4096 keys: every live page is read, and the plan still splits
GROUP, ANYG = 4, 3               # Hq / Hkv of a case; the any-G entries take one that is no power of two, so their rows divide by G


def pkg():
    import cuda_learn_notes_amd
    return cuda_learn_notes_amd


def elem_type(e):
    return BF if e.bf16 else HALF


def pool_type(e):
    return F8 if e.fp8 else elem_type(e)


def aligned4(e):
    """The operands the entry's host check admits at 4-byte alignment, by the names used in the cases below."""
    if isinstance(e, Append):
        return ["bt", "sl"] + (["cu"] if e.varlen else []) + (["ks", "vs"] if e.fp8 else []) + ["rope_table"]
    return (["bt", "sl"] + (["cu"] if e.form == "varlen" else []) + (["ks", "vs"] if e.fp8 else []) + (["sinks"] if e.sink else [])
            + ([] if e.plan else ["lse"]))


def live_entries(bt, lens, page=PAGE):
    """The (b, i) of the table entries a kernel may follow."""
    Nmax = bt.shape[1] * page
    return [(b, i) for b in range(bt.shape[0]) for i in range(-(-min(max(int(lens[b]), 0), Nmax) // page))]


# ---------------------------------------------------------------------------------------------------- attention

@functools.lru_cache(maxsize=None)
def attn_case(name, D, T=1, split=False):
    """The CPU tensors of one small case, made once and never modified. split: B = 1, Hkv = 1, max_pages page = 16384, len 4096 (the plan of every
    decode entry splits it); else B = 2, Hkv = 2, Hq = 8, lengths [9 page + 3, 4 page + 5]: 15 live pages, the second sequence's table has a
    tail of dead entries. An any-G entry has G = 3 (Hq = 6, or 3 with split); a soft-cap entry has q x 4 under the scale and the cap of
    softcap_of(): a cap that acts."""
    e = BY_NAME[name]
    G = ANYG if e.anyg else GROUP
    B, Hkv, mp, lens = (1, 1, 1024, [4096]) if split else (2, 2, 12, [9 * PAGE + 3, 4 * PAGE + 5])
    Hq, dt = Hkv * G, elem_type(e)
    g = torch.Generator().manual_seed(len(name) + 7 * D + 131 * T + split)
    cu = None
    if e.form == "single":
        q = torch.randn(B, Hq, D, generator=g).to(dt)
    elif e.form == "varlen":
        Ts = [1] if split else VARLEN_T
        cu = [0]
        for t in Ts:
            cu.append(cu[-1] + t)
        q = torch.randn(cu[-1], Hq, D, generator=g).to(dt)
    else:
        q = torch.randn(B, T, Hq, D, generator=g).to(dt)
    if e.softcap:
        q = (q.float() * cr.Q_MUL).to(dt)  # a power of two: exact
    k, v = (torch.randn(B, Hkv, mp * PAGE, D, generator=g) for _ in range(2))
    ks = vs = None
    if e.fp8 and not e.bf16:
        ks, vs = cs.scales_for(Hkv, "k"), cs.scales_for(Hkv, "v")
        kp, vp, bt = f8.make_pool(f8.quantize(k, f8.per_head(ks)), f8.quantize(v, f8.per_head(vs)), PAGE, lens, seed=D)
    elif e.fp8:
        ks, vs = b8.scales(Hkv)
        kp, vp, bt = b8.quantize_pools(pr.make_pool(k.to(BF), v.to(BF), PAGE, lens, seed=D), ks, vs)
    else:
        kp, vp, bt = pr.make_pool(k.to(dt), v.to(dt), PAGE, lens, seed=D)
    W = (SPLIT_WINDOW if split else WINDOW) if e.window else None
    sinks = sr.sinks_mixed(Hq, min(W, lens[0])) if e.sink else None
    return dict(e=e, D=D, T=T, B=B, Hq=Hq, Hkv=Hkv, mp=mp, q=q, kp=kp, vp=vp, bt=bt, lens=lens, cu=cu, ks=ks, vs=vs, W=W, sinks=sinks)


def softcap_of(e, D):
    """(softmax_scale, softcap) every case of a soft-cap entry runs with: the sensitive pair of paged_softcap_reference, neither the default
    scale nor a cap that does nothing; () for every other entry."""
    return (cr.scale_for(D), cr.CAP) if e.softcap else ()


def to_dev(c, dev):
    """The device tensors of a case, by the operand names of aligned4()."""
    d = {n: c[n].to(dev) for n in ("q", "kp", "vp", "bt", "ks", "vs", "sinks", "k_new", "v_new", "rope_table") if c.get(n) is not None}
    d["sl"] = torch.tensor(list(c["lens"]), dtype=torch.int32, device=dev)
    if c.get("cu") is not None:
        d["cu"] = torch.tensor(list(c["cu"]), dtype=torch.int32, device=dev)
    return d


def outputs(d):
    """(o, lse) filled with NaN."""
    q = d["q"]
    return torch.full_like(q, float("nan")), torch.full(q.shape[:-1], float("nan"), dtype=torch.float32, device=q.device)


def plan_of(c, D=None):
    """(splits, chunk, workspace_bytes) of a decode entry for the case's shape."""
    e = c["e"]
    dims = (c["B"],) + ((c["T"],) if e.form == "multi" else ()) + (c["Hq"], c["Hkv"], c["mp"], PAGE, c["D"]) + ((c["W"],) if e.window else ())
    return getattr(pkg(), e.name + "_plan")(*dims)


def call(e, d, W, o, lse, workspace=None):
    a = [d["q"], d["kp"], d["vp"], d["bt"], d["sl"]]
    if e.form == "varlen":
        a.append(d["cu"])
    if e.fp8:
        a += [d["ks"], d["vs"]]
    if e.window:
        a.append(W)
    if e.sink:
        a.append(d["sinks"])
    if e.softcap:
        a += list(softcap_of(e, d["q"].shape[-1]))  # two floats, passed by value: no operand to align
    a += [o, lse]
    if e.plan:
        a.append(workspace)
    getattr(pkg(), e.name)(*a)


def run(e, d, W):
    """One call: (o, lse) on the device, synchronised."""
    o, lse = outputs(d)
    call(e, d, W, o, lse)
    torch.cuda.synchronize()
    return o, lse


def check_small(c, o, lse, what):
    """The result (CPU tensors) of the case on its own small pool against the family's fp64 reference, with the family's check and bound."""
    e, q, kp, vp, bt, lens = c["e"], c["q"], c["kp"], c["vp"], c["bt"], c["lens"]
    if e.softcap:
        scale, cap = softcap_of(e, c["D"])
        kw = dict(ks=c["ks"], vs=c["vs"]) if e.fp8 else {}
        if e.form == "varlen":
            ref = cr.prefill(q, kp, vp, bt, lens, c["cu"], c["W"], c["sinks"], scale, cap, **kw)
        else:
            ref = cr.decode(q, kp, vp, bt, lens, c["W"], c["sinks"], scale, cap, **kw)
        t_sink.check(o, lse, *ref, what)
    elif e.bf16:
        sinks = c["sinks"] if e.sink else torch.full((c["Hq"],), NEG_INF, dtype=torch.float32)
        if e.form == "varlen":
            ref = b8.prefill(q, kp, vp, bt, lens, c["cu"], c["ks"], c["vs"], c["W"], sinks) if e.fp8 else sr.prefill(q, kp, vp, bt, lens, c["cu"], c["W"], sinks)
        else:
            ref = b8.decode(q, kp, vp, bt, lens, c["ks"], c["vs"], c["W"], sinks) if e.fp8 else sr.decode(q, kp, vp, bt, lens, c["W"], sinks)
        t_sink.check(o, lse, *ref, what)
    elif e.fp8:
        if e.form == "single":
            t_dec8.check(o, lse, q, kp, vp, bt, lens, c["ks"], c["vs"], what)
        else:
            cs.Entry(e.form).check(o, lse, q, kp, vp, bt, lens, c["ks"], c["vs"], what)
    elif e.form == "varlen":
        t_var.check(o, lse, q, kp, vp, bt, lens, c["cu"], what)
    else:
        {"single": t_dec, "multi": t_multi, "prefill": t_pre}[e.form].check(o, lse, q, kp, vp, bt, lens, what)


# ---------------------------------------------------------------------------------------------------- append

APPEND_B, APPEND_T, APPEND_HKV, APPEND_HQ, APPEND_MP, MAX_POS = 4, 3, 2, 8, 6, 128
APPEND_VARLEN_T = [3, 5, 2, 4]
APPEND_LENS = [66, 67, 65, 66]  # every sequence's new tokens end in page 4 and begin in page 3 of its table: 8 pages receive rows
APPEND_P = 24                   # 20 live pages, three spare ones, the dead entries' page 23


def poison_bits(dtype):
    """What a poisoned element holds: NaN of the 2-byte types (as int16 bits), the e4m3 NaN byte."""
    return {HALF: 0x7E00, BF: 0x7FC0, F8: f8.NAN_BYTE}[dtype]


def poisoned(shape, dtype):
    if dtype == F8:
        return torch.full(shape, f8.NAN_BYTE, dtype=torch.uint8).view(F8)
    return torch.full(shape, poison_bits(dtype), dtype=torch.int16).view(dtype)


@functools.lru_cache(maxsize=None)
def append_case(name, D):
    """The CPU tensors of one append case: the pools start as poison, the table names 5 distinct pages per sequence and the dead page behind."""
    e = BY_NAME[name]
    dt = elem_type(e)
    g = torch.Generator().manual_seed(len(name) + 3 * D)
    Ts = APPEND_VARLEN_T if e.varlen else [APPEND_T] * APPEND_B
    lead = (sum(Ts),) if e.varlen else (APPEND_B, APPEND_T)
    cu = None
    if e.varlen:
        cu = [0]
        for t in Ts:
            cu.append(cu[-1] + t)
    k_new, v_new = (torch.randn(*lead, APPEND_HKV, D, generator=g).to(dt) for _ in range(2))
    q = torch.randn(*lead, APPEND_HQ, D, generator=g).to(dt)
    bt = torch.full((APPEND_B, APPEND_MP), APPEND_P - 1, dtype=torch.int32)
    slots = torch.randperm(APPEND_P - 1, generator=g).tolist()
    for j, (b, i) in enumerate(live_entries(bt, APPEND_LENS)):
        bt[b, i] = slots[j]
    ks = vs = None
    if e.fp8:
        ks, vs = b8.scales(APPEND_HKV) if e.bf16 else (cs.scales_for(APPEND_HKV, "k"), cs.scales_for(APPEND_HKV, "v"))
    receivers = sorted({(b, (APPEND_LENS[b] - Ts[b] + t) // PAGE) for b in range(APPEND_B) for t in range(Ts[b])})
    kp = poisoned((APPEND_P, APPEND_HKV, PAGE, D), pool_type(e))
    return dict(e=e, D=D, k_new=k_new, v_new=v_new, q=q, bt=bt, lens=APPEND_LENS, cu=cu, ks=ks, vs=vs, kp=kp, vp=kp.clone(),
                rope_table=pkg().kv_append_rope_table(MAX_POS, D), receivers=receivers)


def call_append(e, d, rope, q_out):
    """rope "none" takes no q, q_out or rope_table; q_out: the output rows, or None."""
    a = [d["k_new"], d["v_new"], d["kp"], d["vp"], d["bt"], d["sl"]]
    if e.varlen:
        a.append(d["cu"])
    if e.fp8:
        a += [d["ks"], d["vs"]]
    if rope == "none":
        getattr(pkg(), e.name)(*a)
    else:
        getattr(pkg(), e.name)(*a, q=d["q"], q_out=q_out, rope_table=d["rope_table"], rope=rope)
