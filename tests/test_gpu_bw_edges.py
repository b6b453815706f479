"""GPU: the streaming and row kernels on every dispatch path, with exact answers where they exist -- elementwise add, the 42 activations, the 20
block_all_reduce_sum rungs, dot product, the softmax / layer-norm / rms-norm row kernels and rope, at the sizes tests/bw_reference.py chooses
(tests/test_bw_reference.py proves that those reach every cell of the launchers' dispatch). References are fp64 / int64 (the `oracle` module, or
formed here); tolerances are the existing rules of test_gpu_activation.py / test_gpu_bandwidth.py, copied in bw_reference.py. Outputs sit between
sentinel guard bands, inputs are followed by NaN (int8: 127) guards.

Run with `-s` every test prints `family case  error / bound = ratio`.

NOT covered: the wave-per-row branches (`rpw > 1`) of the row kernels. `rows_per_wg` returns 1 from every C-ABI entry point
(ROWS_PER_WG_DEFAULT = 1, no caller passes another value), so no public call reaches them; test_bw_reference.py holds that statement against the
sources.

Figures where an existing rule did not hold (second rule of the file's issue: emulate the kernel's fp32 arithmetic on the CPU, allow twice its error):
layer-norm fp32 on x = 1000 + N(0, 1) -- see test_layer_norm_mean_far_above_spread."""
import pytest
import torch

import bw_reference as bw

pytestmark = pytest.mark.gpu

WORST = {}


def note(family, case, err, bound, ratio=None):
    ratio = (err / bound if bound else float("inf") if err else 0.0) if ratio is None else ratio
    print("%-12s %-70s %.3e / %.3e = %.3f" % (family, case, err, bound, ratio))
    if ratio >= WORST.get(family, (-1.0, ""))[0]:
        WORST[family] = (ratio, case)
    return ratio


def seeded(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def dt(name):
    return getattr(torch, name)


@pytest.fixture(scope="module")
def lib(built, dev):
    return built.load("elementwise", "activation", "reduce", "dot_product", "softmax", "layer_norm", "rms_norm", "rope")


def guarded_input(x, dev):
    """x (a CPU tensor) on the device inside NaN guards."""
    v, buf = bw.guarded(x.numel(), x.dtype, dev, "nan")
    v.copy_(x.reshape(-1))
    return v.view(x.shape), buf


def guarded_output(shape, dtype, dev):
    n = 1
    for s in shape:
        n *= s
    v, buf = bw.guarded(n, dtype, dev, "sentinel")
    return v.view(shape), buf, n


# ------------------------------------------------------------------ elementwise add
@pytest.mark.parametrize("rung", list(bw.ADD_RUNGS))
def test_add_every_kernel_and_partial_block(lib, dev, oracle, rung):
    dname, VEC, CHUNK = bw.ADD_RUNGS[rung]
    dtype = dt(dname)
    for n in bw.stream_sizes(bw.elem_bytes(dtype), VEC, CHUNK, "add"):
        cell = bw.stream_cell(n, bw.elem_bytes(dtype), VEC, CHUNK, "add")
        a, b = seeded(n % 997, n).to(dtype), seeded(n % 997 + 1, n).to(dtype)
        (ad, abuf), (bd, bbuf) = guarded_input(a, dev), guarded_input(b, dev)
        c, cbuf, _ = guarded_output((n,), dtype, dev)
        getattr(lib, "elementwise_add_" + rung)(ad, bd, c)
        torch.cuda.synchronize()
        ref = oracle.elementwise_add(a, b)
        bad = int((c.cpu().view(torch.uint8) != ref.view(torch.uint8)).sum())
        note("add", "%s n=%d %s K=%d grid=%d partial=%d tail=%d" % (rung, n, cell["kernel"], cell["K"], cell["grid"], cell["partial"], cell["tail"]), bad, 0)
        assert torch.equal(c.cpu(), ref), (rung, n)
        assert bw.guards_intact(cbuf, n, dtype, "sentinel"), (rung, n)
        assert bw.guards_intact(abuf, n, dtype, "nan") and bw.guards_intact(bbuf, n, dtype, "nan")


# ------------------------------------------------------------------ activations
def check_activation(lib, dev, oracle, op, rung, x, case, ref_to_dtype=False):
    dtype = x.dtype
    n = x.numel()
    xd, xbuf = guarded_input(x, dev)
    y, ybuf, _ = guarded_output((n,), dtype, dev)
    getattr(lib, "%s_%s" % (op, rung))(xd, y)
    torch.cuda.synchronize()
    got = y.cpu().double()
    ref = oracle.activation(op, x)
    if ref_to_dtype:  # what the output dtype cannot hold is compared after rounding the reference to it (inf where it overflows)
        ref = ref.to(dtype).double()
    assert bw.guards_intact(ybuf, n, dtype, "sentinel"), (op, rung, case)
    assert bw.guards_intact(xbuf, n, dtype, "nan")
    if op in ("relu", "hardshrink"):
        bad = int((got != ref).sum())
        note("activation", "%s_%s %s (bit-exact)" % (op, rung, case), bad, 0)
        assert torch.equal(got, ref), (op, rung, case)
        return
    rule = "activation_f32" if dtype == torch.float32 else "activation_f16"
    r, i = bw.excess(got, ref, rule)
    note("activation", "%s_%s %s worst at x=%.9g got=%.9g ref=%.9g" % (op, rung, case, x.flatten()[i].item(), got[i].item(), ref[i].item()), r, 1.0)
    assert r <= 1.0, (op, rung, case, x.flatten()[i].item(), got[i].item(), ref[i].item())
    assert torch.allclose(got, ref, rtol=bw.RULES[rule][0], atol=bw.RULES[rule][1], equal_nan=True)


@pytest.mark.parametrize("op", bw.ACT_OPS)
def test_activation_every_kernel_and_partial_block(lib, dev, oracle, op):
    for rung, (dname, VEC, CHUNK) in bw.UNARY_RUNGS.items():
        dtype = dt(dname)
        for n in bw.stream_sizes(bw.elem_bytes(dtype), VEC, CHUNK):
            cell = bw.stream_cell(n, bw.elem_bytes(dtype), VEC, CHUNK)
            x = seeded(bw.ACT_OPS.index(op) * 7 + n % 13, n) * 3.0
            x[:6] = torch.tensor([0.0, -0.0, 0.5, -0.5, 3.0, -3.0])
            x[-1] = -3.0  # the ragged tail's last element sits on a threshold
            check_activation(lib, dev, oracle, op, rung, x.to(dtype),
                             "n=%d %s K=%d grid=%d trips=%d partial=%d tail=%d" % (n, cell["kernel"], cell["K"], cell["grid"], cell["trips"], cell["partial"], cell["tail"]))


@pytest.mark.parametrize("op", bw.ACT_OPS)
def test_activation_range_sweep(lib, dev, oracle, op):
    """Every finite half value on the fp16 rungs; on the fp32 rungs magnitudes from 1e-30 to 3e38 in both signs, +-0 and the thresholds +-0.5, +-3,
    +-88.3762626647949 with their fp32 neighbours."""
    for rung, (dname, _, _) in bw.UNARY_RUNGS.items():
        x = bw.half_finite_values() if dname == "float16" else bw.f32_sweep_values()
        check_activation(lib, dev, oracle, op, rung, x, "sweep of %d values" % x.numel(), ref_to_dtype=True)


# ------------------------------------------------------------------ reduce
def bits_of_one(dtype):
    return torch.ones(1, dtype=dtype).view(bw.BITS[bw.elem_bytes(dtype)])[0].item()


@pytest.mark.parametrize("variant", list(bw.REDUCE_RUNGS))
def test_reduce_exact_sums(lib, dev, variant):
    dname, VEC = bw.REDUCE_RUNGS[variant]
    dtype = dt(dname)
    fn = getattr(lib, "block_all_reduce_sum_" + variant)
    for n in bw.reduce_sizes(bw.elem_bytes(dtype), VEC):
        cell = bw.reduce_cell(n, bw.elem_bytes(dtype), VEC)
        if dtype == torch.int8:  # the full range, as tests/test_gpu_bandwidth.py::test_reduce_i8_bit_exact
            x = torch.randint(-128, 128, (n,), generator=torch.Generator().manual_seed(n % 1000), dtype=torch.int8)
            exact = int(x.to(torch.int64).sum())
        else:
            x = bw.exact_sum_inputs(n, dtype, seed=n % 1000)
            exact = int(x.to(torch.float32).to(torch.int64).sum())
            assert int(x.to(torch.float32).abs().sum()) < 2 ** 24
        xd, xbuf = guarded_input(x, dev)
        y = fn(xd)
        got = y.item()
        note("reduce", "%s n=%d nfull=%d grid=%d owner=%d leftover=%d tail=%d got=%r exact=%d" %
             (variant, n, cell["nfull"], cell["grid"], cell["owner"], cell["leftover"], cell["tail"], got, exact), abs(got - exact), 0)
        assert y.dtype == (torch.int32 if dtype == torch.int8 else torch.float32) and y.numel() == 1
        assert got == exact, (variant, n, got, exact)
        assert bw.guards_intact(xbuf, n, dtype, "nan")


def impulse_positions(n, cell, VEC):
    nv, full = cell["nvec"] * VEC, cell["nfull"] * cell["chunk"] * VEC
    own0 = cell["owner"] * cell["chunk"] * VEC  # first element of the left-over owner's first whole chunk
    ps = {0, n - 1, nv - 1, nv, full - 1, full, own0, own0 + cell["chunk"] * VEC - 1, nv - 1}
    return sorted(p for p in ps if 0 <= p < n)


@pytest.mark.parametrize("variant", list(bw.REDUCE_RUNGS))
def test_reduce_impulse(lib, dev, variant):
    """A single 1 among zeros, at both ends, on both sides of the last whole pack and of the last whole chunk, and at the ends of the left-over
    owner's range: the sum is exactly 1 wherever the 1 sits (a dropped or doubled element gives 0 or 2)."""
    dname, VEC = bw.REDUCE_RUNGS[variant]
    dtype = dt(dname)
    eb = bw.elem_bytes(dtype)
    fn = getattr(lib, "block_all_reduce_sum_" + variant)
    for n in bw.reduce_sizes(eb, VEC)[-2:]:
        cell = bw.reduce_cell(n, eb, VEC)
        x, xbuf = bw.guarded(n, dtype, dev, "nan")
        xb = x.view(bw.BITS[eb])
        xb.zero_()
        ps = impulse_positions(n, cell, VEC)
        res = []
        for p in ps:
            xb[p] = bits_of_one(dtype)
            res.append(fn(x))
            xb[p] = 0
        got = torch.cat(res).cpu().tolist()
        wrong = [(p, g) for p, g in zip(ps, got) if g != 1]
        note("impulse", "%s n=%d positions=%s" % (variant, n, ps), len(wrong), 0)
        assert not wrong, (variant, n, wrong)
        assert fn(x).item() == 0


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_fp8_decode_every_code(lib, dev, fmt):
    """[c] -> half(table[c]) for every finite code, through the one-per-lane rung (a pack of one) and the x16 rung (the ragged tail's decode); a pack
    of sixteen copies through the x16 rung -> 16 * table[c] where that sum is exact in fp16."""
    table, nan, inf = bw.fp8_code_table(fmt)
    dtype = dt(bw.FP8[fmt])
    skip = set(bw.fp8_pack16_skip(fmt))
    one_rung = getattr(lib, "block_all_reduce_sum_fp8_%s_f16" % fmt)
    x16_rung = getattr(lib, "block_all_reduce_sum_fp8_%sx16_pack_f16" % fmt)
    codes = [c for c in range(256) if not nan[c] and not inf[c]]
    allc = torch.arange(256, dtype=torch.int32).to(torch.uint8).to(dev)
    packs = allc.view(256, 1).repeat(1, 16).contiguous()  # row c: sixteen copies of code c, 16-byte aligned
    r1, r16, rp = [], [], []
    for c in codes:
        r1.append(one_rung(allc[c:c + 1].view(dtype)))
        rp.append(x16_rung(packs[c].view(dtype)) if c not in skip else torch.zeros(1, device=dev))
    single = torch.empty(16, dtype=torch.uint8, device=dev)  # the x16 rung demands a 16-byte aligned pointer: one code at the front of its own buffer
    for c in codes:
        single[0] = c
        r16.append(x16_rung(single[:1].view(dtype)).clone())
    r1, r16, rp = (torch.cat(r).cpu().double() for r in (r1, r16, rp))
    want = table[codes].to(torch.float16).double()
    assert torch.equal(want, table[codes])
    bad1 = [(hex(c), g, w) for c, g, w in zip(codes, r1.tolist(), want.tolist()) if g != w]
    bad16 = [(hex(c), g, w) for c, g, w in zip(codes, r16.tolist(), want.tolist()) if g != w]
    badp = [(hex(c), g, 16 * w) for c, g, w in zip(codes, rp.tolist(), want.tolist()) if c not in skip and g != 16 * w]
    note("fp8", "%s single code, one-per-lane rung (%d codes)" % (fmt, len(codes)), len(bad1), 0)
    note("fp8", "%s single code, x16 rung" % fmt, len(bad16), 0)
    note("fp8", "%s pack of sixteen, x16 rung (%d codes skipped)" % (fmt, len(skip)), len(badp), 0)
    assert not bad1, bad1[:8]
    assert not bad16, bad16[:8]
    assert not badp, badp[:8]


# ------------------------------------------------------------------ dot product
@pytest.mark.parametrize("name", list(bw.DOT_RUNGS))
def test_dot_exact_and_impulse(lib, dev, name):
    dname, VEC = bw.DOT_RUNGS[name]
    dtype = dt(dname)
    eb = bw.elem_bytes(dtype)
    fn = getattr(lib, name)
    sizes = bw.reduce_sizes(eb, VEC, "dot")
    for n in sizes:
        cell = bw.reduce_cell(n, eb, VEC, "dot")
        a, b = bw.exact_sum_inputs(n, dtype, seed=n % 1000), bw.exact_sum_inputs(n, dtype, seed=n % 1000 + 1)
        exact = int((a.float().to(torch.int64) * b.float().to(torch.int64)).sum())
        (ad, abuf), (bd, bbuf) = guarded_input(a, dev), guarded_input(b, dev)
        got = fn(ad, bd).item()
        note("dot", "%s n=%d nfull=%d grid=%d owner=%d leftover=%d tail=%d got=%r exact=%d" %
             (name, n, cell["nfull"], cell["grid"], cell["owner"], cell["leftover"], cell["tail"], got, exact), abs(got - exact), 0)
        assert got == exact, (name, n, got, exact)
    for n in sizes[-2:]:  # a = one 1 among zeros, b[i] = i % 2039 + 1 (exact in fp16): the result names the position that was read
        cell = bw.reduce_cell(n, eb, VEC, "dot")
        a, abuf = bw.guarded(n, dtype, dev, "nan")
        ab = a.view(bw.BITS[eb])
        ab.zero_()
        w = (torch.arange(n) % 2039 + 1)
        bd, bbuf = guarded_input(w.to(dtype), dev)
        ps = impulse_positions(n, cell, VEC)
        res = []
        for p in ps:
            ab[p] = bits_of_one(dtype)
            res.append(fn(a, bd))
            ab[p] = 0
        got = torch.cat(res).cpu().tolist()
        wrong = [(p, g, int(w[p])) for p, g in zip(ps, got) if g != int(w[p])]
        note("dot", "%s impulse n=%d positions=%s" % (name, n, ps), len(wrong), 0)
        assert not wrong, (name, n, wrong)


# ------------------------------------------------------------------ row kernels
def row_call(lib, name, x, y, family):
    if family == "softmax":
        getattr(lib, name)(x, y)
    elif family == "layer_norm":
        getattr(lib, name)(x, y, LN_G, LN_B)
    else:
        getattr(lib, name)(x, y, RMS_G)


LN_G, LN_B, RMS_G = 1.5, -0.25, 0.75
ROW_FAMILIES = {"softmax": bw.SOFTMAX_RUNGS, "layer_norm": bw.LAYER_NORM_RUNGS, "rms_norm": bw.RMS_NORM_RUNGS}


def row_reference(oracle, family, x):
    if family == "softmax":
        return oracle.softmax_per_token(x)
    if family == "layer_norm":
        return oracle.layer_norm_kernel(x, LN_G, LN_B)
    return oracle.rms_norm_kernel(x, RMS_G)


def row_input(family, seed, S, K):  # the inputs of test_softmax_per_token / test_layer_norm / test_rms_norm
    x = seeded(seed, S, K)
    return x * 3.0 if family == "softmax" else (x * 2.0 + 0.5 if family == "layer_norm" else x * 2.0)


def run_row(lib, dev, family, name, x):
    """x (CPU, [S, K]) through rung `name`: (output on the CPU, guards intact)."""
    S, K = x.shape
    xd, xbuf = guarded_input(x, dev)
    y, ybuf, n = guarded_output((S, K), x.dtype, dev)
    row_call(lib, name, xd, y, family)
    torch.cuda.synchronize()
    return y.cpu(), bw.guards_intact(ybuf, n, x.dtype, "sentinel") and bw.guards_intact(xbuf, n, x.dtype, "nan")


@pytest.mark.parametrize("family", list(ROW_FAMILIES))
def test_row_kernels_every_cell(lib, dev, oracle, family):
    for name, spec in ROW_FAMILIES[family].items():
        dtype, VEC = dt(spec[0]), spec[1]
        rule = "%s_%s" % (family, "f32" if dtype == torch.float32 else "f16")
        for K in bw.row_Ks(VEC)[:-1]:
            for S in (1, 5):
                x = row_input(family, K % 1000 + S, S, K).to(dtype)
                got, intact = run_row(lib, dev, family, name, x)
                ref = row_reference(oracle, family, x)
                r, i = bw.excess(got.double(), ref.double(), rule)
                note(family, "%s S=%d K=%d cell=%s" % (name, S, K, bw.row_cell(K, VEC)), r, 1.0)
                assert intact, (name, S, K)
                assert r <= 1.0, (name, S, K, i, got.flatten()[i].item(), ref.flatten()[i].item())
                if family == "softmax":
                    assert torch.allclose(got.double().sum(dim=1), torch.ones(S, dtype=torch.float64), atol=1e-5 if dtype == torch.float32 else 2e-3)


@pytest.mark.parametrize("family", list(ROW_FAMILIES))
def test_row_kernels_refuse_the_first_unsupported_length(lib, dev, family):
    for name, spec in ROW_FAMILIES[family].items():
        dtype, VEC = dt(spec[0]), spec[1]
        K = bw.row_Ks(VEC)[-1]
        assert K == 8192 * VEC + VEC and bw.row_cell(K, VEC)[2] == "unsupported"
        x = torch.zeros(2, K, dtype=dtype, device=dev)
        y, ybuf, n = guarded_output((2, K), dtype, dev)
        with pytest.raises(RuntimeError, match="unsupported"):
            row_call(lib, name, x, y, family)
        torch.cuda.synchronize()
        assert bw.untouched(y.reshape(-1), "sentinel") and bw.guards_intact(ybuf, n, dtype, "sentinel"), name


def test_softmax_of_a_constant_row_is_one_over_K(lib, dev):
    """exp(0) = 1 in every position, the sum of K ones is exact, 1.0f / K is an IEEE division: float32(1 / K) everywhere, bit for bit (fp16 rungs:
    that value rounded to half, which is half(1 / K)). The unsafe rungs subtract no maximum: their constant is 0."""
    for name, (dname, VEC, mode) in bw.SOFTMAX_RUNGS.items():
        dtype = dt(dname)
        for K in bw.row_Ks(VEC)[:-1]:
            x = torch.full((3, K), 0.0 if mode == "unsafe" else 0.5, dtype=dtype)
            got, intact = run_row(lib, dev, "softmax", name, x)
            want = torch.tensor(1.0 / K, dtype=torch.float64).to(torch.float32).to(dtype)
            assert want.double().item() == torch.tensor(1.0 / K, dtype=torch.float64).to(dtype).double().item()
            bad = int((got.view(bw.BITS[bw.elem_bytes(dtype)]) != want.view(bw.BITS[bw.elem_bytes(dtype)])).sum())
            note("exact_rows", "softmax constant %s K=%d" % (name, K), bad, 0)
            assert intact and bad == 0, (name, K, got.flatten()[0].item(), want.item())


def test_rms_norm_exact_rows(lib, dev, oracle):
    for name, (dname, VEC) in bw.RMS_NORM_RUNGS.items():
        dtype = dt(dname)
        rule = "rms_norm_" + ("f32" if dtype == torch.float32 else "f16")
        for K in bw.row_Ks(VEC)[:-1]:
            sign = (torch.randint(0, 2, (K,), generator=torch.Generator().manual_seed(K)) * 2 - 1).to(dtype)
            x = torch.stack([torch.zeros(K, dtype=dtype), sign, -sign])
            got, intact = run_row(lib, dev, "rms_norm", name, x)
            assert intact, (name, K)
            assert bool((got[0].view(bw.BITS[bw.elem_bytes(dtype)]) == 0).all()), (name, K)  # +0 everywhere
            mag = got[1:].abs()
            assert mag.unique().numel() == 1, (name, K, mag.unique())                              # one magnitude, bit-identical
            assert torch.equal(got[1], mag[0] * sign) and torch.equal(got[2], -got[1])
            want = RMS_G / (1.0 + 1e-5) ** 0.5
            r, _ = bw.excess(mag.double(), torch.full_like(mag, want, dtype=torch.float64), rule)
            r2, _ = bw.excess(got.double(), oracle.rms_norm_kernel(x, RMS_G).double(), rule)
            note("exact_rows", "rms_norm zero / +-1 rows %s K=%d" % (name, K), max(r, r2), 1.0)
            assert r <= 1.0 and r2 <= 1.0, (name, K, mag[0, 0].item(), want)


def test_layer_norm_of_an_alternating_row(lib, dev, oracle):
    """x = +a, -a, +a, ... (a = 2, K even): the sum is exactly 0, every (x - mean)^2 is a^2 and their sum K a^2 is exact: two output values, one on
    the even positions and one on the odd, each bit-identical along the row, b +- g sqrt((K + 1e-5) / K) within the existing rule."""
    for name, (dname, VEC) in bw.LAYER_NORM_RUNGS.items():
        dtype = dt(dname)
        rule = "layer_norm_" + ("f32" if dtype == torch.float32 else "f16")
        for K in bw.row_Ks(VEC)[:-1]:
            assert K % 2 == 0
            row = torch.tensor([2.0, -2.0]).repeat(K // 2).to(dtype)
            x = torch.stack([row, -row])
            got, intact = run_row(lib, dev, "layer_norm", name, x)
            assert intact, (name, K)
            assert got[0, 0::2].unique().numel() == 1 and got[0, 1::2].unique().numel() == 1, (name, K)
            assert torch.equal(got[1, 0::2], got[0, 1::2]) and torch.equal(got[1, 1::2], got[0, 0::2])
            dev_ = LN_G * ((K + 1e-5) / K) ** 0.5
            want = torch.tensor([LN_B + dev_, LN_B - dev_], dtype=torch.float64).repeat(K // 2)
            r, _ = bw.excess(got[0].double(), want, rule)
            r2, _ = bw.excess(got.double(), oracle.layer_norm_kernel(x, LN_G, LN_B).double(), rule)
            note("exact_rows", "layer_norm alternating +-2 %s K=%d" % (name, K), max(r, r2), 1.0)
            assert r <= 1.0 and r2 <= 1.0, (name, K, got[0, :2].tolist(), want[:2].tolist())


def test_softmax_masked_rows(lib, dev, oracle):
    """Rows of masked logits through every rung: -inf at position 0, at the first position of lane 0's second pack, over the whole first wave's first
    packs, over the trailing third, everywhere but one position (one-hot), everywhere (NaN, as torch), with Gaussian neighbours on both sides of
    the all-masked row. Masked positions come out as exact zeros, the rest under the existing rule."""
    ninf = float("-inf")
    for name, (dname, VEC, mode) in bw.SOFTMAX_RUNGS.items():
        dtype = dt(dname)
        rule = "softmax_" + ("f32" if dtype == torch.float32 else "f16")
        Ks = bw.row_Ks(VEC)
        for K in (Ks[2], Ks[6], Ks[8], Ks[11]):  # one wave with 2 and with 5 packs per lane, two waves, 1024 lanes at the limit
            nt, mv, _ = bw.row_cell(K, VEC)
            assert mv >= 2 and nt * VEC < K
            x = seeded(K % 1000, 8, K) * 3.0
            x[0, 0] = ninf
            x[1, nt * VEC] = ninf
            x[2, :64 * VEC] = ninf
            x[3, K - K // 3:] = ninf
            hot = K // 3
            x[4, :] = ninf
            x[4, hot] = 0.0 if mode == "unsafe" else 1.5  # (the unsafe rungs form exp(x) / exp(x): exact only at exp(0) = 1)
            x[6, :] = ninf
            x = x.to(dtype)
            got, intact = run_row(lib, dev, "softmax", name, x)
            ref = oracle.softmax_per_token(x)
            assert intact, (name, K)
            masked = torch.isinf(x.float())
            worst = 0.0
            for row in (0, 1, 2, 3, 4, 5, 7):
                r, i = bw.excess(got[row].double(), ref[row].double(), rule)
                worst = max(worst, r)
                assert r <= 1.0, (name, K, "row", row, "col", i, got[row, i].item(), ref[row, i].item())
                assert bool((got[row][masked[row]] == 0).all()), (name, K, row)
            note("masked", "%s K=%d cell=%s rows 0-5,7" % (name, K, bw.row_cell(K, VEC)), worst, 1.0)
            onehot = torch.zeros(K, dtype=dtype)
            onehot[hot] = 1.0
            assert torch.equal(got[4], onehot), (name, K, got[4, hot].item())
            assert bool(torch.isnan(got[6].float()).all()) and bool(torch.isnan(ref[6].float()).all()), (name, K)


def test_layer_norm_mean_far_above_spread(lib, dev, oracle):
    """x = 1000 + N(0, 1), fp32: a one-pass E[x^2] - E[x]^2 variance would lose every digit here; the two-pass form does not. The existing rule
    (rtol 1e-5, atol 2e-5) is NOT met by any fp32 two-pass evaluation of this input: the fp32 sum of K values near 1000 carries an error of
    ~1e-4 K^0.5 ulp-steps, so the mean is off by ~1e-4 of the spread. Following the second rule of this file's issue the bound is twice the error of
    bw.emulate_layer_norm_f32 (the kernel's arithmetic in fp32 torch on the CPU) against the fp64 reference, where that exceeds the existing rule:
    measured on the CPU, the emulation sits at 3-8x the existing rule (K = 8192: 8.1x, max error 2e-4; K = 32768: 5.6x)."""
    for name in ("layer_norm_f32", "layer_norm_f32x4"):
        VEC = bw.LAYER_NORM_RUNGS[name][1]
        Ks = bw.row_Ks(VEC)
        for K in (Ks[6], Ks[9], Ks[11]):
            x = 1000.0 + seeded(K % 1000 + 3, 4, K)
            got, intact = run_row(lib, dev, "layer_norm", name, x)
            ref = oracle.layer_norm_kernel(x, LN_G, LN_B).double()
            r, i = bw.excess(got.double(), ref, "layer_norm_f32")
            r_emu, _ = bw.excess(bw.emulate_layer_norm_f32(x, LN_G, LN_B, VEC).double(), ref, "layer_norm_f32")
            allowed = max(1.0, 2.0 * r_emu)
            note("ln_offset", "%s K=%d existing-rule ratio %.3f, CPU fp32 emulation %.3f, allowed %.3f" % (name, K, r, r_emu, allowed), r, allowed)
            assert intact and r <= allowed, (name, K, r, r_emu)


# ------------------------------------------------------------------ rope
@pytest.mark.parametrize("name", list(bw.ROPE_RUNGS))
def test_rope_partial_column_block_and_ragged_rows(lib, dev, oracle, name):
    pairs = bw.ROPE_RUNGS[name]
    for S, hidden in bw.rope_shapes(pairs):
        gx, gy, units = bw.rope_grid(S, hidden, pairs)
        assert gx == 2 and units % 256 and S % gy and S % 4
        x = seeded(S + hidden, S, hidden)
        ref = oracle.rope_torch(x)
        bound = bw.rope_bound(x)
        xd, xbuf = guarded_input(x, dev)
        out, obuf, n = guarded_output((S, hidden), torch.float32, dev)
        getattr(lib, name)(xd, out)
        torch.cuda.synchronize()
        d = (out.cpu().double() - ref.double()).abs()
        note("rope", "%s S=%d hidden=%d grid=(%d, %d)" % (name, S, hidden, gx, gy), float((d / bound).max()), 1.0)
        assert bw.guards_intact(obuf, n, torch.float32, "sentinel") and bw.guards_intact(xbuf, n, torch.float32, "nan")
        assert bool((d <= bound).all()), (name, float((d - bound).max()))
        colmax = d.max(dim=0).values
        assert float((colmax <= bw.ROPE_RULE[0]).double().mean()) >= bw.ROPE_RULE[2], (name, float(colmax.max()))
        n_in, n_out = x.view(S, -1, 2).norm(dim=-1), out.cpu().view(S, -1, 2).norm(dim=-1)
        assert torch.allclose(n_in, n_out, atol=1e-4, rtol=1e-4)


def test_zz_worst_ratios():
    """Prints the worst error / bound ratio of each family above (run after them, in file order)."""
    for family, (ratio, case) in sorted(WORST.items()):
        print("WORST %-12s %.3f  %s" % (family, ratio, case))
