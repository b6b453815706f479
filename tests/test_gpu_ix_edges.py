"""GPU: GEMV, transpose, embedding, histogram and the SGEMM ladder on every dispatch cell, with exact answers -- at the shapes tests/ix_reference.py
lists (tests/test_ix_reference.py proves that those reach every cell of the launchers' dispatch, and that the integer inputs stay exact in fp32).
References are int64 / fp64 / bit patterns; outputs sit between sentinel guard bands, inputs are followed by NaN guards (index and histogram
inputs: by sentinel words / by a valid bin, so that an over-read would be counted), and every guard is checked after every call.

Run with `-s` every test prints `family case  error / bound = ratio` (bit-exact checks: the number of differing elements / 0).

NOT covered, and why:
* `mat_transpose_f32_diagonal2d` takes sqrtf of its block count; the count reaches 2^24 (where a float no longer holds it) only from 4 G elements
  (16 GB per tensor) on -- out of reach of a test that has to run in seconds.
* `sgemm_dma::launch` refuses shapes whose per-lane source offset would not fit 32 bits (BM * K * 4 or 16 * N * 4 bytes above 4 GB): the smallest
  such call needs K > 4 M columns or N > 67 M, operands of tens of GB.
* unaligned views (a tensor with a storage offset that is no multiple of 16 bytes): the packed rungs refuse them on the host; a launcher that let
  one through would fault the device, and a fault on purpose is not something a test may try on a shared machine.
* the vendor rows (`sgemm_cublas*`): rocBLAS's rounding order is not ours to hold to exact answers."""
import pytest
import torch

import ix_reference as ix

pytestmark = pytest.mark.gpu

WORST = {}


def note(family, case, err, bound, ratio=None):
    ratio = (err / bound if bound else float("inf") if err else 0.0) if ratio is None else ratio
    print("%-10s %-86s %.3e / %.3e = %.3f" % (family, case, err, bound, ratio))
    if ratio >= WORST.get(family, (-1.0, ""))[0]:
        WORST[family] = (ratio, case)
    return ratio


def dt(name):
    return getattr(torch, name)


@pytest.fixture(scope="module")
def lib(built, dev):
    return built.load("sgemv", "hgemv", "mat_transpose", "embedding", "histogram", "sgemm")


def gin(x, dev, fill="nan"):
    """x (CPU or device tensor) on the device inside guards; (view of x's shape, buffer)."""
    v, buf = ix.guarded(x.numel(), x.dtype, dev, fill)
    v.copy_(x.reshape(-1))
    return v.view(x.shape), buf


def gout(shape, dtype, dev):
    n = 1
    for s in shape:
        n *= s
    v, buf = ix.guarded(n, dtype, dev, "sentinel")
    return v.view(shape), buf, n


def mismatches(got, want):
    return int((got != want).sum())


# ================================================================== GEMV
def gemv_call(lib, dev, name, a_dev, x_dev, M, K):
    """One guarded call on the first M rows of a_dev; returns y on the CPU as a flat tensor, after the guard checks."""
    dtype = a_dev.dtype
    a, abuf = gin(a_dev[:M], dev)
    x, xbuf = gin(x_dev.view(K, 1), dev)
    y, ybuf, _ = gout((M, 1), dtype, dev)
    getattr(lib, name)(a, x, y)
    torch.cuda.synchronize()
    assert ix.guards_intact(ybuf, M, dtype, "sentinel"), (name, M, K)
    assert ix.guards_intact(abuf, M * K, dtype, "nan") and ix.guards_intact(xbuf, K, dtype, "nan"), (name, M, K)
    assert not ix.untouched(y, "sentinel") or M == 0
    return y.cpu().view(-1)


@pytest.mark.parametrize("name", list(ix.GEMV_RUNGS))
def test_gemv_integers_bit_exact(lib, dev, name):
    """Integers in [-4, 4]: fp32 must return the int64 product, fp16 that product rounded once to half."""
    dtype = dt(ix.GEMV_RUNGS[name][0])
    for K in ix.gemv_Ks(name):
        a8, x8 = ix.gemv_exact_inputs(max(ix.GEMV_M), K, K)
        ref = ix.int_matvec(a8, x8)
        want = ref.float() if dtype == torch.float32 else ref.double().to(torch.float16)
        a_dev, x_dev = a8.to(dev).to(dtype), x8.to(dev).to(dtype)
        for M in ix.GEMV_M:
            c = ix.gemv_cell(name, M, K)
            got = gemv_call(lib, dev, name, a_dev, x_dev, M, K)
            bad = mismatches(got, want[:M])
            note("gemv", "%s M=%d K=%d %s unrolled=%d rem=%d last_rows=%d/%d (integers)" % (name, M, K, c["form"], c["unrolled"], c["rem"], c["last_rows"], c["rpb"]), bad, 0)
            assert torch.equal(got, want[:M]), (name, M, K, c)


GEMV_IMPULSE_M = (37, 4097, 16387)


@pytest.mark.parametrize("name", list(ix.GEMV_RUNGS))
def test_gemv_row_impulse(lib, dev, name):
    """a[m, m % K] = 1, x distinct small integers: y[m] == x[m % K]."""
    dtype = dt(ix.GEMV_RUNGS[name][0])
    for K in ix.gemv_Ks(name):
        Mx = max(GEMV_IMPULSE_M)
        a_dev = torch.zeros(Mx, K, dtype=dtype, device=dev)
        a_dev[torch.arange(Mx, device=dev), torch.arange(Mx, device=dev) % K] = 1
        x = (torch.arange(K) - K // 2).to(dtype)  # |x| <= 1152: exact in half
        for M in GEMV_IMPULSE_M:
            got = gemv_call(lib, dev, name, a_dev, x.to(dev), M, K)
            want = x[torch.arange(M) % K]
            note("gemv", "%s M=%d K=%d %s (row impulse)" % (name, M, K, ix.gemv_cell(name, M, K)["form"]), mismatches(got, want), 0)
            assert torch.equal(got, want), (name, M, K)


@pytest.mark.parametrize("name", list(ix.GEMV_RUNGS))
def test_gemv_x_impulse(lib, dev, name):
    """x = e_k0, a ordinary randn: y == a[:, k0] bit for bit, for k0 on every edge of the row walk."""
    dtype = dt(ix.GEMV_RUNGS[name][0])
    for K in ix.gemv_Ks(name):
        Mx = max(GEMV_IMPULSE_M)
        a_dev = torch.randn(Mx, K, generator=torch.Generator(device=dev).manual_seed(K), device=dev).to(dtype)
        a_cpu = a_dev.cpu()
        for M in GEMV_IMPULSE_M:
            c = ix.gemv_cell(name, M, K)
            k0s, bad, bits = ix.gemv_impulse_k0(c, K), 0, (torch.int32 if dtype == torch.float32 else torch.int16)
            for k0 in k0s:
                x = torch.zeros(K, dtype=dtype, device=dev)
                x[k0] = 1
                got = gemv_call(lib, dev, name, a_dev, x, M, K)
                bad_k = mismatches(got.view(bits), a_cpu[:M, k0].contiguous().view(bits))
                assert bad_k == 0, (name, M, K, k0, c)
                bad += bad_k
            note("gemv", "%s M=%d K=%d %s k0=%s (x impulse)" % (name, M, K, c["form"], k0s), bad, 0)


@pytest.mark.parametrize("name", list(ix.GEMV_RUNGS))
def test_gemv_random_against_fp64(lib, dev, oracle, name):
    """randn operands against the fp64 oracle: sgemv by its existing rule, hgemv by that rule composed with the one rounding to half."""
    dtype = dt(ix.GEMV_RUNGS[name][0])
    Ks = ix.gemv_Ks(name)
    for K in sorted({Ks[0], Ks[len(Ks) // 2], Ks[-1]}):
        g = torch.Generator().manual_seed(K + 1)
        a, x = torch.randn(max(GEMV_IMPULSE_M), K, generator=g).to(dtype), torch.randn(K, generator=g).to(dtype)
        ref_full = oracle.gemv(a, x.view(K, 1)).view(-1)
        a_dev, x_dev = a.to(dev), x.to(dev)
        for M in GEMV_IMPULSE_M:
            got = gemv_call(lib, dev, name, a_dev, x_dev, M, K).double()
            ref = ref_full[:M]
            bound = ix.sgemv_bound(ref, K) if dtype == torch.float32 else ix.hgemv_bound(ref, K)
            ratio = (got - ref).abs() / bound
            i = int(ratio.argmax())
            r = note("gemv", "%s M=%d K=%d %s (randn)" % (name, M, K, ix.gemv_cell(name, M, K)["form"]), float((got - ref).abs()[i]), float(bound[i]))
            assert r <= 1.0 and bool(torch.isfinite(got).all()), (name, M, K, i, float(got[i]), float(ref[i]))


# ================================================================== transpose
@pytest.mark.parametrize("name", list(ix.TR_RUNGS))
def test_transpose_every_cell_bit_exact(lib, dev, name):
    ok, refused = ix.tr_shapes(name)
    for (r, c) in ok:
        cell = ix.tr_cell(name, r, c)
        x = ix.distinct_f32(r * c, r + c).view(r, c)
        xd, xbuf = gin(x, dev)
        y, ybuf, n = gout((c, r), torch.float32, dev)
        getattr(lib, name)(xd, y)
        torch.cuda.synchronize()
        want = xd.t().contiguous()
        bad = mismatches(y, want)
        note("transpose", "%s (%d, %d) %s grid=%d multi=%d perm=%d tail=%d" % (name, r, c, cell["kernel"], cell["grid"], cell["multi"], cell["perm"], cell["tail"]), bad, 0)
        assert torch.equal(y, want), (name, r, c, cell)
        if n <= 1 << 16:
            assert torch.equal(y.cpu(), x.t().contiguous())  # torch's device transpose, held to the CPU's
        assert ix.guards_intact(ybuf, n, torch.float32, "sentinel") and ix.guards_intact(xbuf, n, torch.float32, "nan"), (name, r, c)
    for (r, c) in refused:
        xd, xbuf = gin(ix.distinct_f32(r * c, 1).view(r, c), dev)
        y, ybuf, n = gout((c, r), torch.float32, dev)
        with pytest.raises(RuntimeError, match="multiples of"):
            getattr(lib, name)(xd, y)
        torch.cuda.synchronize()
        assert ix.untouched(y, "sentinel") and ix.guards_intact(ybuf, n, torch.float32, "sentinel"), (name, r, c)


# ================================================================== embedding
def emb_run(lib, dev, name, n, emb, vocab, seed, pin_rows=None):
    dname, VEC = ix.EMB_RUNGS[name]
    dtype, idt = dt(dname), (torch.int32 if dname == "float32" else torch.int16)
    cell = ix.emb_cell(name, n, emb)
    tb = ix.emb_table_bits(vocab, emb, dname, seed)
    idx = ix.emb_indices(n, vocab, seed + n)
    w, wbuf = ix.guarded(vocab * emb, dtype, dev, "nan")
    w.view(idt).copy_(tb.reshape(-1))
    i_d, ibuf = gin(idx, dev, "sentinel")
    o, obuf, total = gout((n, emb), dtype, dev)
    getattr(lib, name)(i_d, w.view(vocab, emb), o)
    torch.cuda.synchronize()
    tb_d = w.view(idt).view(vocab, emb)
    if pin_rows is None:
        want = ix.emb_reference_bits(idx, tb).to(dev)
    else:  # large outputs: torch's gather on the device, held to the CPU reference on sampled rows
        il = i_d.long()
        okd = (il >= 0) & (il < vocab)
        want = tb_d[il.clamp(0, vocab - 1)]
        want[~okd] = 0
        rows = torch.tensor(pin_rows)
        assert torch.equal(want[rows.to(dev)].cpu(), ix.emb_reference_bits(idx[rows], tb))
    got = o.view(idt)
    bad = mismatches(got, want)
    note("embedding", "%s n=%d emb=%d vocab=%d KP=%d nt=%d grid=%d partial=%d" % (name, n, emb, vocab, cell["KP"], cell["nt"], cell["grid"], cell["partial"]), bad, 0)
    assert torch.equal(got, want), (name, n, emb, cell)
    il = idx.long()
    oob = ((il < 0) | (il >= vocab)).to(dev)
    if bool(oob.any()):
        assert bool((got[oob] == 0).all()), (name, n, emb)  # all-zero BITS (not -0, not a flushed value)
    assert ix.guards_intact(obuf, total, dtype, "sentinel"), (name, n, emb)
    assert ix.guards_intact(wbuf, vocab * emb, dtype, "nan") and ix.guards_intact(ibuf, n, torch.int32, "sentinel")
    return cell


@pytest.mark.parametrize("name", list(ix.EMB_RUNGS))
def test_embedding_small_shapes_bit_patterns_and_out_of_range_rows(lib, dev, name):
    for n, emb, vocab in ix.emb_small_cases(name):
        emb_run(lib, dev, name, n, emb, vocab, 3)


@pytest.mark.parametrize("name", list(ix.EMB_RUNGS))
def test_embedding_traffic_cells(lib, dev, name):
    """256 MB and 512 MB of traffic on a small table: non-temporal stores, one pack per lane on the 16-byte rungs, whole and partial last workgroup,
    out-of-range rows among the valid ones."""
    wide = ix.EMB_RUNGS[name][1] * (4 if ix.EMB_RUNGS[name][0] == "float32" else 2) >= 16
    seen = set()
    for n, emb, vocab in ix.emb_traffic_cases(name):
        cell = emb_run(lib, dev, name, n, emb, vocab, 5, pin_rows=[0, 1, 2, 8, 9, 15, 16, 22, n // 2, n - 3, n - 2, n - 1])
        seen.add((cell["KP"], cell["nt"], cell["partial"]))
    assert seen == ({(4, True, False), (4, True, True), (1, True, False), (1, True, True)} if wide else {(4, True, False), (4, True, True)})


def test_embedding_refuses_a_row_that_is_no_multiple_of_the_pack(lib, dev):
    w, _ = gin(torch.zeros(4, 12, dtype=torch.float16), dev)
    i_d, _ = gin(torch.zeros(3, dtype=torch.int32), dev, "sentinel")
    o, obuf, n = gout((3, 12), torch.float16, dev)
    with pytest.raises(RuntimeError, match="multiple of the pack width"):
        lib.embedding_f16x8_pack(i_d, w, o)
    assert ix.untouched(o, "sentinel")


# ================================================================== histogram
def hist_input(v, dev):
    """v on the device with 64 words of bin 0 in front and behind: an over-read would be counted. (view, buffer)"""
    g = 64
    buf = torch.zeros(g + v.numel() + g, dtype=torch.int32, device=dev)
    buf[g:g + v.numel()] = v.to(dev)
    return buf[g:g + v.numel()], buf


@pytest.mark.parametrize("nbins", [8192, 8193])
@pytest.mark.parametrize("name", list(ix.HIST_RUNGS))
def test_histogram_out_of_range_short_inputs_and_loop_edges(built, dev, name, nbins):
    """The raw symbol, so that y is ours: values outside [0, nbins) are ignored, the band past nbins stays untouched, n = 0 touches nothing; every
    case twice (atomics)."""
    from cuda_learn_notes_amd import _loader
    fn = _loader.symbol(name)
    stream = torch.cuda.current_stream().cuda_stream
    sizes = ix.hist_sizes(name)
    v_full = ix.hist_values(max(sizes), nbins, nbins + len(name))
    for n in [0] + sizes:
        cell = ix.hist_cell(name, n, nbins)
        v = v_full[:n]
        a, abuf = hist_input(v, dev)
        ref = ix.hist_reference(v, nbins)
        y, ybuf, _ = gout((nbins,), torch.int32, dev)
        for rep in range(2):
            if n:
                y.zero_()
            rc = fn(a.data_ptr() if n else abuf.data_ptr() + 256, y.data_ptr(), n, nbins, stream)
            torch.cuda.synchronize()
            assert rc == 0, (name, n, nbins, rc)
            assert ix.guards_intact(ybuf, nbins, torch.int32, "sentinel"), (name, n, nbins)
            if n == 0:
                assert ix.untouched(y, "sentinel")
                continue
            got = y.cpu().long()
            bad = mismatches(got, ref)
            if rep == 0:
                note("histogram", "%s n=%d nbins=%d %s grid=%d unrolled=%d single=%d tail=%d valid=%d" % (name, n, nbins, cell["kernel"], cell["grid"], cell["unrolled"], cell["single"], cell["tail"], int(ref.sum())), bad, 0)
            assert torch.equal(got, ref), (name, n, nbins, rep, cell)
        assert int(abuf[:64].abs().sum()) == 0 and int(abuf[64 + n:].abs().sum()) == 0


# ================================================================== SGEMM
def sgemm_call(lib, dev, name, a, b, M, N, prefill, *knobs):
    ad, abuf = gin(a, dev)
    bd, bbuf = gin(b, dev)
    c, cbuf, n = gout((M, N), torch.float32, dev)
    if prefill is not None:
        c.fill_(prefill)
    getattr(lib, name)(ad, bd, c, *knobs)
    torch.cuda.synchronize()
    assert ix.guards_intact(cbuf, n, torch.float32, "sentinel"), (name, M, N)
    assert ix.guards_intact(abuf, a.numel(), torch.float32, "nan") and ix.guards_intact(bbuf, b.numel(), torch.float32, "nan"), (name, M, N)
    return c


@pytest.mark.parametrize("tile", list(ix.SGEMM_TILE_SHAPES))
def test_sgemm_matrix_core_every_tile_form_one_to_seven_stages_exact(built, lib, dev, tile):
    M, N = ix.SGEMM_TILE_SHAPES[tile]
    rows = torch.tensor(sorted({0, 1, 31, 32, 63, 64, M // 2 - 1, M // 2, M - 65, M - 1}))
    for K in ix.SGEMM_STAGE_KS:
        assert ix.sgemm_form(built.manifest.describe(ix.MFMA_NAMES[0], (M, N, K), 2)) == (tile, False)
        a, b = ix.sgemm_exact_inputs(M, N, K, K + M, device=dev)
        want = (a.double() @ b.double()).float()
        assert torch.equal(want[rows.to(dev)].cpu().long(), a[rows.to(dev)].cpu().long() @ b.cpu().long())  # the device's fp64 product, held to int64
        for name in ix.MFMA_NAMES:
            for stages, swz in ((2, False), (3, True)):
                c = sgemm_call(lib, dev, name, a, b, M, N, float("nan"), stages, swz, 256)
                bad = mismatches(c, want)
                note("sgemm", "%s (%d, %d, %d) %s stages=%d swizzle=%d" % (name[-12:], M, N, K, tile, stages, swz), bad, 0)
                assert torch.equal(c, want), (name, M, N, K, stages, swz)
                del c


def test_sgemm_k_split_every_ring_remainder_exact(built, lib, dev):
    """Halves 16+16 ... 19+18: every remainder modulo the three-slot ring in each half; C pre-filled with NaN, four times each."""
    M, N = ix.SGEMM_KSPLIT_SHAPE
    for K in ix.SGEMM_KSPLIT_KS:
        assert ix.sgemm_form(built.manifest.describe(ix.MFMA_NAMES[0], (M, N, K), 2)) == ("64x128", True)
        a, b = ix.sgemm_exact_inputs(M, N, K, K)
        want = (a.long() @ b.long()).float().to(dev)
        for name in ix.MFMA_NAMES:
            for stages in (2, 3):
                for swz in (False, True):
                    for rep in range(4):
                        c = sgemm_call(lib, dev, name, a, b, M, N, float("nan"), stages, swz, 256)
                        bad = mismatches(c, want)
                        if rep == 0:
                            note("sgemm", "%s (%d, %d, %d) K split %d+%d stages=%d swizzle=%d" % ((name[-12:], M, N, K) + ix.ksplit_halves(K) + (stages, swz)), bad, 0)
                        assert torch.equal(c, want), (name, K, stages, swz, rep)


@pytest.mark.parametrize("M,N,K,split", [(192, 256, 48, False), (128, 256, 544, True)])
def test_sgemm_k_impulse_on_the_64x128_forms(built, lib, dev, M, N, K, split):
    """A[:, k0] = 1, B randn: every row of C is B[k0, :] bit for bit."""
    assert ix.sgemm_form(built.manifest.describe(ix.MFMA_NAMES[0], (M, N, K), 2)) == ("64x128", split)
    b = torch.randn(K, N, generator=torch.Generator().manual_seed(K))
    for k0 in ix.sgemm_impulse_k0(K, split):
        a = torch.zeros(M, K)
        a[:, k0] = 1
        for name in ix.MFMA_NAMES:
            c = sgemm_call(lib, dev, name, a, b, M, N, float("nan"), 2, k0 & 1, 256)
            want = b[k0].to(dev).view(1, N).expand(M, N)
            bad = mismatches(c.view(torch.int32), want.contiguous().view(torch.int32))
            note("sgemm", "%s (%d, %d, %d) split=%d k0=%d (K impulse)" % (name[-12:], M, N, K, split, k0), bad, 0)
            assert bad == 0, (name, K, k0)


@pytest.mark.parametrize("name", list(ix.VALU_RUNGS))
def test_sgemm_valu_ladder_one_to_five_k_tiles_exact(lib, dev, name):
    BK, TN = ix.VALU_RUNGS[name]
    for (M, N, K) in ix.valu_cases(name):
        a, b = ix.sgemm_exact_inputs(M, N, K, M + N + K)
        want = (a.long() @ b.long()).float().to(dev)
        c = sgemm_call(lib, dev, name, a, b, M, N, float("nan"))
        bad = mismatches(c, want)
        note("sgemm", "%s (%d, %d, %d) BK=%d TN=%d tiles=%d" % (name[6:], M, N, K, BK, TN, K // BK), bad, 0)
        assert torch.equal(c, want), (name, M, N, K)
    if BK == 16:
        a, b = ix.sgemm_exact_inputs(128, 16 * TN, 8, 1)
        ad, _ = gin(a, dev)
        bd, _ = gin(b, dev)
        c, cbuf, n = gout((128, 16 * TN), torch.float32, dev)
        with pytest.raises(RuntimeError, match="multiples of the block tile"):
            getattr(lib, name)(ad, bd, c)
        torch.cuda.synchronize()
        assert ix.untouched(c, "sentinel")


@pytest.mark.parametrize("name", ix.ANY_SHAPE_NAMES)
def test_sgemm_any_shape_names_on_ragged_shapes_exact(lib, dev, name):
    for (M, N, K) in ix.ANY_SHAPES:
        a, b = ix.sgemm_exact_inputs(M, N, K, M + K)
        want = (a.long() @ b.long()).float().to(dev)
        c = sgemm_call(lib, dev, name, a, b, M, N, float("nan"))
        bad = mismatches(c, want)
        note("sgemm", "%s (%d, %d, %d)" % (name, M, N, K), bad, 0)
        assert torch.equal(c, want), (name, M, N, K)


def test_zz_worst_ratio_per_family():
    for family, (ratio, case) in sorted(WORST.items()):
        print("WORST %-10s %.3f  %s" % (family, ratio, case))
