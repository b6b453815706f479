"""GPU: every HGEMM kernel family at the shapes tests/hgemm_reference.py lists (tests/test_hgemm_reference.py proves that the table reaches every
family csrc/hgemm.hip can name, and that the integer inputs stay exact in fp32 in every order and split), with answers that have no tolerance:

* exact: integer operands, C must equal the int64 product rounded once to half, ties to even (a share of the sums lies past 2048, where the half
  grid is coarser than the integers, and from K = 4096 on past 65520: +-inf);
* dependency: one NaN per chosen row of A / column of B at the edges of K tiles and of fragment / wave / block tiles -- C must be NaN exactly on
  those rows and columns and the exact answer everywhere else;
* special values: fp16 subnormal inputs and results, 65504, the tie 65520, +inf against a nonzero and against a zero;
* placement: A and B sit inside NaN guards at a base address that is an odd multiple of 16 bytes, C inside a sentinel guard band, pre-filled with the
  sentinel; every guard is checked after every call and no element of C may keep the sentinel;
* the scheduled kernels (ping-pong, hgemm_w4, hgemm_w4s, split-K, tail split) run the exact case three times, block swizzle alternating.

Run with `-s` every case prints one line, `family case  mismatches / 0` (the mismatches of all its launches together: exact, poison, special).

NOT covered, and why:
* the interleaved XCD walk (csrc/hgemm_mfma.cuh tile_coords_interleaved) needs A + B past 512 MB -- far outside a test of seconds;
  test_operands_past_the_infinity_cache_take_the_interleaved_walk (bit-equality to the un-swizzled launch) stays the check for it.
* views that are not 16-byte aligned: check_args refuses them on the host; a launcher that let one through would fault the device, and a fault on
  purpose is not something a test may try on a shared machine.
* split-K on the 256 x 256 tile in the one-launch (fix-up) form: splitk_plan never picks it for M, N up to 4608 and K up to 8256
  (test_hgemm_reference.py holds that), and the probe kinds that could force it allocate 512 MiB of their own.
* the vendor rows (`hgemm_cublas_tensor_op_*`): guard bands and the tolerance of tests/test_gpu_hgemm.py only -- rocBLAS's rounding is not ours to
  hold to exact answers.
The only instantiations left out are the rings that do not fit the 160 KiB LDS (the skips of test_every_ring_instantiation): the table does not
list them, and the last test of the module holds that every listed case ran."""
import pytest
import torch

import hgemm_reference as hr

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2 ** -10, 2e-3  # vendor rows only: the rule of tests/test_gpu_hgemm.py
RAN = set()
NAN = float("nan")


@pytest.fixture(scope="module")
def hg(built, dev):
    lib = built.hgemm_lib()
    lib.init_cublas_handle()
    yield lib
    lib.destroy_cublas_handle()


def note(family, cid, bad):
    print("%-11s %s  %d / 0" % (family, cid, bad))


def place(x, dev, fill):
    """x flat inside guards, its first element at an odd multiple of 16 bytes: (flat view, buffer, elements the buffer's payload holds)."""
    n = x.numel()
    v, buf = hr.guarded(n + 8, torch.float16, dev, fill)  # the payload starts 256-byte aligned: 8 halves further is 16-byte aligned and no more
    assert (v.data_ptr() // 16) % 2 == 0
    w = v[8:]
    assert w.data_ptr() % 16 == 0 and (w.data_ptr() // 16) % 2 == 1
    if x is not None and fill == "nan":
        w.copy_(x.reshape(-1))
    return w, (v, buf, n + 8)


def intact(guard, fill):
    v, buf, n = guard
    return hr.guards_intact(buf, n, torch.float16, fill) and hr.untouched(v[:8], fill)


def launch(case, hg, host, a, b, dev, swizzle):
    """One call of the case's entry on guarded operands; returns C (device) after the guard checks. a [M, K], b [K, N]: device halves."""
    M, N, K = case.M, case.N, case.K
    av, ag = place(a, dev, "nan")
    bv, bg = place(b.t() if case.layout else b, dev, "nan")  # TN: storage [N, K] under the shape [K, N] (bench_utils.as_col_major)
    cv, cg = place(torch.empty(M * N), dev, "sentinel")
    av, bv, cv = av.view(M, K), bv.view(K, N), cv.view(M, N)
    e = case.entry
    if e[0] in ("g3", "vendor"):
        getattr(hg, e[1])(av, bv, cv)
    elif e[0] == "g6":
        getattr(hg, e[1])(av, bv, cv, e[2], bool(swizzle), 2 * case.bn)
    else:
        host.hgemm_variant(e[1], case.layout, e[2], e[3], e[4], av, bv, cv, swizzle=int(swizzle), swizzle_stride=2 * case.bn)
    torch.cuda.synchronize()
    assert intact(cg, "sentinel"), ("C guard", case.cid)
    assert intact(ag, "nan") and intact(bg, "nan"), ("A / B guard", case.cid)
    left = int((cv.view(torch.int16) == cg[1][0]).sum())
    assert left == 0, ("elements of C left untouched", left, case.cid)
    return cv


def report(case, what, got, want):
    """Count and first position of mismatches (NaN compared by position); prints the case's line and raises if there are any."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    diff = (gn != wn) | (~gn & ~wn & (got != want))
    bad = int(diff.sum())
    if bad:
        note(case.family, case.cid + " " + what, bad)
        m, n = (int(i) for i in diff.nonzero()[0])
        raise AssertionError("%s %s: %d mismatches, first at (%d, %d): got %r want %r" % (case.cid, what, bad, m, n, float(got[m, n]), float(want[m, n])))


_REF = {}


def reference(case, dev, manifest):
    """(a, b device halves, expected half on the device) of the exact case; one per (M, N, K), shared by every case of that shape."""
    key = (case.M, case.N, case.K)
    if key in _REF:
        return _REF[key]
    a8, b8 = hr.exact_inputs(*key)
    ad, bd = a8.to(dev), b8.to(dev)
    if case.big:
        want = hr.expected_exact(ad, bd)  # float64 on the device: exact in any order for these integers
        seam = None
        if case.family == "tail":
            seam = hr.tail_m_split(manifest.describe(case.entry[1], key, 2))
        rows = hr.sample_rows(case.M, seam)
        pin = hr.half_rne(a8[rows].to(torch.int64) @ b8.to(torch.int64))
        assert torch.equal(want[rows].cpu().view(torch.int16), pin.view(torch.int16)), ("device float64 product off the int64 one", key)
    else:
        want = hr.expected_exact(a8, b8).to(dev)
    if len(_REF) >= 4:
        _REF.clear()
    _REF[key] = (ad.half(), bd.half(), want)
    return _REF[key]


def run_case(case, hg, host, dev, manifest):
    a, b, want = reference(case, dev, manifest)
    if case.family == "vendor":
        c = launch(case, hg, host, a, b, dev, 0)
        truth = a.double() @ b.double()
        bad = int(((c.double() - truth).abs() > ATOL + RTOL * truth.abs()).sum())
        note(case.family, case.cid + " (tolerance)", bad)
        assert bad == 0, case.cid
        RAN.add(case.cid)
        return
    # exact (the scheduled kernels three times, block swizzle alternating; every launch against the reference)
    for rep in range(3 if case.scheduled else 1):
        report(case, "exact#%d" % rep, launch(case, hg, host, a, b, dev, rep & 1), want)
    # dependency
    rows, cols = hr.poison_plan(case)
    ap, bp = a.clone(), b.clone()
    for m, k in rows:
        ap[m, k] = NAN
    for n, k in cols:
        bp[k, n] = NAN
    wantp = torch.where(hr.poison_mask(case).to(dev), torch.full_like(want, NAN), want)
    report(case, "poison", launch(case, hg, host, ap, bp, dev, 1), wantp)
    # special values
    if case.K >= 8:
        sa, sb, sw = hr.special_inputs(case)
        report(case, "special", launch(case, hg, host, sa.to(dev), sb.to(dev), dev, 0), sw.to(torch.float16).to(dev))
    note(case.family, case.cid, 0)
    RAN.add(case.cid)


def run_family(family, hg, built, dev, pick=None):
    from cuda_learn_notes_amd import host
    cases = hr.table(built.manifest)["cases"][family]
    if pick is not None:
        cases = [c for c in cases if pick(c)]
    assert cases, family
    for case in cases:
        run_case(case, hg, host, dev, built.manifest)


@pytest.mark.parametrize("family", ["valu", "naive_mfma", "1stage"] + hr.RING_FAMILIES + ["pingpong", "w4s", "vendor"])
def test_explicit_instantiations(hg, built, dev, family):
    run_family(family, hg, built, dev)


@pytest.mark.parametrize("tile", sorted(set("%dx%d" % t for t in list(hr.W4_KIND15.values()) + [(256, 256)])))
def test_one_wave_per_simd_tiles(hg, built, dev, tile):
    run_family("w4", hg, built, dev, lambda c: "%dx%d" % (c.bm, c.bn) == tile)


@pytest.mark.parametrize("fam", hr.DISPATCHED_FAMILIES)
def test_run_time_dispatched_names(hg, built, dev, fam):
    run_family("dispatched", hg, built, dev, lambda c: hr.expected_family(c, built.manifest) == fam)


@pytest.mark.parametrize("form", ["fixup", "reduce"])
@pytest.mark.parametrize("tile", hr.SPLITK_TILES)
def test_split_k(hg, built, dev, tile, form):
    if (tile, form) == ("256x256", "fixup"):
        assert not any(hr.expected_family(c, built.manifest) == "splitk<256x256>,fixup" for c in hr.table(built.manifest)["cases"]["splitk"])
        return  # the planner never picks it (module docstring); nothing to run, nothing skipped
    run_family("splitk", hg, built, dev, lambda c: hr.expected_family(c, built.manifest) == "splitk<%s>,%s" % (tile, form))


@pytest.mark.parametrize("layout", [hr.NN, hr.TN])
@pytest.mark.parametrize("form", ["fixup", "reduce"])
def test_tail_split(hg, built, dev, form, layout):
    run_family("tail", hg, built, dev, lambda c: c.layout == layout and hr.expected_family(c, built.manifest) == "tail_split,%s" % form)


def test_refused_shapes_raise_and_write_nothing(hg, built, dev):
    from cuda_learn_notes_amd import host
    for r in hr.table(built.manifest)["refused"]:
        M, N, K = r.M, r.N, r.K
        av, ag = place(torch.ones(M * K, dtype=torch.float16), dev, "nan")
        bv, bg = place(torch.ones(K * N, dtype=torch.float16), dev, "nan")
        cv, cg = place(torch.empty(M * N), dev, "sentinel")
        with pytest.raises(RuntimeError):
            if r.entry[0] == "g3":
                getattr(hg, r.entry[1])(av.view(M, K), bv.view(K, N), cv.view(M, N))
            else:
                host.hgemm_variant(r.entry[1], r.layout, r.entry[2], r.entry[3], r.entry[4], av.view(M, K), bv.view(K, N), cv.view(M, N), swizzle=0,
                                   swizzle_stride=1)
        torch.cuda.synchronize()
        assert intact(cg, "sentinel") and hr.untouched(cv, "sentinel"), r
        note(r.family, "%s %dx%dx%d refused" % (r.entry[1:], M, N, K), 0)


def test_every_case_of_the_table_ran(built, dev):
    """Nothing skipped: the rings that do not fit the LDS are not in the table (hr.table()["lds_skips"] names them), every other case ran."""
    tb = hr.table(built.manifest)
    every = {c.cid for cs in tb["cases"].values() for c in cs}
    assert len(every) == hr.case_count(built.manifest)  # (case ids are unique)
    missing = sorted(every - RAN)
    print("cases run %d of %d; ring instantiations outside the LDS budget: %d" % (len(RAN), len(every), len(tb["lds_skips"])))
    assert not missing, missing[:10]
