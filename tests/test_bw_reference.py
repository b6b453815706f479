"""CPU only: the helpers of tests/bw_reference.py, proven before they judge a kernel (tests/test_gpu_bw_edges.py) -- the dispatch mirrors against the
constants and expressions of the HIP sources, the shape choosers against the cells they must reach, broken copies of each mirror against those same
checks, the exact-sum inputs, the fp8 tables, the guard bands and the copied tolerance rules."""
import os
import re

import pytest
import torch

import bw_reference as bw

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cuda-learn-notes_amd", "csrc")

# (name suffix, elem bytes, VEC, CHUNK) of the six add / unary rungs; add's f16x8 rung runs the half2 kernel (VEC = CHUNK = 2)
UNARY_RUNGS = [("f32", 4, 1, 1), ("f32x4", 4, 4, 4), ("f16", 2, 1, 1), ("f16x2", 2, 2, 2), ("f16x8", 2, 8, 2), ("f16x8_pack", 2, 8, 8)]
ADD_RUNGS = [("f32", 4, 1, 1), ("f32x4", 4, 4, 4), ("f16", 2, 1, 1), ("f16x2", 2, 2, 2), ("f16x8", 2, 2, 2), ("f16x8_pack", 2, 8, 8)]
# (elem bytes, VEC) of the reduce rungs and of the dot rungs
REDUCE_RUNGS = [(4, 1), (4, 4), (2, 1), (2, 2), (2, 8), (1, 1), (1, 16)]
DOT_RUNGS = [(4, 1), (4, 4), (2, 1), (2, 2), (2, 8)]


def src(name):
    return open(os.path.join(CSRC, name)).read()


def one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) >= 1, pattern
    assert len(set(m)) == 1, (pattern, m)  # every occurrence (kernel and launcher) states the same thing
    return m[0]


# ---------------------------------------------------------------- constants
def test_row_constants_are_those_of_rowwise_cuh():
    s = src("rowwise.cuh")
    per_lane, wave_a, wave_b = re.search(r"int nt = \(\(\(nvec \+ \d+\) / (\d+) \+ \d+\) / (\d+)\) \* (\d+);", s).groups()
    assert int(per_lane) == bw.ROW_PACKS_PER_LANE and int(wave_a) == int(wave_b) == bw.WAVE
    assert re.search(r"int nt = \(\(\(nvec \+ %d\) / %d \+ %d\) / %d\) \* %d;" % (bw.ROW_PACKS_PER_LANE - 1, bw.ROW_PACKS_PER_LANE, bw.WAVE - 1, bw.WAVE, bw.WAVE), s)
    assert int(one(r"if \(nt > (\d+)\) nt = \d+;", s)) == bw.ROW_NT_CAP == int(one(r"if \(nt > \d+\) nt = (\d+);", s))
    assert int(one(r"if \(nt < (\d+)\) nt = \d+;", s)) == bw.WAVE
    assert "return (K / VEC + nt - 1) / nt; }" in s
    m = re.search(r"const int mv_ = \(vpt\) <= (\d) \? (\d) : \(vpt\) <= (\d) \? (\d) : \(vpt\) <= (\d) \? (\d) : (\d);", s)
    assert tuple(int(x) for x in m.groups()) == (1, 1, 2, 2, 4, 4, 8) and bw.ROW_MAXV == (1, 2, 4, 8)
    assert "if ((vpt) > %d) return CLN_ERR_UNSUPPORTED;" % bw.ROW_MAXV[-1] in s
    assert "const bool full_ = (long long)(K) == (long long)mv_ * (nt) * (VEC);" in s
    # one row per workgroup from every C-ABI entry point: the wave-per-row (rpw > 1) branches are unreachable, as the GPU file's docstring says
    assert "constexpr int ROWS_PER_WG_DEFAULT = 1;" in s
    for f in ("softmax.hip", "norm.hip"):
        assert set(re.findall(r"rpw = rows_per_wg\(([^)]*)\)", src(f))) <= {"nt, S", "nt, N"}  # no `want` argument anywhere


def test_stream_constants_are_those_of_the_launchers():
    kb_expr = r"constexpr int KB = AB >= 16 \? (\d+) : \((\d+) / AB > (\d+) \? (\d+) : (\d+) / AB\);"
    for f in ("elementwise.hip", "activation.hip"):
        s = src(f)
        wide, b0, mx0, mx1, b1 = (int(x) for x in one(kb_expr, s))
        assert (wide, b0, mx0, mx1, b1) == (bw.STREAM_KB_WIDE, bw.STREAM_KB_BYTES, bw.STREAM_KB_MAX, bw.STREAM_KB_MAX, bw.STREAM_KB_BYTES)
        assert int(one(r"nvec < (\d+) \* KB\)", s)) == bw.STREAM_K1_BLOCKS
        assert int(one(r"blockIdx\.x \* \((\d+) \* K\) \+ threadIdx\.x", s)) == bw.STREAM_NT
        assert int(one(r"base \+ \(K - 1\) \* (\d+) < nvec", s)) == bw.STREAM_NT
    assert int(one(r"traffic >= \((\d+)LL << 20\)\) \|\| nvec", src("elementwise.hip"))) << 20 == bw.STREAM_CAP_LIFT
    assert "const long long traffic = 3LL * n * (long long)sizeof(T);" in src("elementwise.hip")
    act = src("activation.hip")
    assert "nvec = n / CHUNK, traffic = 2LL * n * (long long)sizeof(T);" in act
    assert "const int grid = cln_stream_grid(n / VEC + 1, 256, traffic);" in act
    assert "const long long stride = (long long)gridDim.x * %d;" % bw.STREAM_NT in act
    c = src("common.h")
    assert int(one(r"#define CLN_STREAM_WGS_PER_CU (\d+)", c)) == bw.STREAM_WGS_PER_CU
    lift, cus = re.search(r"const long long cap = traffic_bytes >= \((\d+)LL << 20\) \? 0x7fffffffLL : (\d+)LL \* CLN_STREAM_WGS_PER_CU;", c).groups()
    assert int(lift) << 20 == bw.STREAM_CAP_LIFT and int(cus) == bw.STREAM_CUS


def test_reduce_and_dot_constants_are_those_of_the_sources():
    r = src("reduce.hip")
    nt, wg = re.search(r"constexpr int RED_NT = (\d+), RED_MAX_WG = (\d+),", r).groups()
    assert (int(nt), int(wg)) == (bw.RED_NT, bw.RED_MAX_WG)
    assert tuple(int(x) for x in one(r"constexpr int K = sizeof\(P\) >= 16 \? (\d) : (\d);", r)) == bw.RED_K
    assert tuple(int(x) for x in one(r"constexpr int K = sizeof\(E\) \* VEC >= 16 \? (\d) : (\d);", r)) == bw.RED_K
    assert "chunks < 1 ? 1 : (chunks > RED_MAX_WG ? RED_MAX_WG : chunks)" in r
    assert "if (blockIdx.x == (unsigned)(nfull % gridDim.x))" in r
    d = src("blas1.hip")
    assert tuple(int(x) for x in one(r"constexpr int K = sizeof\(P\) >= 16 \? (\d) : (\d);", d)) == bw.DOT_K
    assert tuple(int(x) for x in one(r"constexpr int K = sizeof\(T\) \* VEC >= 16 \? (\d) : (\d);", d)) == bw.DOT_K
    assert "chunk = %dLL * K, nfull = nvec / chunk;" % bw.RED_NT in d
    assert "chunks < 1 ? 1 : (chunks > %d ? %d : chunks)" % (bw.RED_MAX_WG, bw.RED_MAX_WG) in d
    assert "if (blockIdx.x == (unsigned)(nfull % gridDim.x))" in d
    assert int(one(r"SOFTMAX_ONE_BLOCK_MAX = (\d+);", src("softmax.hip"))) == bw.SOFTMAX_ONE_BLOCK_MAX


def test_rope_grid_is_that_of_the_launcher():
    s = src("rope.hip")
    cap, rows = re.search(r"constexpr int cap_wg = (\d+), min_rows = (\d+);", s).groups()
    assert (int(cap), int(rows)) == (bw.ROPE_CAP_WG, bw.ROPE_MIN_ROWS)
    assert "#pragma unroll %d" % bw.ROPE_MIN_ROWS in s and "const int gx = (half_hidden / PAIRS + 255) / 256;" in s
    for pairs in (1, 2):
        for S, hidden in bw.rope_shapes(pairs):
            gx, gy, units = bw.rope_grid(S, hidden, pairs)
            assert hidden % (2 * pairs) == 0 and units == 256 + 3 and gx == 2  # a partial second column block
            assert S % gy and S % bw.ROPE_MIN_ROWS and gy == (S + 3) // 4
    assert bw.rope_grid(8192, 8192, 2) == (8, 2048, 2048) and bw.rope_grid(3, 64, 1) == (1, 1, 32)


# ---------------------------------------------------------------- coverage of the shape choosers (and that broken mirrors fail them)
def check_row_coverage(row_cell, row_Ks, VEC):
    Ks = row_Ks(VEC)
    cells = {K: row_cell(K, VEC) for K in Ks}
    seen = set(cells.values())
    for mv in (1, 2, 4, 8):
        assert (64, mv, True) in seen and (64, mv, False) in seen, (VEC, mv)
    for full in (False, True):
        assert any(64 < nt < 1024 and f is full for nt, _, f in seen), (VEC, full)
        assert any(nt == 1024 and f is full for nt, _, f in seen), (VEC, full)
    assert 8192 * VEC in Ks and cells[8192 * VEC] == (1024, 8, True)
    assert Ks[-1] == 8192 * VEC + VEC and cells[Ks[-1]][2] == "unsupported"
    assert all(c[2] != "unsupported" for K, c in cells.items() if K != Ks[-1])
    assert all(K % VEC == 0 for K in Ks)


@pytest.mark.parametrize("VEC", [1, 2, 4, 8])
def test_row_Ks_reach_every_cell(VEC):
    check_row_coverage(bw.row_cell, bw.row_Ks, VEC)


def brute_row_cell(K, VEC):
    """rowwise.cuh restated lane by lane: the smallest MAXV in {1,2,4,8} whose MAXV * nt packs hold the row."""
    nvec = K // VEC
    nt = 64
    while nt < 1024 and nt * 8 < nvec:
        nt += 64
    for mv in (1, 2, 4, 8):
        if mv * nt >= nvec:
            return nt, mv, mv * nt == nvec
    return nt, 0, "unsupported"


def test_row_cell_equals_the_lane_by_lane_restatement():
    for VEC in (1, 2, 4, 8):
        for nvec in list(range(1, 1100)) + list(range(7600, 8300)):
            assert bw.row_cell(nvec * VEC, VEC) == brute_row_cell(nvec * VEC, VEC), (VEC, nvec)


def test_broken_row_mirrors_are_caught():
    def off_by_one_rounding(K, VEC):  # (nvec + 8) / 8 instead of (nvec + 7) / 8
        nvec = K // VEC
        nt = max(64, min(1024, (((nvec + 8) // 8 + 63) // 64) * 64))
        vpt = (nvec + nt - 1) // nt
        if vpt > 8:
            return nt, 0, "unsupported"
        mv = next(m for m in (1, 2, 4, 8) if vpt <= m)
        return nt, mv, K == mv * nt * VEC

    def le_for_lt(K, VEC):  # vpt < m instead of vpt <= m
        nt = bw.row_threads(K, VEC)
        vpt = (K // VEC + nt - 1) // nt
        if vpt >= 8:
            return nt, 0, "unsupported"
        mv = next(m for m in (1, 2, 4, 8) if vpt < m)
        return nt, mv, K == mv * nt * VEC

    for broken in (off_by_one_rounding, le_for_lt):
        with pytest.raises(AssertionError):
            for VEC in (1, 2, 4, 8):
                check_row_coverage(broken, bw.row_Ks, VEC)
        assert any(broken(n * 8, 8) != brute_row_cell(n * 8, 8) for n in range(1, 8300))


def check_stream_coverage(stream_cell, eb, VEC, CHUNK, op):
    cells = [stream_cell(n, eb, VEC, CHUNK, op) for n in bw.stream_sizes(eb, VEC, CHUNK, op)]
    if op == "unary" and eb * CHUNK >= 16:
        assert all(c["kernel"] == "stride" for c in cells)
        assert any(c["trips"] == 1 and c["partial"] and c["tail"] for c in cells)
        assert any(c["trips"] > 1 and c["grid"] == bw.STREAM_CUS * bw.STREAM_WGS_PER_CU and c["tail"] for c in cells)
        return
    assert any(c["kernel"] == "k1" and c["partial"] for c in cells)
    assert any(c["kernel"] == "kb" and not c["partial"] and c["grid"] > 1 for c in cells)
    assert any(c["kernel"] == "kb" and c["mixed"] and c["tail"] == 0 for c in cells)
    if CHUNK > 1:
        assert any(c["kernel"] == "kb" and c["mixed"] and c["tail"] for c in cells)
        assert any(c["kernel"] == "k1" and c["tail"] for c in cells)
    assert all(c["K"] == (bw.stream_kb(eb * CHUNK) if c["kernel"] == "kb" else 1) for c in cells)


@pytest.mark.parametrize("op,rungs", [("unary", UNARY_RUNGS), ("add", ADD_RUNGS)])
def test_stream_sizes_reach_every_cell(op, rungs):
    for _, eb, VEC, CHUNK in rungs:
        check_stream_coverage(bw.stream_cell, eb, VEC, CHUNK, op)
        for n in bw.stream_sizes(eb, VEC, CHUNK, op):
            assert n * eb * 3 < bw.STREAM_CAP_LIFT // 4  # small tensors: tens of MB at most


def brute_stream_kb_cell(n, eb, CHUNK):
    """The block-contiguous kernels restated pack by pack: which packs the if-branch and the else-branch of each workgroup touch."""
    kb = bw.stream_kb(eb * CHUNK)
    nvec = n // CHUNK
    K = 1 if nvec < 1024 * kb else kb
    grid = (nvec + 256 * K - 1) // (256 * K)
    covered, partial, mixed = 0, False, False
    for b in sorted({0, max(0, grid - 2), grid - 1}):  # the first, last-but-one and last workgroups
        for t in range(256):
            base = b * 256 * K + t
            if base + (K - 1) * 256 < nvec:
                held = K
            else:
                held = sum(1 for k in range(K) if base + k * 256 < nvec)
                if b == grid - 1:
                    partial = True
                    mixed = mixed or 0 < held < K
            covered += held if b == grid - 1 else 0
    return K, grid, partial, mixed, covered


def test_stream_cell_equals_the_pack_by_pack_restatement():
    for op, rungs in (("unary", UNARY_RUNGS), ("add", ADD_RUNGS)):
        for _, eb, VEC, CHUNK in rungs:
            if op == "unary" and eb * CHUNK >= 16:
                continue
            kb = bw.stream_kb(eb * CHUNK)
            edge = 1024 * kb
            for nvec in (1, 255, 256, 257, 1000, edge - 1, edge, edge + 1, edge + 256 * kb - 1, edge + 256 * kb, edge + 3 * 256 + 17, 9 * edge + 5):
                n = nvec * CHUNK + (CHUNK - 1)
                c = bw.stream_cell(n, eb, VEC, CHUNK, op)
                K, grid, partial, mixed, covered = brute_stream_kb_cell(n, eb, CHUNK)
                assert (c["K"], c["grid"], c["partial"], c["mixed"]) == (K, grid, partial, mixed), (op, eb, CHUNK, nvec)
                assert covered == nvec - (grid - 1) * 256 * K and c["tail"] == CHUNK - 1


def test_broken_stream_mirrors_are_caught():
    def le_for_lt(n, eb, VEC, CHUNK, op="unary"):  # nvec <= 1024 * KB picks the K = 1 kernel
        c = bw.stream_cell(n, eb, VEC, CHUNK, op)
        if c["kernel"] == "kb" and c["packs"] == bw.STREAM_K1_BLOCKS * c["K"]:
            c.update(kernel="k1", K=1, grid=(c["packs"] + 255) // 256, partial=False, mixed=False)
        return c

    def off_by_one_rounding(n, eb, VEC, CHUNK, op="unary"):  # grid = nvec / (256 K) + 1
        c = bw.stream_cell(n, eb, VEC, CHUNK, op)
        if c["kernel"] == "kb":
            per = 256 * c["K"]
            c["grid"] = c["packs"] // per + 1
            c["partial"] = True
        return c

    eb, VEC, CHUNK = 2, 2, 2
    kb = bw.stream_kb(eb * CHUNK)
    n_edge = 1024 * kb * CHUNK
    assert le_for_lt(n_edge, eb, VEC, CHUNK)["K"] != brute_stream_kb_cell(n_edge, eb, CHUNK)[0]
    assert off_by_one_rounding(n_edge, eb, VEC, CHUNK)["grid"] != brute_stream_kb_cell(n_edge, eb, CHUNK)[1]
    with pytest.raises(AssertionError):
        check_stream_coverage(off_by_one_rounding, eb, VEC, CHUNK, "unary")  # no whole grid left


def check_reduce_coverage(reduce_cell, eb, VEC, op):
    sizes = bw.reduce_sizes(eb, VEC, op)
    cells = [reduce_cell(n, eb, VEC, op) for n in sizes]
    if VEC > 1:
        assert any(c["nvec"] == 0 and c["tail"] for c in cells)
    assert any(c["nfull"] > 0 and c["leftover"] == 0 and c["tail"] == 0 for c in cells)
    want_tail = (lambda c: c["tail"] > 0) if VEC > 1 else (lambda c: True)
    assert any(0 < c["nfull"] <= bw.RED_MAX_WG and c["leftover"] and want_tail(c) for c in cells)
    assert any(c["nfull"] > bw.RED_MAX_WG and c["nfull"] % bw.RED_MAX_WG and c["owner"] != 0 and c["grid"] == bw.RED_MAX_WG and c["leftover"]
               and want_tail(c) for c in cells)
    assert sizes[-2:] == sorted(sizes)[-2:]


@pytest.mark.parametrize("op,rungs", [("reduce", REDUCE_RUNGS), ("dot", DOT_RUNGS)])
def test_reduce_sizes_reach_every_region(op, rungs):
    for eb, VEC in rungs:
        check_reduce_coverage(bw.reduce_cell, eb, VEC, op)


def test_reduce_cell_equals_the_launcher_restated_and_broken_copies_are_caught():
    def brute(n, eb, VEC, op):
        K = (bw.RED_K if op == "reduce" else bw.DOT_K)[0 if eb * VEC >= 16 else 1]
        nvec, chunk = n // VEC, 256 * K
        nfull = 0
        while (nfull + 1) * chunk <= nvec:
            nfull += 1
        chunks = nfull + (1 if nvec > nfull * chunk else 0)
        grid = min(max(chunks, 1), 1024)
        return K, chunk, nfull, grid, nfull % grid, nvec - nfull * chunk, n - nvec * VEC

    def off_by_one(n, eb, VEC, op="reduce"):  # chunks = nvec / chunk + 1
        c = bw.reduce_cell(n, eb, VEC, op)
        c["grid"] = max(1, min(1024, c["nvec"] // c["chunk"] + 1))
        c["owner"] = c["nfull"] % c["grid"]
        return c

    def le_for_lt(n, eb, VEC, op="reduce"):  # sizeof(P) > 16 instead of >= 16
        c = bw.reduce_cell(n, eb, VEC, op)
        if eb * VEC == 16:
            return bw.reduce_cell(n, eb // 2, VEC, op)
        return c

    key = ("K", "chunk", "nfull", "grid", "owner", "leftover", "tail")
    for op, rungs in (("reduce", REDUCE_RUNGS), ("dot", DOT_RUNGS)):
        for eb, VEC in rungs:
            caught = {off_by_one: False, le_for_lt: eb * VEC != 16}
            for n in bw.reduce_sizes(eb, VEC, op) + [1, 2 * 256 * 8 * VEC, 1024 * 256 * 8 * VEC]:
                want = brute(n, eb, VEC, op)
                assert tuple(bw.reduce_cell(n, eb, VEC, op)[k] for k in key) == want, (op, eb, VEC, n)
                for broken in caught:
                    caught[broken] = caught[broken] or tuple(broken(n, eb, VEC, op)[k] for k in key) != want
            assert all(caught.values()), (op, eb, VEC)


# ---------------------------------------------------------------- exact inputs
EXACT_DTYPES = [(torch.float32, 4, (1, 4), "f32"), (torch.float16, 2, (1, 2, 8), "f16"), (torch.bfloat16, 2, (1, 2, 8), "bf16"),
                (torch.float8_e4m3fn, 1, (1, 16), "f16"), (torch.float8_e5m2, 1, (1, 16), "f16"), (torch.int8, 1, (1, 16), "i32")]


def test_exact_sum_inputs_are_small_integers_below_2_to_24():
    for dtype, eb, vecs, acc in EXACT_DTYPES:
        for VEC in vecs:
            for op in ("reduce", "dot") if dtype in (torch.float32, torch.float16) else ("reduce",):
                for n in bw.reduce_sizes(eb, VEC, op):
                    x = bw.exact_sum_inputs(n, dtype, seed=n % 1000)
                    assert x.dtype == dtype and x.numel() == n
                    xi = x.to(torch.float32).to(torch.int64)
                    assert torch.equal(xi.to(torch.float32).to(dtype).view(torch.uint8), x.view(torch.uint8))  # stored exactly
                    assert int(xi.min()) >= -2 and int(xi.max()) <= 2
                    assert int(xi.abs().sum()) < 2 ** 24
                    if op == "dot":
                        y = bw.exact_sum_inputs(n, dtype, seed=n % 1000 + 1).to(torch.float32).to(torch.int64)
                        assert int((xi * y).abs().sum()) < 2 ** 24
                    if n > 1000:
                        assert set(xi.unique().tolist()) == {-2, -1, 0, 1, 2} and int(xi.sum()) != 0
            # every in-pack partial (at most VEC terms of magnitude <= 2; dot products <= 4 in fp32) is an integer the accumulator holds
            assert 2 * max(vecs) <= 2 ** bw.ACC_BITS[acc]
    assert 4 * 8 <= 2 ** bw.ACC_BITS["f32"]
    for dtype in (torch.float8_e4m3fn, torch.float8_e5m2):  # the fp8 formats hold -4 ... 4
        v = torch.arange(-4, 5, dtype=torch.float32)
        assert torch.equal(v.to(dtype).to(torch.float32), v)
    assert not torch.equal(bw.exact_sum_inputs(4096, torch.float32, 1), bw.exact_sum_inputs(4096, torch.float32, 2))
    assert torch.equal(bw.exact_sum_inputs(4096, torch.float32, 1), bw.exact_sum_inputs(4096, torch.float32, 1))


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
def test_fp8_code_table(fmt):
    v, nan, inf = bw.fp8_code_table(fmt)
    assert v.dtype == torch.float64 and v.shape == (256,)
    if fmt == "e4m3":  # OCP e4m3fn: no infinities, NaN = S.1111.111, max 448, least subnormal 2^-9
        assert int(nan.sum()) == 2 and nan[0x7f] and nan[0xff] and int(inf.sum()) == 0
        assert v[0x7e] == 448.0 and v[0x01] == 2.0 ** -9 and v[0x08] == 2.0 ** -6 and v[0x38] == 1.0
    else:              # e5m2: IEEE-like, inf = S.11111.00, NaN above, max 57344, least subnormal 2^-16
        assert int(inf.sum()) == 2 and inf[0x7c] and inf[0xfc] and int(nan.sum()) == 6
        assert v[0x7b] == 57344.0 and v[0x01] == 2.0 ** -16 and v[0x04] == 2.0 ** -14 and v[0x3c] == 1.0
    fin = ~(nan | inf)
    assert torch.equal(v[128:][fin[128:]], -v[:128][fin[:128]])  # sign bit
    assert torch.equal(v[fin].to(torch.float16).double(), v[fin])  # every finite code is a half value
    mag = v[:128][fin[:128]]
    assert bool((mag[1:] > mag[:-1]).all())  # codes order the magnitudes
    skip = bw.fp8_pack16_skip(fmt)
    assert len(skip) < 64, len(skip)  # under a quarter of the codes: the pack check cannot quietly empty itself
    assert all(abs(v[c].item()) * 16 > 65504 for c in skip) or fmt == "e4m3"
    if fmt == "e4m3":
        assert skip == []


# ---------------------------------------------------------------- guard bands
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2, torch.int8, torch.int32])
@pytest.mark.parametrize("n", [1, 7, 1000])
def test_guard_bands(dtype, n):
    for fill in ("nan", "sentinel"):
        if dtype == torch.int32 and fill == "nan":
            continue
        v, buf = bw.guarded(n, dtype, "cpu", fill)
        eb = v.element_size()
        assert v.dtype == dtype and v.numel() == n and v.is_contiguous()
        assert bw.GUARD_BYTES % 16 == 0 and (v.data_ptr() - buf.data_ptr()) == bw.GUARD_BYTES
        assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0
        assert buf.numel() * eb == 2 * bw.GUARD_BYTES + n * eb
        assert bw.guards_intact(buf, n, dtype, fill) and bw.untouched(v, fill)
        if fill == "nan" and dtype != torch.int8:
            assert bool(torch.isnan(buf.view(dtype).to(torch.float32)).all())
        if fill == "nan" and dtype == torch.int8:
            assert bool((buf.view(dtype) == 127).all())
        v.copy_(torch.zeros(n).to(dtype))  # writing the payload leaves the guards alone ...
        assert bw.guards_intact(buf, n, dtype, fill) and not bw.untouched(v, fill)
        for pos in (bw.GUARD_BYTES // eb - 1, bw.GUARD_BYTES // eb + n, 0, buf.numel() - 1):  # ... one element next to it does not
            b2 = buf.clone()
            b2[pos] = 0
            assert not bw.guards_intact(b2, n, dtype, fill)


# ---------------------------------------------------------------- copied rules
def test_copied_rules_are_the_originals():
    for key, (path, line) in bw.RULE_TEXT.items():
        assert line in open(os.path.join(HERE, path)).read(), key
    num = r"([0-9.]+(?:e-?\d+)?)"
    a = re.search(r"\(%s, %s\) if dt == torch\.float32 else \(%s, %s\)" % (num, num, num, num), bw.RULE_TEXT["activation"][1]).groups()
    assert (float(a[0]), float(a[1])) == bw.RULES["activation_f32"] and (float(a[2]), float(a[3])) == bw.RULES["activation_f16"]
    for key in ("softmax_f32", "softmax_f16", "layer_norm_f32", "layer_norm_f16", "rms_norm_f32", "rms_norm_f16"):
        atol, rtol = re.search(r"atol=%s, rtol=%s" % (num, num), bw.RULE_TEXT[key][1]).groups()
        assert (float(rtol), float(atol)) == bw.RULES[key], key
    floor, slack = re.search(r"\(%s \+ pair_norm \* t \* freq \* %s\)" % (num, num), bw.RULE_TEXT["rope"][1]).groups()
    assert (float(floor), float(slack)) == bw.ROPE_RULE[:2]
    orig = open(os.path.join(HERE, "test_gpu_bandwidth.py")).read()
    assert "assert float((colmax <= 2e-4).double().mean()) >= 0.75" in orig and bw.ROPE_RULE[2] == 0.75
    # rope_bound forms the bound as the original does: the same four lines
    mine = open(os.path.join(HERE, "bw_reference.py")).read()
    for ln in ("t = torch.arange(S, dtype=torch.float64).view(S, 1)",
               "freq = (1.0 / (10000.0 ** (torch.arange(0, Hd, 2).float() / Hd))).double().view(1, Hd // 2)",
               "pair_norm = x.double().view(S, -1, 2).norm(dim=-1)"):
        assert ln in orig and ln in mine


def test_excess_is_allclose_as_a_ratio():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn(1000, generator=g).double()
    for scale, ok in ((0.5, True), (0.999, True), (1.001, False), (3.0, False)):
        got = ref + scale * (1e-6 + 2e-6 * ref.abs())
        r, _ = bw.excess(got, ref, "activation_f32")
        assert (r <= 1.0) is ok and torch.allclose(got, ref, rtol=2e-6, atol=1e-6) is ok
        assert abs(r - scale) < 1e-6
    inf, nan = float("inf"), float("nan")
    assert bw.excess(torch.tensor([inf, -inf, nan, 1.0]), torch.tensor([inf, -inf, nan, 1.0]), "activation_f32")[0] == 0.0
    for got, ref in (([inf], [1.0]), ([1.0], [inf]), ([nan], [1.0]), ([1.0], [nan]), ([inf], [-inf])):
        assert bw.excess(torch.tensor(got), torch.tensor(ref), "activation_f32")[0] == inf


# ---------------------------------------------------------------- sweeps
def test_activation_sweeps():
    h = bw.half_finite_values()
    assert h.dtype == torch.float16 and h.numel() == 63488 and bool(torch.isfinite(h).all())
    assert h.view(torch.int16).unique().numel() == 63488 and h.float().max().item() == 65504.0 and h.float().min().item() == -65504.0
    f = bw.f32_sweep_values()
    assert f.dtype == torch.float32 and bool(torch.isfinite(f).all())
    a = f.abs()
    assert a[a > 0].min().item() <= 1.0001e-30 and a.max().item() >= 2.999e38
    for th in bw.ACT_THRESHOLDS:
        t = torch.tensor(th, dtype=torch.float32)
        for s in (1.0, -1.0):
            for v in (t, torch.nextafter(t, torch.tensor(float("inf"))), torch.nextafter(t, torch.tensor(-float("inf")))):
                assert bool((f == s * v).any()), (th, s)
    assert bool(((f == 0) & ~torch.signbit(f)).any()) and bool(((f == 0) & torch.signbit(f)).any())
    # the issue's second prediction, on the CPU: the oracle returns x above the clamp, the clamped formula 88.376
    import oracle
    x = torch.tensor([100.0, 1000.0])
    assert oracle.activation("gelu", x).tolist() == [100.0, 1000.0]
    xc = x.clamp(-88.3762626647949, 88.3762626647949)
    u = 0.7978845608028654 * (xc + 0.044715 * xc ** 3)
    assert torch.allclose(xc / (1 + torch.exp(-2 * u)), torch.tensor([88.3763, 88.3763]), atol=1e-3)


def test_online_softmax_recurrence_loses_a_lane_that_starts_at_minus_inf():
    """The issue's first prediction, on the CPU: the per-lane (m, d) recurrence of softmax_row_kernel's ONLINE mode, as the source had it and as
    it is now (no exp(m - mn) while mn == -inf)."""
    ninf = float("-inf")

    def run(vals, fixed):
        m, d = torch.tensor(ninf), torch.tensor(0.0)
        for v in vals:
            v = torch.tensor(v)
            mn = torch.maximum(m, v)
            ms = torch.tensor(0.0) if (fixed and mn == ninf) else mn
            d = d * torch.exp(m - ms) + torch.exp(v - ms)
            m = mn
        return m.item(), d.item()

    m, d = run([ninf, 1.0, 2.0], fixed=False)
    assert m == 2.0 and d != d
    m, d = run([ninf, 1.0, 2.0], fixed=True)
    assert m == 2.0 and abs(d - (1 + torch.exp(torch.tensor(-1.0)).item())) < 1e-6
    assert run([ninf, ninf], fixed=True) == (ninf, 0.0)
    assert run([0.5, 1.0, -3.0], fixed=True) == run([0.5, 1.0, -3.0], fixed=False)  # rows without -inf: the same operations
    assert "const float ms = (mn == -INFINITY) ? 0.f : mn;" in src("softmax.hip")


def test_emulated_softmax_is_a_softmax():
    g = torch.Generator().manual_seed(1)
    for K, VEC in ((1000, 1), (65536, 8), (32768, 4), (520, 4)):
        x = torch.randn(2, K, generator=g) * 3
        ref = torch.softmax(x.double(), dim=1)
        r, _ = bw.excess(bw.emulate_softmax_f32(x, VEC).double(), ref, "softmax_f32")
        assert r < 1.0, (K, VEC, r)
