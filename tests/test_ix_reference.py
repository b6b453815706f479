"""CPU only: the helpers of tests/ix_reference.py, proven before they judge a kernel (tests/test_gpu_ix_edges.py) -- the dispatch mirrors against the
constants and expressions of the HIP sources, each mirror restated lane by lane on small cases, the shape lists against the cells they must reach,
broken copies of each mirror against those same checks, the exact-input constructors in int64, and the SGEMM tile forms through cln_describe."""
import os
import re

import pytest
import torch

import ix_reference as ix

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "cuda-learn-notes_amd", "csrc")


def src(name):
    return open(os.path.join(CSRC, name)).read()


def one(pattern, text):
    m = re.findall(pattern, text)
    assert len(m) >= 1, pattern
    assert len(set(m)) == 1, (pattern, m)
    return m[0]


# ---------------------------------------------------------------- constants
def test_gemv_constants_are_those_of_blas1_hip():
    s = src("blas1.hip")
    assert int(one(r"constexpr int U = (\d+);", s)) == ix.GEMV_U
    assert "for (; k + (U - 1) * G * VEC < K; k += U * G * VEC)" in s and "for (; k < K; k += G * VEC)" in s
    assert "for (; k + (U - 1) * 64 * VEC < K; k += U * 64 * VEC)" in s and "for (; k < K; k += 64 * VEC)" in s
    macro = s[s.index("#define CLN_GEMV"):s.index("CLN_GEMV(sgemv_k32_f32")]
    assert set(re.findall(r"launch_gemv_rows<T, VEC, (\d), (\d)>", macro)) == {("4", "8"), ("2", "8"), ("4", "4"), ("2", "4")}
    rows = re.findall(r"M >= (\d+) \? launch_gemv_rows<T, VEC, 4, (\d)>\(a, x, y, M, K, \(hipStream_t\)stream\)\s*\\\s*: launch_gemv_rows<T, VEC, 2, (\d)>", macro)
    assert rows == [(str(ix.GEMV_ROWS4_M), "8", "8"), (str(ix.GEMV_ROWS4_M), "4", "4")] and ix.GEMV_ROWS_U == {1: 8, 4: 4}
    assert "if (G == 32 && VEC == 1 && sizeof(T) == 2 && K %% 64 == 0 && K >= %d && M >= %d)" % (ix.GEMV_WIDE_K, ix.GEMV_ROWS_M) in macro
    assert "if (G == 32 && VEC == 1 && K %% 64 == 0 && K >= %d) return launch_gemv<T, VEC, 64>" % ix.GEMV_WIDE_K in macro
    assert "if (G == 32 && VEC > 1 && sizeof(T) == 2 && K %% (64 * VEC) == 0 && K >= %d * 64 * VEC && M >= %d)" % (ix.GEMV_ROWS4X_PIECES, ix.GEMV_ROWS_M) in macro
    assert "constexpr int RPB = 4 * R;" in s and "constexpr int RPB = 4 * (64 / G);" in s
    decl = dict((n, (t, int(v), int(g), c)) for n, t, v, g, c in re.findall(r"^CLN_GEMV\((\w+), (\w+), (\d), (\d+), (.*)\)$", s, re.M))
    assert set(decl) == set(ix.GEMV_RUNGS)
    for name, (dname, VEC, G) in ix.GEMV_RUNGS.items():
        t, v, g, cond = decl[name]
        assert (t == "float") == (dname == "float32") and (v, g) == (VEC, G)
        assert cond == ("K == 16" if G == 16 else "K %% %d == 0" % (32 * VEC))


def test_transpose_constants_are_those_of_blas1_hip_and_common_h():
    s, c = src("blas1.hip"), src("common.h")
    assert int(one(r"#define CLN_STREAM_WGS_PER_CU (\d+)", c)) == ix.STREAM_WGS_PER_CU
    assert int(re.search(r"0x7fffffffLL : (\d+)LL \* CLN_STREAM_WGS_PER_CU;", c).group(1)) == ix.STREAM_CUS
    assert "const int grid = cln_stream_grid(n / (v4 ? 4 : 1), %d);" % ix.TR_NT in s
    assert s.count("stride = (long long)gridDim.x * %d;" % ix.TR_NT) == 2
    assert "if (row %% %d == 0 && col %% %d == 0 && cln_aligned16(x) && cln_aligned16(y))" % (ix.TR_REG_BLOCK, ix.TR_REG_BLOCK) in s
    assert "(row %% %d || col %% %d || !cln_aligned16(x)" % (ix.TR_LDS_TILE, ix.TR_LDS_TILE) in s
    assert "if (v4 && ((kind == TR_READ4 ? col : row) % 4 ||" in s
    assert "const long long nb = total / %d;" % ix.TR_NT in s and "if (nb > 1 && t < nb * %d)" % ix.TR_NT in s
    assert "if (side * side == nb) t = ((b % side) * side + (b / side + b % side) % side) * 256 + (t % 256);" in s
    assert "dim3((int)((n + 255) / 256))" in s
    kinds = {"TR_READ1": "read1", "TR_READ4": "read4", "TR_WRITE1": "write1", "TR_WRITE4": "write4", "TR_DIAG": "diag", "TR_LDS": "lds",
             "TR_LDS_BCF": "lds_bcf", "TR_READ4_2D": "read4_2d", "TR_WRITE4_2D": "write4_2d"}
    decl = dict(re.findall(r"^CLN_TR\((\w+), (\w+)\)$", s, re.M))
    assert {n: kinds[k] for n, k in decl.items()} == ix.TR_RUNGS and len(decl) == 13 and len(set(decl.values())) == 9


def test_indexing_constants_are_those_of_indexing_hip():
    s, c = src("indexing.hip"), src("common.h")
    assert int(one(r"constexpr int HIST_LDS_BINS = (\d+);", s)) == ix.HIST_LDS_BINS
    assert int(one(r"constexpr int NT = (\d+);", s)) == ix.HIST_LDS_NT
    assert "const int grid = (int)(gw < 1 ? 1 : (gw > %d ? %d : gw));" % (ix.HIST_LDS_MAX_WG, ix.HIST_LDS_MAX_WG) in s
    assert "const int grid = (int)(g < 1 ? 1 : (g > %d ? %d : g));" % (ix.HIST_GLOBAL_MAX_WG, ix.HIST_GLOBAL_MAX_WG) in s
    assert "long long g = (n / VEC + 255) / %d;" % ix.HIST_GLOBAL_NT in s and "long long gw = (n / VEC + NT - 1) / NT;" in s
    assert s.count("for (; i + 3 * stride < nvec; i += %d * stride)" % ix.HIST_UNROLL) == 2 and "if (nbins <= HIST_LDS_BINS)" in s
    assert "if (VEC > 1 && blockIdx.x == 0) {  // ragged tail" in s
    assert "const long long base = (long long)blockIdx.x * (%d * KP) + threadIdx.x;" % ix.EMB_NT in s
    kp1, kp = re.search(r"traffic >= \((\d+)LL << 20\)\) \? (\d) : (\d);", s).groups()[0], re.search(r"traffic >= \(\d+LL << 20\)\) \? (\d) : (\d);", s).groups()
    assert int(kp1) << 20 == ix.EMB_KP1_TRAFFIC and (int(kp[0]), int(kp[1])) == (1, ix.EMB_KP)
    assert "const int kp = (VEC * sizeof(T) >= 16 && traffic >=" in s
    assert "const long long grid = (total + %d * kp - 1) / (%d * kp);" % (ix.EMB_NT, ix.EMB_NT) in s
    assert "traffic = 2LL * n * emb * (long long)sizeof(T);" in s
    assert int(re.search(r"cln_stream_nt\(long long footprint_bytes\) \{ return footprint_bytes >= \((\d+)LL << 20\)", c).group(1)) << 20 == ix.NT_TRAFFIC
    decl = dict((n, (t, int(v))) for n, t, v in re.findall(r"^CLN_EMB\((\w+), (\w+), (\d), \w+\)$", s, re.M))
    assert {n: ("float32" if t == "float" else "float16", v) for n, (t, v) in decl.items()} == ix.EMB_RUNGS
    assert "return launch_hist<1>" in s and "return launch_hist<4>" in s


def test_sgemm_constants_are_those_of_the_sources():
    s, d = src("sgemm.hip"), src("sgemm_dma.cuh")
    assert "(long long)(M / 64) * (N / 128) <= %d && K >= %d) best.ksplit = true;" % (ix.SGEMM_KSPLIT_TILES, ix.SGEMM_KSPLIT_K) in s
    launches = re.findall(r"sgemm_dma::launch<2, 2, (\d), 2, (\d+), (\d)(, true)?>", s)
    assert launches == [("1", "16", "3", ", true"), ("4", "16", "3", ""), ("2", "16", "3", ""), ("1", "16", "3", "")]
    assert ix.SGEMM_BK == 16 and ix.SGEMM_RING == 3
    assert "const int first = (nt + 1) / 2;" in d and "int nt = K / BK;" in d
    valu = dict((n, (int(bk), int(tn))) for n, bk, tn in re.findall(r"^CLN_S3\((\w+), \(launch_valu<(\d+), (\d+), \w+, \w+>", s, re.M))
    assert valu == ix.VALU_RUNGS
    assert "if (M % 128 || N % (16 * TN) || K % BK) return CLN_ERR_UNSUPPORTED;" in s


# ---------------------------------------------------------------- GEMV: lane by lane, every cell, broken mirrors
GEMV_WANT = {  # form -> (unrolled, rem) cells that the lists must reach
    "g16": {(0, 1)},
    "g32x1": {(0, 1), (0, 7), (1, 0), (1, 1), (1, 7), (2, 1)},
    "g64": {(1, 0), (1, 1), (1, 7), (2, 0)},
    "g32x4": {(0, 1), (0, 7), (1, 0), (1, 1)},
    "rows_x1": {(1, 0), (1, 1), (1, 7), (2, 1)},
    "rows_x4": {(1, 0), (1, 1), (1, 3), (2, 1)},
}


def check_gemv(gemv_cell):
    seen = {}
    for name, (dname, VEC, G) in ix.GEMV_RUNGS.items():
        for M, K in ix.gemv_cases(name):
            c = gemv_cell(name, M, K)
            assert c["form"] != "unsupported", (name, M, K)
            # the mirror's trip counts are those of the kernel's loops, for the first and the last lane of a row
            for lane in (0, c["lanes"] - 1):
                un, rem, cover = ix.gemv_lane_trips(K, c["lanes"], VEC, c["U"], lane)
                assert (un, rem) == (c["unrolled"], c["rem"]), (name, M, K, lane)
                assert max(cover) < K and len(set(cover)) == len(cover) == K // c["lanes"]
            rows = c["form"].startswith("rows")
            key = "g16" if G == 16 else ("rows_x%d" % VEC if rows else "g64" if c["form"] == "g64" else "g32x%d" % VEC)
            seen.setdefault((name, key), set()).add((c["unrolled"], c["rem"], M, c["form"]))
            # dispatch, restated from the text of the macro
            half = dname == "float16"
            if half and G == 32 and M >= 4096 and ((VEC == 1 and K % 64 == 0 and K >= 512) or (VEC == 4 and K % 256 == 0 and K >= 1024)):
                assert c["form"] == ("rows4" if M >= 16384 else "rows2") and c["U"] == (8 if VEC == 1 else 4) and c["lanes"] == 64
            elif G == 32 and VEC == 1 and K % 64 == 0 and K >= 512:
                assert c["form"] == "g64" and c["U"] == 8
            else:
                assert c["form"] == "g%d" % G and c["U"] == 8
            assert c["grid"] == -(-M // c["rpb"]) and 1 <= c["last_rows"] <= c["rpb"]
    for (name, key), cells in seen.items():
        assert {(u, r) for u, r, _, _ in cells} >= GEMV_WANT[key], (name, key)
        Ms = {m for _, _, m, _ in cells}
        if key.startswith("rows"):  # both row counts per wave, each from its first row count on, the clamped last rows included
            assert Ms == set(m for m in ix.GEMV_M if m >= 4096)
            assert {f for _, _, m, f in cells if m < 16384} == {"rows2"} and {f for _, _, m, f in cells if m >= 16384} == {"rows4"}
        elif key == "g64" and name.startswith("hgemv"):
            assert Ms == set(m for m in ix.GEMV_M if m < 4096)  # 4095: the last row count of the 64-lane kernel
        else:
            assert Ms >= set(ix.GEMV_M if not (name.startswith("hgemv") and key == "g32x4") else ix.GEMV_SMALL_M)
    keys = {name: {k for (n, k) in seen if n == name} for name in ix.GEMV_RUNGS}
    assert keys["sgemv_k32_f32"] == {"g32x1", "g64"} and keys["hgemv_k32_f16"] == {"g32x1", "g64", "rows_x1"}
    assert keys["sgemv_k128_f32x4"] == {"g32x4"} and keys["hgemv_k128_f16x4"] == {"g32x4", "rows_x4"}
    assert keys["sgemv_k16_f32"] == keys["hgemv_k16_f16"] == {"g16"}
    # partly empty last waves / workgroups, and the rows forms' clamped rows (M - m0 < R for the last wave)
    for name in ix.GEMV_RUNGS:
        assert any(gemv_cell(name, M, ix.gemv_Ks(name)[0])["last_rows"] < gemv_cell(name, M, ix.gemv_Ks(name)[0])["rpb"] for M in ix.GEMV_SMALL_M)
    for M, R in ((4097, 2), (16385, 4), (16386, 4), (16387, 4)):
        assert gemv_cell("hgemv_k32_f16", M, 512)["form"] == "rows%d" % R and M % R


def test_gemv_lists_reach_every_cell_and_broken_mirrors_fail():
    check_gemv(ix.gemv_cell)
    assert ix.gemv_cell("sgemv_k32_f32", 8, 48)["form"] == "unsupported" and ix.gemv_cell("sgemv_k16_f32", 8, 32)["form"] == "unsupported"
    assert ix.gemv_cell("hgemv_k128_f16x4", 4096, 1152)["form"] == "g32"  # K % 256 != 0 keeps 32 lanes per row

    def with_const(**kw):
        def f(name, M, K):
            old = {k: getattr(ix, k) for k in kw}
            try:
                for k, v in kw.items():
                    setattr(ix, k, v)
                return ix.gemv_cell(name, M, K)
            finally:
                for k, v in old.items():
                    setattr(ix, k, v)
        return f

    for broken in (with_const(GEMV_U=4), with_const(GEMV_ROWS_M=4097), with_const(GEMV_ROWS4_M=16385), with_const(GEMV_WIDE_K=576),
                   with_const(GEMV_ROWS_U={1: 8, 4: 8}), with_const(GEMV_ROWS4X_PIECES=5)):
        with pytest.raises(AssertionError):
            check_gemv(broken)


def test_gemv_impulse_positions():
    c = ix.gemv_cell("hgemv_k128_f16x4", 16384, 2304)
    assert (c["form"], c["piece"], c["unrolled"], c["rem"]) == ("rows4", 256, 2, 1)
    assert ix.gemv_impulse_k0(c, 2304) == [0, 3, 255, 256, 2047, 2048, 2303]
    c = ix.gemv_cell("sgemv_k32_f32", 5, 32)
    assert ix.gemv_impulse_k0(c, 32) == [0, 31]


# ---------------------------------------------------------------- transpose
def check_tr(tr_cell):
    seen = set()
    for name, kind in ix.TR_RUNGS.items():
        ok, refused = ix.tr_shapes(name)
        for (r, c) in refused:
            assert tr_cell(name, r, c)["kernel"] == "unsupported", (name, r, c)
        for (r, c) in ok:
            cell = tr_cell(name, r, c)
            assert cell["kernel"] != "unsupported", (name, r, c)
            seen.add((name, cell["kernel"], cell["multi"], cell["perm"], cell["tail"], cell["partial"]))
            if cell["kernel"] in ("read1", "read4", "write1", "write4"):  # lane 0 of workgroup 0, walked
                vec = 4 if cell["kernel"][-1] == "4" else 1
                total, stride = r * c // vec, cell["grid"] * 256
                assert cell["multi"] == (len(range(0, total, stride)) > 1) and cell["grid"] <= 8192
                assert (r * c) % vec == 0
            if cell["kernel"] == "reg4x4":
                assert r % 32 == 0 and c % 32 == 0
    for name, kind in ix.TR_RUNGS.items():
        mine = {s[1:] for s in seen if s[0] == name}
        kernels = {m[0] for m in mine}
        if kind in ("read1", "write1", "read4", "write4"):
            assert kernels == {kind} and {m[1] for m in mine} == {False, True}  # one trip and more
        elif kind.endswith("_2d"):
            assert kernels == {"reg4x4", kind[:-3]} and (kind[:-3], True, False, False, True) in mine
            assert {m[4] for m in mine if m[0] == "reg4x4"} == {False, True}  # whole and partly idle last workgroup
        elif kind == "diag":
            assert {(m[2], m[3]) for m in mine} == {(False, False), (True, False), (True, True), (False, True)}
        else:
            assert kernels == {kind}
    big = ix.TR_BIG[0] * ix.TR_BIG[1]
    assert big // 4 > 256 * 32 * 256 >= 2048 * 4096 // 4 and ix.TR_BIG[0] % 32 and ix.TR_BIG[1] % 32 and big < (1 << 24)


def test_transpose_lists_reach_every_cell_and_broken_mirrors_fail():
    check_tr(ix.tr_cell)
    c = ix.tr_cell("mat_transpose_f32_diagonal2d", 33, 32)
    assert (c["grid"], c["perm"], c["tail"]) == (5, True, True)
    assert ix.tr_cell("mat_transpose_f32_diagonal2d", 48, 48)["grid"] == 9 and not ix.tr_cell("mat_transpose_f32_diagonal2d", 16, 16)["perm"]
    # the permutation is a bijection of the whole blocks: with it on, every output element is still written exactly once
    for nb in (4, 9, 16):
        assert sorted(ix.diag_block(b, nb) for b in range(nb)) == list(range(nb)) and any(ix.diag_block(b, nb) != b for b in range(nb))
    assert [ix.diag_block(b, 7) for b in range(7)] == list(range(7)) and ix.diag_block(0, 1) == 0

    def cap_one_more(name, r, c):  # a grid cap that (2052, 4100) would no longer exceed
        old = ix.STREAM_WGS_PER_CU
        ix.STREAM_WGS_PER_CU = 33
        try:
            return ix.tr_cell(name, r, c)
        finally:
            ix.STREAM_WGS_PER_CU = old

    def no_tail(name, r, c):
        cell = dict(ix.tr_cell(name, r, c))
        cell["tail"] = False
        return cell

    def reg_everywhere(name, r, c):  # forgets that the register-block kernel needs multiples of 32
        cell = dict(ix.tr_cell(name, r, c))
        if ix.TR_RUNGS[name].endswith("_2d") and cell["kernel"] != "unsupported":
            cell["kernel"] = "reg4x4"
        return cell

    for broken in (cap_one_more, no_tail, reg_everywhere):
        with pytest.raises(AssertionError):
            check_tr(broken)


# ---------------------------------------------------------------- embedding
def emb_all_cases(name):
    return [(n, emb) for n, emb, _ in ix.emb_small_cases(name) + ix.emb_traffic_cases(name)]


def check_emb(emb_cell):
    for name, (dname, VEC) in ix.EMB_RUNGS.items():
        eb = 4 if dname == "float32" else 2
        wide = VEC * eb >= 16
        seen = set()
        for n, emb in emb_all_cases(name):
            c = emb_cell(name, n, emb)
            assert c["KP"] in (1, 4), (name, n, emb)
            seen.add((c["KP"], c["nt"], c["partial"]))
            total = n * (emb // VEC)
            # lane by lane: the last workgroup's live flags, and nobody beyond the grid
            live = ix.emb_block_live(total, c["KP"], c["grid"] - 1)
            nlive = sum(sum(row) for row in live)
            assert c["partial"] == (nlive < 256 * c["KP"]) and nlive == total - (c["grid"] - 1) * 256 * c["KP"] and nlive >= 1
            assert c["nt"] == (2 * n * emb * eb >= 256 << 20)
            assert (c["KP"] == 1) == (wide and 2 * n * emb * eb >= 512 << 20)
        want = {(4, False, False), (4, False, True), (4, True, False), (4, True, True)}
        want |= {(1, True, False), (1, True, True)} if wide else set()
        assert seen == want, (name, sorted(seen))
        small = [emb_cell(name, n, emb) for n, emb, _ in ix.emb_small_cases(name)]
        assert small[0]["total"] == 1 and [c["total"] for c in small[3:]] == [1023, 1024, 1025] and [c["grid"] for c in small[3:]] == [1, 1, 2]
        assert 256 % small[1]["ppr"] != 0 and small[1]["total"] < 256 and small[2]["total"] > 256 or VEC == 8  # (f16x8: 3 packs per row, 135 packs)
        assert 256 % small[1]["ppr"] != 0
    # the traffic cells sit exactly on the thresholds
    assert ix.emb_cell("embedding_f32", 32768, 1024)["traffic"] == 256 << 20 and ix.emb_cell("embedding_f32x4_pack", 65536, 1024)["traffic"] == 512 << 20
    assert ix.emb_cell("embedding_f16", 65536, 1024)["traffic"] == 256 << 20 and ix.emb_cell("embedding_f16x8", 131072, 1024)["traffic"] == 512 << 20


def test_embedding_lists_reach_every_cell_and_broken_mirrors_fail():
    check_emb(ix.emb_cell)
    assert ix.emb_cell("embedding_f16x8", 4, 12) == {"KP": 0}

    def kp1_late(name, n, emb):
        c = dict(ix.emb_cell(name, n, emb))
        if c["KP"] == 1 and c["traffic"] == 512 << 20:  # `>` for `>=`
            c["KP"] = 4
        return c

    def nt_late(name, n, emb):
        c = dict(ix.emb_cell(name, n, emb))
        c["nt"] = c["traffic"] > 256 << 20
        return c

    def kp1_everywhere(name, n, emb):  # forgets that the scalar rungs keep four packs per lane
        c = dict(ix.emb_cell(name, n, emb))
        if c["traffic"] >= 512 << 20:
            c["KP"] = 1
        return c

    for broken in (kp1_late, nt_late, kp1_everywhere):
        with pytest.raises(AssertionError):
            check_emb(broken)


# ---------------------------------------------------------------- histogram
def check_hist(hist_cell):
    for name, VEC in ix.HIST_RUNGS.items():
        seen = set()
        for nbins in (8192, 8193):
            for n in ix.hist_sizes(name):
                c = hist_cell(name, n, nbins)
                assert c["kernel"] == ("lds" if nbins <= 8192 else "global")
                nvec = n // VEC
                assert c["tail"] == n % VEC and c["nvec"] == nvec
                stride = c["grid"] * c["nt"]
                if c["kernel"] == "lds":
                    un, single, cover = ix.hist_lane_trips(nvec, stride, 0)
                    assert (un, single) == (c["unrolled"], c["single"]), (name, n)
                    # every pack once, over all lanes (small cases only: the walk is Python)
                    if nvec <= 4096:
                        allp = sorted(p for start in range(stride) for p in ix.hist_lane_trips(nvec, stride, start)[2])
                        assert allp == list(range(nvec))
                else:
                    assert c["single"] == len(range(0, nvec, stride)) and c["unrolled"] == 0
                seen.add((c["kernel"], min(c["unrolled"], 2), min(c["single"], 2), c["tail"], nvec == 0))
        lds = {s[1:] for s in seen if s[0] == "lds"}
        assert {s[0] for s in lds} == {0, 1, 2}
        assert {s[2] for s in lds} == set(range(VEC)) and {s[3] for s in seen if s[0] == "global"} == set(range(VEC))
        assert (VEC == 1) or any(s[3] for s in lds)  # x4: n < 4, no whole pack
        assert {s[2] for s in seen if s[0] == "global"} >= {1, 2}  # the global kernel's loop trips twice
        e = ix.HIST_EDGE
        assert [hist_cell(name, (e + d) * VEC, 8192)["unrolled"] for d in (-1, 0, 1)] == [0, 0, 1] and e == 3 * 256 * 1024
        assert hist_cell(name, (e + 1) * VEC, 8192)["grid"] == 256
        assert hist_cell(name, 0, 8)["kernel"] == "none"


def test_histogram_lists_reach_every_cell_and_broken_mirrors_fail():
    check_hist(ix.hist_cell)

    def with_const(**kw):
        def f(name, n, nbins):
            old = {k: getattr(ix, k) for k in kw}
            try:
                for k, v in kw.items():
                    setattr(ix, k, v)
                return ix.hist_cell(name, n, nbins)
            finally:
                for k, v in old.items():
                    setattr(ix, k, v)
        return f

    def edge_inclusive(name, n, nbins):  # `<=` for `<` at the unrolled loop's edge
        c = dict(ix.hist_cell(name, n, nbins))
        if c["kernel"] == "lds" and c["nvec"] == 3 * c["grid"] * c["nt"]:
            c["unrolled"] += 1
        return c

    for broken in (with_const(HIST_LDS_BINS=8193), with_const(HIST_LDS_BINS=8191), with_const(HIST_LDS_MAX_WG=128), with_const(HIST_LDS_NT=256),
                   edge_inclusive):
        with pytest.raises(AssertionError):
            check_hist(broken)


# ---------------------------------------------------------------- exact inputs
def test_gemv_exact_inputs_stay_exact_and_half_rounding_is_one_rne():
    for K in (16, 544, 2304):
        a, x = ix.gemv_exact_inputs(300, K, K)
        assert int(a.abs().max()) <= ix.GEMV_RANGE and int(x.abs().max()) <= ix.GEMV_RANGE
        assert ix.abs_sum_bound(a, x) < 1 << 24 and 16 * K < 1 << 24
        ref = ix.int_matvec(a, x)
        assert ref.dtype == torch.int64 and torch.equal(ref, (a.long() * x.long().view(1, -1)).sum(1))
        assert torch.equal(ref.float().long(), ref)  # fp32 holds the answer itself
        want = ix.half_rne(ref)
        assert torch.equal(want, ref.double().to(torch.float16))  # torch's conversion is that single rounding
        if K == 2304:  # and the rounding is exercised: some sums are no half values
            assert int((want.double() != ref.double()).sum()) > 10 and int(ref.abs().max()) < 65504
    assert max(max(v) for v in ix.GEMV_K.values()) * 16 < 1 << 24
    v = torch.tensor([2047, 2048, 2049, 2050, 2051, 4097, 4098, 4102, -2049, -2051, 36863, 65519, 0, -1])
    assert ix.half_rne(v).double().tolist() == [2047, 2048, 2048, 2050, 2052, 4096, 4096, 4104, -2048, -2052, 36864, 65504, 0, -1]


def test_sgemm_exact_inputs_stay_exact():
    for (M, N, K) in ((64, 128, 112), (64, 128, 592), (33, 68, 37)):
        a, b = ix.sgemm_exact_inputs(M, N, K, K)
        assert a.dtype == torch.float32 and torch.equal(a, a.round()) and float(a.abs().max()) <= ix.SGEMM_RANGE and float(b.abs().max()) <= ix.SGEMM_RANGE
        assert ix.abs_sum_bound(a, b) < 1 << 24
        ref = a.long() @ b.long()
        assert torch.equal((a.double() @ b.double()).long(), ref) and torch.equal(ref.float().long(), ref)  # the fp64 product is the integer one
    assert 16 * max(ix.SGEMM_KSPLIT_KS + ix.SGEMM_STAGE_KS) < 1 << 24
    assert [ix.ksplit_halves(K) for K in ix.SGEMM_KSPLIT_KS] == [(16, 16), (17, 16), (17, 17), (18, 17), (18, 18), (19, 18)]
    assert {h % 3 for K in ix.SGEMM_KSPLIT_KS for h in ix.ksplit_halves(K)} == {0, 1, 2}
    assert {ix.ksplit_halves(K)[1] % 3 for K in ix.SGEMM_KSPLIT_KS} == {0, 1, 2} == {ix.ksplit_halves(K)[0] % 3 for K in ix.SGEMM_KSPLIT_KS}
    assert ix.sgemm_impulse_k0(544, True) == [0, 15, 16, 271, 272, 543] and ix.sgemm_impulse_k0(48, False) == [0, 15, 16, 47]
    assert [K // 16 for K in ix.SGEMM_STAGE_KS] == [1, 2, 3, 4, 5, 6, 7]


def test_transpose_and_embedding_inputs_are_pairwise_distinct():
    x = ix.distinct_f32(ix.TR_BIG[0] * ix.TR_BIG[1], 3)
    assert x.dtype == torch.float32 and float(x.max()) < 1 << 24 and x.long().unique().numel() == x.numel()
    assert not torch.equal(x[:64], torch.arange(64.0))  # scrambled
    t = ix.emb_table_bits(ix.EMB_VOCAB, ix.EMB_WIDE, "float16", 1)
    assert t.dtype == torch.int16 and torch.equal(t.flatten().long().sort().values, torch.arange(-32768, 32768))  # every 16-bit pattern
    assert t.flatten()[:8].tolist() == list(ix.F16_SPECIALS)
    shapes = {(dname, emb, vocab) for name, (dname, _) in ix.EMB_RUNGS.items() for _, emb, vocab in ix.emb_small_cases(name) + ix.emb_traffic_cases(name)}
    assert len(shapes) >= 12
    for dname, emb, vocab in sorted(shapes):  # every table the GPU tests build
        t = ix.emb_table_bits(vocab, emb, dname, 2)
        assert t.shape == (vocab, emb) and t.flatten().long().unique().numel() == t.numel(), (vocab, emb, dname)
        f = t.view(torch.float32 if dname == "float32" else torch.float16)
        if t.numel() >= 8:
            tiny = 2.0 ** -126 if dname == "float32" else 2.0 ** -14
            assert bool(torch.isnan(f).any()) and bool((f == 0).any()) and bool(((f != 0) & (f.abs().double() < tiny)).any())
    idx = ix.emb_indices(1025, 9, 4)
    assert idx.dtype == torch.int32 and {-1, 9, ix.INT_MIN, ix.INT_MAX, 10} <= set(idx.tolist()) and idx[0] == 8 and idx[-1] == 0
    ref = ix.emb_reference_bits(idx, ix.emb_table_bits(9, 8, "float32", 2))
    bad = (idx < 0) | (idx >= 9)
    assert 100 < int(bad.sum()) < 200 and bool((ref[bad] == 0).all()) and bool((ref[~bad] != 0).any(dim=1).all())


def test_histogram_values_mix_every_kind_the_kernel_must_ignore():
    for nbins in (8192, 8193):
        v = ix.hist_values(5000, nbins, nbins)
        s = set(v.tolist())
        assert {-1, -nbins, nbins, nbins + 1, ix.INT_MIN, ix.INT_MAX, 0, nbins - 1} <= s
        ref = ix.hist_reference(v, nbins)
        assert ref.shape == (nbins,) and ref.dtype == torch.int64
        valid = int(((v >= 0) & (v < nbins)).sum())
        assert int(ref.sum()) == valid and 0.5 < valid / 5000 < 0.8 and int(ref[nbins // 2]) > 300
    assert ix.hist_reference(torch.tensor([-1, 8], dtype=torch.int32), 8).tolist() == [0] * 8


# ---------------------------------------------------------------- SGEMM tile forms through cln_describe (host only)
def test_sgemm_shapes_reach_every_tile_form(built):
    m = built.manifest
    for name in ix.MFMA_NAMES:
        for tile, (M, N) in ix.SGEMM_TILE_SHAPES.items():
            for K in ix.SGEMM_STAGE_KS:
                assert ix.sgemm_form(m.describe(name, (M, N, K), 2)) == (tile, False), (tile, K)
        for K in ix.SGEMM_KSPLIT_KS:
            assert ix.sgemm_form(m.describe(name, ix.SGEMM_KSPLIT_SHAPE + (K,), 3)) == ("64x128", True), K
        assert ix.sgemm_form(m.describe(name, ix.SGEMM_KSPLIT_SHAPE + (496,), 2)) == ("64x128", False)
        assert ix.sgemm_form(m.describe(name, (64, 128, 48), 2)) == ("64x128", False) and ix.sgemm_form(m.describe(name, (64, 128, 544), 2)) == ("64x128", True)
    name = ix.MFMA_NAMES[0]
    # (1792, 3584): 392 tiles of 128x128 in two rounds against 784 of 64x128 in four; one tile row or column less goes back to 64x128
    assert (1792 // 128) * (3584 // 128) == 392 and (1792 // 64) * (3584 // 128) == 784
    assert ix.sgemm_form(m.describe(name, (1792 - 128, 3584, 64), 2))[0] == "64x128" and ix.sgemm_form(m.describe(name, (1792, 3584 - 128, 64), 2))[0] == "64x128"
    # 256x128 needs an output of 8192^2: just below, the 128x128 tile
    assert ix.sgemm_form(m.describe(name, (8192, 8192 - 128, 64), 2))[0] == "128x128" and ix.sgemm_form(m.describe(name, (8192 - 256, 8192, 64), 2))[0] == "128x128"
    with pytest.raises(ValueError):
        m.describe(name, (64, 128, 8), 2)


def test_valu_and_any_shape_lists():
    for name, (BK, TN) in ix.VALU_RUNGS.items():
        cases = ix.valu_cases(name)
        assert {K // BK for _, _, K in cases} == {1, 2, 3, 5} and {M for M, _, _ in cases} == {128, 256} and {N // (16 * TN) for _, N, _ in cases} == {1, 2}
        assert all(K % BK == 0 for _, _, K in cases)
    assert {bk for bk, _ in ix.VALU_RUNGS.values()} == {8, 16} and {tn for _, tn in ix.VALU_RUNGS.values()} == {4, 8, 16}
    assert all(N % 4 == 0 for _, N, _ in ix.ANY_SHAPES) and any(M % 32 and K % 32 and N % 32 for M, N, K in ix.ANY_SHAPES)
