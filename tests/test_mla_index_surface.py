"""CPU: the DSA indexer (include/cln_amd_ext.h: cln_kv_append_paged_index_bf16, cln_mla_index_logits_paged_bf16, cln_mla_index_topk with
their describe entries; csrc/kv_append_paged_index_bf16.*, csrc/mla_index_logits_paged_bf16.*, csrc/mla_index_topk.*) -- the
top-k reference against a brute-force definition, the logits reference against the two wrong readings of the ReLU, the exact case's
partial sums, a model of the top-k kernel with named faults against the long rows and the old ones, what the case builders claim (where the
tie class starts and krem is cut, which blocks hold winners, the row residues, the wraps of the large rows, the append edges), header, exports and package, every status that returns before a device call in its documented order, the Python entries'
refusals, the describe texts against their manifest mirrors and the kernels' resources in the built library. No GPU needed."""
import ctypes
import glob
import os
import random
import re
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "cln_amd_ext.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mla_index_reference as ix  # noqa: E402
import test_paged_bf16_fp8_surface as fs  # noqa: E402  (the sibling surface test's readers of the built library)

APPEND, LOGITS, TOPK = "cln_kv_append_paged_index_bf16", "cln_mla_index_logits_paged_bf16", "cln_mla_index_topk"
NAMES = (APPEND, APPEND + "_describe", LOGITS, LOGITS + "_describe", TOPK, TOPK + "_describe")
UNITS = ("kv_append_paged_index_bf16", "mla_index_logits_paged_bf16", "mla_index_topk")
I, LL, VP = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
APPEND_ARGS = [VP] * 5 + [I] * 5 + [VP]
LOGITS_ARGS = [VP] * 6 + [I] * 3 + [LL] + [I] * 3 + [VP]
TOPK_ARGS = [VP] * 3 + [I] * 2 + [LL, I, VP]
BF = torch.bfloat16
_fn = fs._fn


# ---------------------------------------------------------------------------------------------------- the references

def test_topk_reference_is_the_brute_force_definition():
    """A few hundred tiny rows with heavy ties, +-0 and +-inf among them."""
    rnd = random.Random(5)
    pick = [0.0, -0.0, 1.0, 1.0, -1.0, 2.5, float("inf"), float("-inf"), 1e-45, -1e-45]
    n_sel = 0
    for _ in range(400):
        n, topk = rnd.randint(0, 24), rnd.randint(1, 12)
        vals = torch.tensor([rnd.choice(pick) for _ in range(n)], dtype=torch.float32)
        want = ix.topk_brute(vals.tolist(), topk)
        assert ix.topk_row(vals, topk).tolist() == want, (vals, topk)
        n_sel += n > topk
    assert n_sel > 100
    lg = torch.tensor([[[3.0, 1.0, 3.0, 2.0, 9.0, 9.0]]])
    assert ix.topk_ref(lg, [5], 2).tolist() == [[[0, 4]]] and ix.topk_ref(lg, [5], 3).tolist() == [[[0, 2, 4]]]  # position 5 is not visible
    assert ix.topk_ref(lg, [9], 2).tolist() == [[[4, 5]]] and ix.topk_ref(lg, [2], 4).tolist() == [[[0, 1, -1, -1]]]


@pytest.mark.parametrize("case", [("one",) + ht + (16,) for ht in ix.ONE_HT + ix.ONE_HT_MORE] + [("long",)], ids=lambda c: "-".join(str(x) for x in c))
def test_the_gpu_cases_would_notice_a_missing_or_a_misplaced_relu(case):
    """For every random-data case of tests/test_gpu_mla_index.py the reference without the ReLU, and with the ReLU applied after the head
    sum, lies more than 20 x the bound from the true reference at some position."""
    q, w, (pool, bt), lens, ld = (ix.one_case if case[0] == "one" else ix.long_case)(*case[1:])
    ref, bound, vis = ix.reference(*case)
    fin = torch.isfinite(ref)
    assert int(fin.sum()) == sum(max(v, 0) for row in vis for v in row) > 0
    for wrong in ("none", "after"):
        other = ix.logits_ref(q, w, pool, bt, lens, ld, relu=wrong)[0]
        far = ((other[fin] - ref[fin]).abs() > 20 * bound[fin])
        print("mla index %s relu=%s: %d of %d positions farther than 20 x bound" % (case, wrong, int(far.sum()), int(fin.sum())))
        assert bool(far.any())


def test_exact_case_stays_below_two_to_the_24():
    for args in ((64, 3, 16), (17, 3, 16), (48, 3, 16), (33, 3, 16), (49, 3, 16)):
        q, w, (pool, bt), lens, ld = ix.exact_case(*args)
        _, bound, _ = ix.logits_ref(q, w, pool, bt, lens, ld)
        a = bound / (ix.EPS_TERMS * 2.0 ** -23)  # A = sum_h |w_h| sum_d |q k|: above every partial sum
        assert 0 < float(a.max()) * 4 < 2 ** 24  # in units of the smallest weight, 1/4
        assert bool(((w.abs().log2() % 1) == 0).all()) and float(w.abs().min()) == 0.25 and float(w.abs().max()) == 4 and bool((w < 0).any())


def test_pool_builder_poisons_every_unlisted_row():
    q, w, (pool, bt), lens, ld = ix.one_case(17, 3, 16)
    listed = torch.zeros(pool.shape[:2], dtype=torch.bool)
    for b, n in enumerate(lens):
        for j in range(n):
            listed[int(bt[b, j // 16]), j % 16] = True
    assert bool(torch.isfinite(pool[listed].float()).all()) and bool(torch.isnan(pool[~listed].float()).all()) and int((~listed).sum()) > 16
    for b, n in enumerate(lens):
        assert all(bool(torch.isnan(pool[int(p)].float()).all()) for p in bt[b, -(-n // 16):])


# ---------------------------------------------------------------------------------------------------- the long rows bite

def _long_rows(block=ix.SCAN_BLOCK, kinds=ix.LONG_KINDS, prod=True):
    """Every (kind, n, topk, vals, facts) of tests/test_gpu_mla_index_long_rows.py (block = 4096), or their shortened versions."""
    for kind in kinds:
        for topk in ix.long_topks(block):
            for n in ix.long_ns(block) + ([ix.PROD_N] if prod and block == ix.SCAN_BLOCK and topk == 2048 else []):
                row = ix.long_row(kind, n, topk, block)
                if row is not None:
                    yield kind, n, topk, row[0], row[1]


def _wrong(vals, topk, want, fault, block=ix.SCAN_BLOCK):
    got, info = ix.topk_model(vals, topk, fault=fault, block=block)
    return not torch.equal(got, want) or bool(info["spill"])


@pytest.mark.parametrize("kind", ix.LONG_KINDS)
def test_long_rows_hold_what_their_builders_claim_and_the_model_is_the_reference(kind):
    """With fault=None the model of the kernel's three steps equals topk_ref on every long row, and every row has the property its recipe
    states: where the winners lie, where the threshold's tie class starts and where krem is cut, how many blocks the pass runs."""
    B = ix.SCAN_BLOCK
    seen = set()
    for _, n, topk, x, facts in _long_rows(kinds=[kind]):
        want = ix.topk_row(x, topk)
        got, info = ix.topk_model(x, topk)
        assert torch.equal(got, want) and not info["spill"], (kind, n, topk)
        assert torch.equal(ix.topk_ref(ix.long_logits(kind, n, topk, ld=max(n, ix.LONG_TOPK_LD))[0], [n], topk)[0, 0], want)
        keys, prefix, krem = info["keys"], info["prefix"], info["krem"]
        gt, eq = (keys > prefix), (keys == prefix)
        assert int(gt.sum()) + krem == topk and int(eq.sum()) >= krem
        cut = int(eq.nonzero()[krem - 1])  # the last tie taken
        blocks_with_winners = sorted(set((want.long() // B).tolist()))
        seen.add((n, topk))
        if "selected" in facts:
            assert torch.equal(facts["selected"].to(torch.int32), want), (kind, n, topk)
        if kind == "late":
            assert int(want.min()) >= facts["from"] and int(want[-1]) == n - 1 and info["blocks"] == info["nblocks"] >= 2
            assert facts["from"] == (n - 1) // B * B or n - (n - 1) // B * B <= topk  # the last block, unless it is too short for topk
        elif kind == "early":
            assert int(want.max()) < facts["to"] and info["blocks"] <= -(-facts["to"] // B) and blocks_with_winners[0] == 0
            assert (topk <= B and blocks_with_winners == [0]) or (topk > B and blocks_with_winners == [0, 1])
            assert info["blocks"] < info["nblocks"] or n <= facts["to"]  # the break fires with whole blocks left
        elif kind == "straddle":
            first = int(eq.nonzero()[0])
            assert first < B and bool(eq[3 * B:].any()) and int(eq[:2 * B].sum()) == 2 * facts["e"] < krem  # starts in block 0, runs past 3 B
            assert 2 * B < cut < 3 * B - 1 and bool(eq[cut + 1:3 * B].any())                         # krem is cut strictly inside block 2
            assert all(int(gt[b * B:min((b + 1) * B, cut)].sum()) > 0 for b in range(3)) and not bool(gt[3 * B:].any())
            assert info["blocks"] == 3 < info["nblocks"]
        elif kind == "spread":
            full = range(min(info["blocks"], n // B))  # a ragged last block may hold one position
            assert all(bool(eq[b * B:(b + 1) * B].any()) for b in full)
            if topk >= 2048 and n < ix.PROD_N:
                assert all(bool(gt[b * B:(b + 1) * B].any()) for b in full) and info["blocks"] >= 2
        else:
            span = B // ix.WAVES
            p = want.long()
            cand = (p % span == 0) | (p % span == span - 1) | (p % 4 == 3)
            assert int(cand.sum()) == min(topk, facts["candidates"]) and (topk < 16 * 2 * info["nblocks"] or blocks_with_winners == list(range(info["nblocks"])))
    print("%s: %d rows" % (kind, len(seen)))
    # 2 ... 6 blocks and the production row of 32, topk 4097 and 6000 among them
    assert {n for n, _ in seen} >= set(ix.long_ns()[4 if kind == "straddle" else 0:]) | {ix.PROD_N} and {4097, 6000} <= {k for _, k in seen}


def test_model_is_the_brute_force_definition_on_shortened_long_rows():
    """The same recipes at a scan block of 256 positions (rows of 511 ... 1281, topk 1 ... 375): the model equals topk_brute."""
    count = 0
    for kind, n, topk, x, _ in _long_rows(block=256):
        got, info = ix.topk_model(x, topk, block=256)
        assert got.tolist() == ix.topk_brute(x.tolist(), topk), (kind, n, topk)
        count += 1
    assert count > 150


def test_every_harmful_fault_of_the_model_changes_a_long_row_and_the_old_rows_miss_the_block_faults():
    """Each named fault of topk_model, on the long rows of tests/test_gpu_mla_index_long_rows.py and on the rows the suite had before
    (topk_case, n <= 5000: two scan blocks at the most). Every harmful fault changes the list of a long row; the two harmless ones change
    none anywhere (the break is an optimisation; the slot clip cannot bite on a row that holds still: topk_model's docstring). The old rows
    see none of the faults that need a third block -- a count buffer used a second time, a pass that ends after two blocks, a carry that
    forgets the blocks in front of the previous one: the gap the long rows close."""
    faults = ix.FAULTS_HARMFUL + ix.FAULTS_HARMLESS
    new = {f: [] for f in faults}
    for kind, n, topk, x, _ in _long_rows():
        want = ix.topk_row(x, topk)
        for f in faults:
            if _wrong(x, topk, want, f):
                new[f].append((kind, n, topk))
    old = {f: 0 for f in faults}
    rows = 0
    for x, topk, _ in ix.old_topk_rows():
        want = ix.topk_row(x, topk)
        rows += 1
        for f in faults:
            old[f] += _wrong(x, topk, want, f)
    for f in faults:
        print("fault %-24s wrong on %3d long rows (by kind: %s), on %3d of the %d old rows"
              % (f, len(new[f]), {k: sum(c[0] == k for c in new[f]) for k in ix.LONG_KINDS}, old[f], rows))
    assert all(new[f] for f in ix.FAULTS_HARMFUL) and not any(new[f] or old[f] for f in ix.FAULTS_HARMLESS)
    assert rows >= 100 and old["stale_counts"] == 0 and old["stop_after_two_blocks"] == 0 and old["no_carry_gt"] == 0 and old["no_carry_eq"] == 0
    assert old["ties_last"] > 0  # the old rows were not blind: what two blocks can show, they showed
    # every kind but one catches a fault; "early" cannot (its list is complete after block 0 or 1, where the old rows already look): it is
    # there to take the break with whole blocks left, which no fault of a model can stand for -- the kernel either leaves the loop or hangs
    assert all(any(c[0] == k for f in ix.FAULTS_HARMFUL for c in new[f]) == (k != "early") for k in ix.LONG_KINDS)
    assert any(c[0] == "straddle" for c in new["no_carry_eq"]) and any(c[0] == "late" for c in new["stale_counts"])
    assert any(topk > ix.SCAN_BLOCK for _, _, topk in new["stop_after_two_blocks"])


def test_align_rows_start_at_every_residue():
    """fp32 rows of ld = 4101 or 4103 elements start at 0, 4, 8 and 12 bytes past a 16-byte boundary within six rows; ld = 4102 gives 0 and 8,
    and 4 and 12 when the tensor itself starts 4 bytes in; the lengths make n = 4097, 4100 and ld occur."""
    for ld in ix.ALIGN_LDS:
        res, res4 = set(ix.row_residues(ld)), set(ix.row_residues(ld, base=4))
        assert res | res4 == {0, 4, 8, 12}
        assert (res == {0, 4, 8, 12} == res4) if ld % 2 else (res == {0, 8} and res4 == {4, 12})
        ns = set()
        for which in (0, 1):
            x, lens = ix.align_case(ld, "ties", which)
            vis = ix.visible(lens, ix.ALIGN_T, ld)
            ns |= {v for row in vis for v in row}
            for b in range(ix.ALIGN_B):
                for t in range(ix.ALIGN_T):
                    assert bool(torch.isnan(x[b, t, vis[b][t]:]).all()) and not bool(torch.isnan(x[b, t, :vis[b][t]]).any())
        assert {4097, 4100, ld} <= ns, (ld, sorted(ns))


def test_large_rows_wrap_into_the_empty_row():
    """tests/test_gpu_mla_index_large_rows.py: with ld = 2^30 + 1 a row start whose byte offset or element offset wraps at 32 bits lands in
    the window of row 0, whose sequence is empty; no live row is the image of another."""
    ld, Nmax = ix.ROWS_LD, ix.ROWS_NMAX
    assert ix.ROWS_LENS[0] == 0 and 4 * ld > 2 ** 32 and 2 * ld > 2 ** 31 and 4 * ld > 2 ** 32
    for r in range(1, 5):
        assert r * ld == r * 2 ** 30 + r
        for image in ix.row_start_wraps(r):
            assert image == r * ld or (0 <= image and image + Nmax <= Nmax + 8), (r, image)
        assert any(image != r * ld for image in ix.row_start_wraps(r))
    assert ix.row_start_wraps(4)[1] == 4 and ix.row_start_wraps(1) == (1, ld)
    x, lens = ix.rows_topk_case()
    for b, n in enumerate(lens):
        if n > 64:
            assert ix.topk_row(x[b, 0, :n], 64).tolist() != list(range(64))


@pytest.mark.parametrize("name", ix.APPEND_CASES)
def test_append_problems_are_the_edges_they_claim(name):
    p = ix.append_problem(name)
    page, P, bt, lens, cu, k_new, new = (p[k] for k in ("page", "P", "bt", "lens", "cu", "k_new", "new"))
    c, Ts = ix.append_clamped(cu, k_new.shape[0])
    assert Ts == new and c[0] >= 0 and c[-1] <= k_new.shape[0]
    Nmax = bt.shape[1] * page
    pool = torch.full((P, page, ix.D), 0, dtype=torch.int16).fill_(ix.MARK).view(BF)
    want = ix.append_ref(pool, bt, lens, cu, k_new)
    written = int((want.view(torch.int16) != pool.view(torch.int16)).any(dim=-1).sum())
    live = sum(1 for b, t in enumerate(Ts) for i in range(t)
               if 0 <= lens[b] - t + i < Nmax and 0 <= int(bt[b, (lens[b] - t + i) // page]) < P)
    assert written == live > 0
    dropped = sum(Ts) - live
    assert (dropped > 0) == (name in ("short_len", "past_nmax", "bad_entries")), (name, dropped)
    if name == "empties":
        assert new == [0, 3, 0, 0, 20, 0]
    if name == "cu_outside":
        assert cu[0] < 0 and cu[-1] > k_new.shape[0]
    if name == "bad_entries":
        assert sorted(int(v) for v in bt.flatten() if not 0 <= int(v) < P) == [-1, P]
    if name == "b37":
        assert len(new) == 37 and sum(t > 0 for t in new) == 5


# ---------------------------------------------------------------------------------------------------- header, exports

@pytest.mark.parametrize("lang,cc", [("c", "gcc"), ("c++", "g++")])
def test_ext_header_compiles_with_the_six_prototypes(tmp_path, lang, cc):
    assert shutil.which(cc), cc
    protos = ("const void*, void*, const int*, const int*, const int*, int, int, int, int, int, void*", "int, int, int, int, char*, int",
              "const void*, const float*, const void*, const int*, const int*, float*, int, int, int, long long, int, int, int, void*",
              "int, int, int, long long, int, int, char*, int", "const float*, const int*, int*, int, int, long long, int, void*",
              "int, int, long long, int, char*, int")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "cln_amd_ext.h"\n' + "".join("int (*f%d)(%s) = %s;\n" % (i, p, n) for i, (p, n) in enumerate(zip(protos, NAMES)))
                   + "int main(void) { return f0 && f1 && f2 && f3 && f4 && f5 ? 0 : 1; }\n")
    r = subprocess.run([cc, "-x", lang, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HDR), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_header_manifest_package_host_and_build_hold_the_entries(built):
    lib, hdr = fs._lib(), open(HDR).read()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\bint %s\(" % n, hdr), n
    from cuda_learn_notes_amd import host
    for n in (APPEND, LOGITS, TOPK):
        assert hasattr(built, n[4:]) and hasattr(host, n[4:]), n
        assert hasattr(built.manifest, "describe_" + n[4:]), n
    build = open(os.path.join(ROOT, "cuda-learn-notes_amd", "_build.py")).read()
    for u in UNITS:
        assert '"%s.hip"' % u in build and all(os.path.exists(os.path.join(fs.CSRC, u + e)) for e in (".hip", ".cuh")), u


# ---------------------------------------------------------------------------------------------------- statuses

def _ptrs(n):
    buf = (ctypes.c_char * (256 * (n + 1)))()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    return buf, [base + 256 * i for i in range(n)]


def test_logits_statuses_in_their_order(built):
    """Pointers (q_idx, idx_pool 16 bytes; weights, block_table, seqlens, logits 4), output equal to an input, P, non-positive dimensions,
    then the -2s. Nothing is launched before a refusal."""
    fn = _fn(LOGITS, LOGITS_ARGS)
    keep, (q, w, pool, bt, sl, lg) = _ptrs(6)
    dims = (2, 3, 64, 320, 5, 20, 16)  # B, T, Hi, ld, P, max_pages, page
    call = lambda *a, d=dims: fn(*a, *d, None)  # noqa: E731
    for i in range(6):  # a missing pointer, ahead of an unsupported shape
        args = [q, w, pool, bt, sl, lg]
        args[i] = None
        assert call(*args) == -1 and call(*args, d=(2, 3, 65, 320, 5, 20, 16)) == -1, i
    for i, off in ((0, 8), (1, 2), (2, 8), (3, 2), (4, 2), (5, 2)):  # misaligned, one by one
        args = [q, w, pool, bt, sl, lg]
        args[i] += off
        assert call(*args) == -1, i
    # 4-byte aligned operands that are not 16-byte aligned pass the pointer check: the next refusal is P's, then the shape's
    assert call(q, w + 4, pool, bt + 4, sl + 4, lg + 4, d=(2, 3, 64, 320, 0, 20, 16)) == -1
    assert call(q, w + 4, pool, bt + 4, sl + 4, lg + 4, d=(2, 3, 65, 320, 5, 20, 16)) == -2
    for i in range(5):  # the output equal to an input
        args = [q, w, pool, bt, sl, lg]
        args[5] = args[i]
        assert call(*args, d=(2, 3, 65, 320, 5, 20, 16)) == -1, i
    assert call(q, w, pool, bt, sl, lg, d=(2, 3, 65, 320, 0, 20, 16)) == -1 and call(q, w, pool, bt, sl, lg, d=(2, 3, 65, 320, -1, 20, 48)) == -1  # P first
    for d in ((0, 3, 64, 320, 5, 20, 16), (2, 0, 64, 320, 5, 20, 16), (2, 3, 0, 320, 5, 20, 16), (2, 3, 64, 0, 5, 20, 16), (2, 3, 64, 320, 5, 0, 16),
              (2, 3, 64, 320, 5, 20, 0), (2, -1, 65, 320, 5, 20, 48)):
        assert call(q, w, pool, bt, sl, lg, d=d) == -1, d
    for d in ((2, 3, 65, 320, 5, 20, 16), (2, 3, 64, 320, 5, 20, 48), (2, 3, 64, 320, 5, 20, 8), (2, 3, 64, 320, 5, 20, 512),
              (2, 3, 64, 320, 5, 1 << 23, 256), (1 << 16, 1 << 15, 64, 320, 5, 20, 16), (1 << 12, 1 << 12, 64, 1 << 20, 5, 1 << 22, 256)):
        assert call(q, w, pool, bt, sl, lg, d=d) == -2, d  # Hi, the page, max_pages page, B T, the grid
    dsc = _fn(LOGITS + "_describe", [I, I, I, LL, I, I, ctypes.c_char_p, I])
    buf = ctypes.create_string_buffer(4096)
    assert dsc(2, 3, 64, 320, 20, 16, None, 4096) == -1 and dsc(2, 3, 64, 320, 20, 16, buf, 0) == -1
    assert dsc(2, 3, 65, 320, 20, 16, buf, 4096) == -2 and dsc(2, 3, 64, 0, 20, 16, buf, 4096) == -1 and dsc(2, 3, 64, 1 << 40, 20, 16, buf, 4096) > 0


def test_topk_statuses_in_their_order(built):
    fn = _fn(TOPK, TOPK_ARGS)
    keep, (lg, sl, ix_) = _ptrs(3)
    call = lambda *a, d=(2, 3, 320, 64): fn(*a, *d, None)  # noqa: E731
    for i in range(3):
        args = [lg, sl, ix_]
        args[i] = None
        assert call(*args) == -1 and call(*args, d=(2, 3, 1 << 31, 64)) == -1, i
        args = [lg, sl, ix_]
        args[i] += 2
        assert call(*args) == -1, i
    assert call(lg, sl, lg) == -1 and call(lg, sl, sl) == -1  # indices aliasing an input
    assert call(lg + 4, sl + 4, ix_ + 4, d=(2, 3, 320, 0)) == -1  # 4-byte aligned operands pass the pointer check
    for d in ((0, 3, 320, 64), (2, 0, 320, 64), (2, 3, 0, 64), (2, 3, 320, 0), (2, 3, 320, -4), (2, 3, -1, 64), (0, 3, 1 << 31, 64)):
        assert call(lg, sl, ix_, d=d) == -1, d
    for d in ((2, 3, 1 << 31, 64), (1 << 16, 1 << 15, 320, 64), (1 << 15, (1 << 16) - 1, 320, (1 << 31) - 1), (1 << 12, 1 << 10, 320, 64)):
        assert call(lg, sl, ix_, d=d) == -2, d  # ld, B T, topk B T, the grid (B T 1024 = 2^32)
    dsc = _fn(TOPK + "_describe", [I, I, LL, I, ctypes.c_char_p, I])
    buf = ctypes.create_string_buffer(4096)
    assert dsc(2, 3, 320, 64, None, 4096) == -1 and dsc(2, 3, 1 << 31, 64, buf, 4096) == -2 and dsc(2, 3, (1 << 31) - 1, 64, buf, 4096) > 0
    assert dsc(1 << 12, (1 << 10) - 1, 320, 64, buf, 4096) > 0


def test_append_statuses_in_their_order(built):
    fn = _fn(APPEND, APPEND_ARGS)
    keep, (kn, pool, bt, sl, cu) = _ptrs(5)
    call = lambda *a, d=(2, 7, 5, 20, 16): fn(*a, *d, None)  # noqa: E731  B, total_q, P, max_pages, page
    for i in range(5):
        args = [kn, pool, bt, sl, cu]
        args[i] = None
        assert call(*args) == -1 and call(*args, d=(2, 7, 5, 20, 48)) == -1, i
    for i, off in ((0, 8), (1, 8), (2, 2), (3, 2), (4, 2)):
        args = [kn, pool, bt, sl, cu]
        args[i] += off
        assert call(*args) == -1, i
    for i in (0, 2, 3, 4):  # the pool equal to an input
        args = [kn, pool, bt, sl, cu]
        args[1] = args[i]
        assert call(*args) == -1, i
    assert call(kn, pool, bt + 4, sl + 4, cu + 4, d=(2, 7, 0, 20, 48)) == -1 and call(kn, pool, bt + 4, sl + 4, cu + 4, d=(2, 7, 5, 20, 48)) == -2
    for d in ((0, 7, 5, 20, 16), (2, 0, 5, 20, 16), (2, 7, 5, 0, 16), (2, 7, 5, 20, 0)):
        assert call(kn, pool, bt, sl, cu, d=d) == -1, d
    for d in ((2, 7, 5, 20, 48), (2, 7, 5, 20, 8), (2, 7, 5, 1 << 23, 256)):
        assert call(kn, pool, bt, sl, cu, d=d) == -2, d


# ---------------------------------------------------------------------------------------------------- describe texts

def test_describe_texts_equal_their_manifest_mirrors(built):
    m = built.manifest
    buf = ctypes.create_string_buffer(4096)
    dl = _fn(LOGITS + "_describe", [I, I, I, LL, I, I, ctypes.c_char_p, I])
    for B, T, Hi, ld, mp, page in ((64, 1, 64, 131072, 2048, 64), (8, 3, 17, 320, 20, 16), (1, 2048, 1, 5000, 64, 64), (4, 4, 33, 100, 20, 16)):
        rc = dl(B, T, Hi, ld, mp, page, buf, 4096)
        text = buf.value.decode()
        cap = min(mp * page, ld)
        chunks = -(-cap // ix.CHUNK)
        assert rc == len(text) and text == m.describe_mla_index_logits_paged_bf16(B, T, Hi, ld, mp, page)
        assert text.startswith("mla_index_logits_paged_bf16_mfma<NHB=%d> T=%d Hi=%d ld=%d cap=%d page=%d: " % (-(-Hi // 16), T, Hi, ld, cap, page))
        assert "%d workgroups of 4 waves" % (B * T * chunks) in text and "chunk of 1024 keys; %d chunks a token" % chunks in text
        assert "v_mfma_f32_16x16x32_bf16, %d MFMAs per block" % (4 * -(-Hi // 16)) in text and "%d padding heads" % (-Hi % 16) in text
        assert "no LDS" in text and "nothing else" in text and text.endswith("; deterministic") and "_f16" not in text
    dt = _fn(TOPK + "_describe", [I, I, LL, I, ctypes.c_char_p, I])
    for B, T, ld, topk in ((64, 1, 131072, 2048), (3, 5, 300, 1)):
        rc = dt(B, T, ld, topk, buf, 4096)
        text = buf.value.decode()
        assert rc == len(text) and text == m.describe_mla_index_topk(B, T, ld, topk)
        assert text.startswith("mla_index_topk_rows T=%d ld=%d topk=%d: " % (T, ld, topk)) and "%d workgroups of 1024 threads" % (B * T) in text
        assert "blocks of %d positions" % ix.SCAN_BLOCK in text and "no global atomics" in text and text.endswith("; deterministic")
    for B, tq, mp, page in ((64, 64, 2048, 64), (3, 100, 20, 16)):
        rc, text = fs._describe(APPEND + "_describe", B, tq, mp, page)
        assert rc == len(text) and text == m.describe_kv_append_paged_index_bf16(B, tq, mp, page)
        assert text.startswith("kv_append_paged_index_bf16_rows B=%d total_q=%d page=%d: " % (B, tq, page)) and "Hadamard" in text
        assert "%d workgroups of 256 threads (16 packed rows each" % (-(-tq // 16)) in text
    with pytest.raises(ValueError, match="status -2"):
        m.describe_mla_index_logits_paged_bf16(1, 1, 65, 320, 20, 16)
    with pytest.raises(ValueError, match="status -1"):
        m.describe_mla_index_topk(1, 1, 320, 0)
    with pytest.raises(ValueError, match="status -2"):
        m.describe_kv_append_paged_index_bf16(1, 1, 20, 48)


# ---------------------------------------------------------------------------------------------------- the Python entries

def test_python_entries_refuse_bad_tensors_before_any_device_call(built, monkeypatch):
    """No GPU: the device check is replaced, and a call that gets as far as the C entry shows it by raising Reached."""
    from cuda_learn_notes_amd import host

    class Reached(Exception):
        pass

    def reached(name, argtypes):
        raise Reached(name)

    with pytest.raises(RuntimeError, match="expected a GPU"):
        built.mla_index_topk(torch.zeros(2, 3, 320), torch.zeros(2, dtype=torch.int32), 64, torch.zeros(2, 3, 64, dtype=torch.int32))
    monkeypatch.setattr(host, "_check_dev", lambda *ts: None)
    b = lambda *sh: torch.zeros(*sh, dtype=BF)  # noqa: E731
    f = lambda *sh: torch.zeros(*sh, dtype=torch.float32)  # noqa: E731
    i = lambda *sh: torch.zeros(*sh, dtype=torch.int32)  # noqa: E731
    good = dict(q_idx=b(2, 3, 17, 128), weights=f(2, 3, 17), idx_pool=b(5, 16, 128), block_table=i(2, 20), seqlens=i(2), logits=f(2, 3, 320))
    lg = lambda **kw: built.mla_index_logits_paged_bf16(**{**good, **kw})  # noqa: E731
    for kw in (dict(q_idx=good["q_idx"].half()), dict(weights=good["weights"].double()), dict(idx_pool=good["idx_pool"].float()),
               dict(block_table=torch.zeros(2, 20, dtype=torch.int64)), dict(seqlens=torch.zeros(2, dtype=torch.int64)), dict(logits=good["logits"].half())):
        with pytest.raises(RuntimeError, match="values must be"):
            lg(**kw)
    with pytest.raises(RuntimeError, match="q_idx of 64 dims not supported"):
        lg(q_idx=b(2, 3, 17, 64))
    for kw in (dict(idx_pool=b(5, 16, 64)), dict(weights=f(2, 3, 16)), dict(weights=f(2, 3)), dict(seqlens=i(3)), dict(block_table=i(3, 20)),
               dict(logits=f(2, 2, 320)), dict(logits=f(6, 320)), dict(q_idx=b(6, 17, 128)), dict(idx_pool=b(80, 128))):
        with pytest.raises(RuntimeError, match="size mismatch"):
            lg(**kw)
    with pytest.raises(RuntimeError, match="65 index heads not supported"):
        lg(q_idx=b(2, 3, 65, 128), weights=f(2, 3, 65))
    with pytest.raises(RuntimeError, match="page size 48"):
        lg(idx_pool=b(5, 48, 128))
    tk = lambda **kw: built.mla_index_topk(**{**dict(logits=f(2, 3, 320), seqlens=i(2), topk=64, indices=i(2, 3, 64)), **kw})  # noqa: E731
    for kw in (dict(logits=f(2, 3, 320).half()), dict(seqlens=torch.zeros(2, dtype=torch.int64)), dict(indices=torch.zeros(2, 3, 64, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="values must be"):
            tk(**kw)
    for kw in (dict(indices=i(2, 3, 63)), dict(indices=i(2, 2, 64)), dict(indices=i(6, 64)), dict(seqlens=i(3)), dict(logits=f(6, 320)), dict(topk=65)):
        with pytest.raises(RuntimeError, match="size mismatch"):
            tk(**kw)
    ap = lambda **kw: built.kv_append_paged_index_bf16(**{**dict(k_idx_new=b(7, 128), idx_pool=b(5, 16, 128), block_table=i(2, 20), seqlens=i(2),  # noqa: E731
                                                               cu_q=i(3)), **kw})
    for kw in (dict(k_idx_new=b(7, 128).half()), dict(cu_q=torch.zeros(3, dtype=torch.int64))):
        with pytest.raises(RuntimeError, match="values must be"):
            ap(**kw)
    for kw in (dict(k_idx_new=b(7, 64)), dict(k_idx_new=b(7, 1, 128)), dict(idx_pool=b(5, 16, 576)), dict(seqlens=i(3)), dict(cu_q=i(2))):
        with pytest.raises(RuntimeError, match="size mismatch"):
            ap(**kw)
    with pytest.raises(RuntimeError, match="page size 48"):
        ap(idx_pool=b(5, 48, 128))
    with pytest.raises(TypeError):
        built.kv_append_paged_index_bf16(b(7, 128), b(5, 16, 128), i(2, 20), i(2), i(3), None)  # there is no rope argument
    monkeypatch.setattr(host, "_ext_fn", reached)  # a good call reaches the C entry
    for name, call in ((LOGITS, lg), (TOPK, tk), (APPEND, ap)):
        with pytest.raises(Reached, match=name):
            call()


# ---------------------------------------------------------------------------------------------------- registers and LDS

def _built_kernels(tmp_path):
    """{kernel name: metadata} of the indexer's kernels in the gfx950 code objects inside the built product library."""
    from cuda_learn_notes_amd import _loader
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    assert os.path.exists(objdump) and os.path.exists(readelf)
    local = str(tmp_path / "libcln_amd.so")
    shutil.copy(_loader.so_path("libcln_amd.so"), local)
    subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=str(tmp_path))
    out = {}
    for co in sorted(glob.glob(local + ".*gfx950")):
        notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
        if "mla_index" not in notes and "paged_index" not in notes:
            continue
        for blk in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            out[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, "- .agpr_count" + blk).group(1))
                         for k in ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                                   "group_segment_fixed_size")}
    return out


def test_kernel_resources_in_the_built_library(built, tmp_path):
    """No spill, no scratch; the logits kernels take no LDS and fit two workgroups a CU (__launch_bounds__(256, 2): at most 256 registers);
    the top-k kernel takes the 1288 bytes its describe text states."""
    got = _built_kernels(tmp_path)
    logits = sorted((n, k) for n, k in got.items() if "mla_index_logits_paged_bf16_mfma" in n)
    topk = [(n, k) for n, k in got.items() if "mla_index_topk_rows" in n]
    append = [(n, k) for n, k in got.items() if "kv_append_paged_index_bf16_rows" in n]
    assert len(logits) == 4 and len(topk) == 1 and len(append) == 1, sorted(got)
    for n, k in logits + topk + append:
        print(n, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
    for nhb, (n, k) in enumerate(logits, 1):
        assert "ILi%dE" % nhb in n and k["vgpr_count"] <= 256 and k["group_segment_fixed_size"] == 0, (n, k)
    assert topk[0][1]["group_segment_fixed_size"] == 1288 and "1288 bytes of LDS" in built.manifest.describe_mla_index_topk(1, 1, 320, 64)
    assert topk[0][1]["vgpr_count"] <= 128 and append[0][1]["group_segment_fixed_size"] == 0


def test_logits_kernel_mfmas(tmp_path):
    """The loop's MFMAs per wave and block of 16 keys: 4 k-steps per block of 16 heads, all bf16 16x16x32; no LDS instruction at all."""
    got = fs._bodies("mla_index_logits_paged_bf16.hip", tmp_path)  # asserts no spill, no scratch, no atomics
    assert len(got) == 4, [k["name"] for k, _ in got]
    for k, body in got:
        nhb = int(re.search(r"mfmaILi(\d)E", k["name"]).group(1))
        print(k["name"], {x: k.get(x) for x in ("vgpr", "agpr", "sgpr", "lds")})
        assert fs._loop_mfmas(body) == 4 * nhb and k["lds"] == 0
        assert "v_mfma" not in body.replace("v_mfma_f32_16x16x32_bf16", "") and "ds_" not in body and "v_readlane_b32" in body
