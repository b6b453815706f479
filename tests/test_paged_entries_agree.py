"""CPU: the siblings of a paged KV-cache entry family agree on every shape. The kernels of a family are separate bodies (one per element type,
DESIGN 4.4.6 / 4.4.8); their shape checks and plans are one definition in csrc/paged_entry.h, and this test is what notices a unit that stops
using it. Only the *_plan and *_describe entries are called: they take no pointer, so no GPU is needed.

For every point of the cross product below, every sibling of a family returns the same status, and the multi-token *_plan siblings the same
plan. The single-token decode pair is not a family: its FP8 plan has another key step, so its statuses may differ at the grid limit."""
import ctypes
import itertools

import pytest

BS = (0, 1, 3, 2 ** 24)
TS = (0, 1, 5, 9, 170, 2 ** 24, 2 ** 28)  # T, or total_q of the packed entries
HEADS = ((8, 2), (8, 8), (3, 1), (8, 3), (16, 1), (0, 1))  # (Hq, Hkv)
MAX_PAGES = (0, 6, 256, 2 ** 23)
PAGES = (0, 8, 16, 48, 256, 512)
DS = (0, 64, 96, 128)
ROPE_MODES = (-1, 0, 1, 2, 3)

# family -> (siblings, has a rope mode); every entry is cln_<name>_describe(B, T | total_q, Hq, Hkv, max_pages, page, D[, rope_mode], buf, len)
DESCRIBE = {
    "fixed-T prefill": (("fa2_prefill_paged", "fa2_prefill_paged_fp8"), False),
    "packed prefill": (("fa2_prefill_paged_varlen", "fa2_prefill_paged_varlen_bf16"), False),
    "multi-token decode": (("fa2_decode_paged_multi", "fa2_decode_paged_multi_fp8", "fa2_decode_paged_multi_bf16"), False),
    "fixed-T append": (("kv_append_paged", "kv_append_paged_fp8"), True),
    "packed append": (("kv_append_paged_varlen", "kv_append_paged_varlen_bf16"), True),
}
MULTI = DESCRIBE["multi-token decode"][0]
# the windowed multi-token decode plans, cln_<name>_plan(B, T, Hq, Hkv, max_pages, page, D, window, ...): one definition for all seven; the
# any-G forms take every Hq / Hkv in 1 ... 16 with T Hq / Hkv <= 64, and where the power-of-two forms accept they return the same plan
WINDOW_POW2 = ("fa2_decode_paged_multi_window_bf16", "fa2_decode_paged_multi_window_sink_bf16", "fa2_decode_paged_multi_window_sink_bf16_fp8")
WINDOW_ANYG = ("fa2_decode_paged_multi_window_sink_anyg_bf16", "fa2_decode_paged_multi_window_sink_anyg_bf16_fp8",
               "fa2_decode_paged_multi_window_sink_softcap_anyg_bf16", "fa2_decode_paged_multi_window_sink_softcap_anyg_bf16_fp8")
WINDOWS = (0, 1, 65, 300, 2 ** 31 - 1)


def _shapes():
    for B, T, (Hq, Hkv), mp, page, D in itertools.product(BS, TS, HEADS, MAX_PAGES, PAGES, DS):
        yield B, T, Hq, Hkv, mp, page, D


@pytest.fixture(scope="module")
def lib(built):
    from cuda_learn_notes_amd import _loader
    return ctypes.CDLL(_loader.so_path("libcln_amd.so"))


@pytest.mark.parametrize("family", sorted(DESCRIBE))
def test_describe_siblings_return_the_same_status(lib, family):
    names, has_rope = DESCRIBE[family]
    fns = []
    for n in names:
        fn = getattr(lib, "cln_%s_describe" % n)
        fn.argtypes, fn.restype = [ctypes.c_int] * (8 if has_rope else 7) + [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
        fns.append(fn)
    buf = ctypes.create_string_buffer(4096)
    calls = seen_ok = 0
    for shape in _shapes():
        for dims in ((shape + (m,) for m in ROPE_MODES) if has_rope else (shape,)):
            # a describe entry returns the length of its text, which is the sibling's own, or a negative status
            status = [min(fn(*dims, buf, 4096), 0) for fn in fns]
            assert len(set(status)) == 1, (family, dims, dict(zip(names, status)))
            calls += len(fns)
            seen_ok += status[0] == 0
    assert calls >= 2 * 16128 and seen_ok  # the whole sweep ran, and it is not a sweep of refusals only


def test_multi_plan_siblings_return_the_same_status_and_plan(lib):
    fns = []
    for n in MULTI:
        fn = getattr(lib, "cln_%s_plan" % n)
        fn.argtypes, fn.restype = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 3, ctypes.c_int
        fns.append(fn)
    seen_ok = seen_split = 0
    for dims in _shapes():
        got = []
        for fn in fns:
            s, c, w = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)  # a refusal leaves them alone, for every sibling alike
            rc = fn(*dims, ctypes.addressof(s), ctypes.addressof(c), ctypes.addressof(w))
            got.append((rc, s.value, c.value, w.value))
        assert len(set(got)) == 1, (dims, dict(zip(MULTI, got)))
        seen_ok += got[0][0] == 0
        seen_split += got[0][0] == 0 and got[0][1] > 1
    assert seen_ok and seen_split  # plans with one split and with several were compared


def test_window_plan_siblings_return_the_same_status_and_plan(lib):
    def plans(names, dims):
        got = []
        for n in names:
            fn = getattr(lib, "cln_%s_plan" % n)
            fn.argtypes, fn.restype = [ctypes.c_int] * 8 + [ctypes.c_void_p] * 3, ctypes.c_int
            s, c, w = ctypes.c_int(-7), ctypes.c_int(-7), ctypes.c_longlong(-7)
            rc = fn(*dims, ctypes.addressof(s), ctypes.addressof(c), ctypes.addressof(w))
            got.append((rc, s.value, c.value, w.value))
        return got

    seen_ok = seen_split = seen_anyg_only = 0
    for shape in _shapes():
        for W in WINDOWS:
            dims = shape + (W,)
            pow2, anyg = plans(WINDOW_POW2, dims), plans(WINDOW_ANYG, dims)
            assert len(set(pow2)) == 1, (dims, dict(zip(WINDOW_POW2, pow2)))
            assert len(set(anyg)) == 1, (dims, dict(zip(WINDOW_ANYG, anyg)))
            if pow2[0][0] == 0:  # what the power-of-two forms plan, the any-G forms plan alike
                assert anyg[0] == pow2[0], (dims, pow2[0], anyg[0])
                seen_ok += 1
                seen_split += pow2[0][1] > 1
            seen_anyg_only += anyg[0][0] == 0 and pow2[0][0] != 0
    assert seen_ok and seen_split and seen_anyg_only  # (8, 3) is no integer group; (3, 1) and (16, 1) are groups only the any-G forms take


@pytest.mark.parametrize("family", ("fa2_prefill_paged_varlen", "fa2_decode_paged_multi"))
def test_window_describe_siblings_return_the_same_status(lib, family):
    """The windowed describe entries, cln_<name>_describe(B, T | total_q, Hq, Hkv, max_pages, page, D, window[, softmax_scale, softcap], buf,
    len): one shape check per family in csrc/paged_entry.h for the power-of-two forms and one for the any-G forms (the softcap forms at the
    default scale and no cap), and what the former accept the latter accept."""
    def entries(names):
        fns = []
        for n in names:
            fn = getattr(lib, "cln_%s_describe" % n.replace("fa2_decode_paged_multi", family))
            floats = (0.0, 0.0) if "softcap" in n else ()
            fn.argtypes, fn.restype = [ctypes.c_int] * 8 + [ctypes.c_float] * len(floats) + [ctypes.c_char_p, ctypes.c_int], ctypes.c_int
            fns.append((fn, floats))
        return fns

    pow2_fns, anyg_fns = entries(WINDOW_POW2), entries(WINDOW_ANYG)
    buf = ctypes.create_string_buffer(4096)
    calls = seen_ok = seen_anyg_only = 0
    for shape in _shapes():
        for W in WINDOWS:
            dims = shape + (W,)
            # a describe entry returns the length of its text, which is the sibling's own, or a negative status
            pow2 = [min(fn(*dims, *floats, buf, 4096), 0) for fn, floats in pow2_fns]
            anyg = [min(fn(*dims, *floats, buf, 4096), 0) for fn, floats in anyg_fns]
            assert len(set(pow2)) == 1, (dims, dict(zip(WINDOW_POW2, pow2)))
            assert len(set(anyg)) == 1, (dims, dict(zip(WINDOW_ANYG, anyg)))
            if pow2[0] == 0:
                assert anyg[0] == 0, (dims, anyg[0])
                seen_ok += 1
            seen_anyg_only += anyg[0] == 0 and pow2[0] != 0
            calls += len(pow2) + len(anyg)
    assert calls == 7 * 16128 * len(WINDOWS) and seen_ok and seen_anyg_only  # the whole sweep ran, and it is not a sweep of refusals only
