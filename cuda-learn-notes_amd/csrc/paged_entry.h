// The host side of the paged KV-cache entries (cln_kv_append_paged*, cln_fa2_prefill_paged*, cln_fa2_decode_paged*; DESIGN 4.4.6, 4.4.8 - 4.4.10,
// 4.4.16): one definition of every argument check, shape check, plan and compile-time dispatch that the 24 compile units share. Host code only -- the kernels
// are siblings, one body per element type, for the measured reason given there; nothing here can change a kernel's schedule. A unit keeps its
// entry points, its PagedKV / Args struct and its describe text; the sixteen windowed bf16-query units share the entry body and the text too.
#pragma once
#include "flash_attn_decode_common.cuh"
#include "flash_attn_decode_paged_multi.cuh"  // fa2pm::kKeyStep, kMaxT
#include "flash_attn_prefill_paged.cuh"       // fa2pp::kRowTile
#include "kv_append_paged.cuh"                // kva::grid_y
#include <cstdarg>
#include <cstdio>
#include <type_traits>

namespace paged {

// ---------------------------------------------------------------- compile-time dispatch
// f(std::integral_constant<int, V>()) for the V of Vs... that v equals; the shape checks have made sure that it is one of them. A unit writes
// its launcher once, in a generic lambda. The lists below descend because clang emits the instantiations of a generic lambda last one first: so
// the kernels of a code object stay in ascending order, where they were when each unit spelled its switch out.
template <int... Vs, class F>
int pick(int v, F&& f) {
  int rc = CLN_ERR_UNSUPPORTED;
  (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>())), true)) || ...);
  return rc;
}
template <class F>
int for_head_dim(int D, F&& f) { return pick<128, 64>(D, f); }
template <class F>
int for_row_tiles(int tiles, F&& f) { return pick<4, 3, 2, 1>(tiles, f); }
template <class F>
int for_rope_mode(int rope_mode, F&& f) { return pick<2, 1, 0>(rope_mode, f); }

// ---------------------------------------------------------------- append
// The pointers and what goes with them. in = the n_req required inputs, then q, then rope_table; al4[i]: input i is an int32 / fp32 array,
// 4-byte aligned, else 16-byte; out = {k_pages, v_pages, q_out}, 16-byte aligned, q_out may be null. No output is another output or an input,
// but q_out may be q: a thread reads its pairs before it writes. rope_mode 0 takes no q, q_out or rope_table; 1 and 2 need a table, max_pos > 0
// and q with q_out together.
inline int append_args(const void* const* in, const int* al4, int n_req, const void* const (&out)[3], int P, int max_pos, int rope_mode) {
  const int n_in = n_req + 2;
  const void *q = in[n_req], *rope_table = in[n_req + 1], *q_out = out[2];
  for (int i = 0; i < n_req; ++i)
    if (!in[i]) return CLN_ERR_BAD_ARG;
  if (!out[0] || !out[1]) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < n_in; ++i)
    if (in[i] && !cln_aligned(in[i], al4[i] ? 4 : 16)) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < 3; ++i) {
    if (!out[i]) continue;
    if (!cln_aligned16(out[i])) return CLN_ERR_BAD_ARG;
    for (int j = 0; j < i; ++j)
      if (out[i] == out[j]) return CLN_ERR_BAD_ARG;
    for (int j = 0; j < n_in; ++j)
      if (out[i] == in[j] && !(i == 2 && j == n_req)) return CLN_ERR_BAD_ARG;
  }
  if (P <= 0) return CLN_ERR_BAD_ARG;
  if (rope_mode == 0 && (q || q_out || rope_table)) return CLN_ERR_BAD_ARG;
  if ((rope_mode == 1 || rope_mode == 2) && (!rope_table || max_pos <= 0 || (q == nullptr) != (q_out == nullptr))) return CLN_ERR_BAD_ARG;
  return CLN_OK;
}

// The checks that need no pointer: -1 for a non-positive dimension or Hq % Hkv != 0, -2 for another D, page or rope_mode, max_pages page >= 2^31
// or a grid that does not fit. T = the tokens per sequence, or with `packed` the packed rows total_q of all B sequences. *y = the workgroups per
// token (a thread per 8 elements, whatever the pools hold).
inline int append_shape(bool packed, int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int rope_mode, bool has_q, int* page_shift,
                        long long* y) {
  if (B <= 0 || T <= 0 || D <= 0 || Hq <= 0 || Hkv <= 0 || max_pages <= 0 || page <= 0 || Hq % Hkv != 0) return CLN_ERR_BAD_ARG;
  if ((D != 64 && D != 128) || rope_mode < 0 || rope_mode > 2) return CLN_ERR_UNSUPPORTED;
  fa2d::PagedGeometry g;
  const int rc = fa2d::paged_geometry(1, 1, max_pages, page, &g);  // the page size and max_pages page; the group size is of no concern here
  if (rc != CLN_OK) return rc;
  *page_shift = g.page_shift;
  *y = kva::grid_y(packed ? 1 : B, T, Hq, Hkv, has_q, D, rope_mode);
  return *y > 0 ? CLN_OK : CLN_ERR_UNSUPPORTED;
}

// what a describe text says of the rows, by rope_mode (the FP8 entry, which never copies a row bit for bit, words mode 0 itself)
constexpr const char* kRot[] = {"rows copied bit for bit", "K and q rotated in half-split pairs (i, i + D/2)",
                                "K and q rotated in interleaved pairs (2i, 2i + 1)"};

// ---------------------------------------------------------------- prefill
// The pointers: n_in inputs, all required, 16-byte aligned up to the block table (index 3), 4-byte from there on; o 16-byte aligned; lse may be
// null and is 4-byte aligned (not the 16 bytes of fa2d::check_pointers, which the decode entries use); no output is an input or the other output.
// The *_sink_* entries put their fp32 sinks [Hq] last: required, 4-byte aligned, not an output.
inline int prefill_args(const void* const* in, int n_in, const void* o, const float* lse, int P) {
  for (int i = 0; i < n_in; ++i)
    if (!in[i] || !cln_aligned(in[i], i >= 3 ? 4 : 16)) return CLN_ERR_BAD_ARG;
  if (!o || !cln_aligned16(o) || !cln_aligned(lse, 4) || (const void*)lse == o) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < n_in; ++i)
    if (o == in[i] || (lse && (const void*)lse == in[i])) return CLN_ERR_BAD_ARG;
  return P <= 0 ? CLN_ERR_BAD_ARG : CLN_OK;
}

// The checks that need no pointer: -1 for a non-positive dimension or Hq % Hkv != 0, -2 for another D, G or page, max_pages page >= 2^31, the
// rows T G of a sequence (packed: total_q G of all of them) past an int, or a grid that does not fit: 256 threads per workgroup, all in x.
// *tiles = the row tiles (workgroups) per (sequence, KV head) ...
inline int prefill_shape(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, fa2d::PagedGeometry* g, long long* tiles) {
  if (B <= 0 || T <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  const int rc = fa2d::paged_geometry(Hq, Hkv, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if (D != 64 && D != 128) return CLN_ERR_UNSUPPORTED;
  const long long R = (long long)T * g->group;
  *tiles = (R + fa2pp::kRowTile - 1) / fa2pp::kRowTile;
  if (R > 0x7fffffffLL || *tiles > 0xffffffffLL / fa2d::kThreads / B / Hkv) return CLN_ERR_UNSUPPORTED;
  return CLN_OK;
}
// ... and for a packed batch *slots = the workgroups per KV head, the B that may stay empty included: a function of B, total_q and G alone, the
// offsets stay on the device
inline int prefill_varlen_shape(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, fa2d::PagedGeometry* g, long long* slots) {
  if (B <= 0 || total_q <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  const int rc = fa2d::paged_geometry(Hq, Hkv, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if (D != 64 && D != 128) return CLN_ERR_UNSUPPORTED;
  const long long R = (long long)total_q * g->group;
  *slots = R / fa2pp::kRowTile + B;
  if (R > 0x7fffffffLL || *slots > 0xffffffffLL / fa2d::kThreads / Hkv) return CLN_ERR_UNSUPPORTED;
  return CLN_OK;
}

// ---------------------------------------------------------------- decode
// The split plan (fa2d::split_plan) of a paged decode entry: a function of (B, T, Hq, Hkv, max_pages, page, D) and the key step of its kernel
// only. A workgroup serves all T G query rows of a (sequence, KV head, split), so the workgroup count is B Hkv S whatever T is.
inline int decode_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int key_step, fa2d::PagedGeometry* g, fa2d::Plan* p) {
  if (B <= 0 || T <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  const int rc = fa2d::paged_geometry(Hq, Hkv, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if ((D != 64 && D != 128) || T > fa2pm::kMaxT) return CLN_ERR_UNSUPPORTED;
  return fa2d::split_plan((long long)B * Hkv, (long long)B * T * Hq, g->Nmax, page > key_step ? page : key_step, D, p);
}
// ... of the multi-token entries, whatever their pools hold: the key step of the three kernels is one number
inline int multi_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, fa2d::PagedGeometry* g, fa2d::Plan* p) {
  return decode_plan(B, T, Hq, Hkv, max_pages, page, D, fa2pm::kKeyStep, g, p);
}
// The sliding window of the *_window_* entries: the query at position p sees the keys max(0, p - window + 1) .. p; window >= 1.
inline int window_arg(int window) { return window <= 0 ? CLN_ERR_BAD_ARG : CLN_OK; }
// ... and the split plan of the windowed multi-token decode: not max_pages page but the span of keys a sequence can hold between the aligned start
// of its window (a multiple of U = max(page, key step) at or below the lower edge of its first new token) and its length,
//   span = min(Nmax, round_up(window + T - 1, U) + U),
// is what the S splits of C keys divide, so S C >= span. A function of the shape and the window only; for window >= Nmax the plan of multi_plan.
inline long long multi_window_unit(int page) { return page > fa2pm::kKeyStep ? page : fa2pm::kKeyStep; }
inline long long multi_window_span(int T, int page, int window, long long Nmax) {
  const long long U = multi_window_unit(page), reach = ((long long)window + T - 1 + U - 1) / U * U + U;
  return reach < Nmax ? reach : Nmax;
}
inline int multi_window_plan(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window, fa2d::PagedGeometry* g, fa2d::Plan* p) {
  if (B <= 0 || T <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  int rc = fa2d::paged_geometry(Hq, Hkv, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if ((D != 64 && D != 128) || T > fa2pm::kMaxT) return CLN_ERR_UNSUPPORTED;
  rc = window_arg(window);
  if (rc != CLN_OK) return rc;
  return fa2d::split_plan((long long)B * Hkv, (long long)B * T * Hq, multi_window_span(T, page, window, g->Nmax), multi_window_unit(page), D, p);
}
// the 16-row MFMA tiles of the T G query rows of a KV head: 1 ... 4, as T <= 8 and G <= 8
inline int multi_tiles(int T, const fa2d::PagedGeometry& g) { return (T * g.group + 15) / 16; }

// ---------------------------------------------------------------- any group size (the *_anyg_* entries)
// fa2d::paged_geometry for a group size G = Hq / Hkv that is any integer 1 ... kMaxGroupAnyG, not a power of two only: -1 for a non-positive
// dimension or Hq % Hkv != 0, -2 for a larger G, another page or max_pages page >= 2^31. g_shift stays 0 and means nothing: these kernels take
// g->group and divide.
constexpr int kMaxGroupAnyG = 16;
inline int geometry_anyg(int Hq, int Hkv, int max_pages, int page, fa2d::PagedGeometry* g) {
  if (Hq <= 0 || Hkv <= 0 || max_pages <= 0 || page <= 0 || Hq % Hkv != 0) return CLN_ERR_BAD_ARG;
  if (Hq / Hkv > kMaxGroupAnyG) return CLN_ERR_UNSUPPORTED;
  const int rc = fa2d::paged_geometry(1, 1, max_pages, page, g);  // the page size and max_pages page
  g->group = Hq / Hkv;
  return rc;
}
// prefill_varlen_shape on it: slots = total_q G / 128 + B
inline int prefill_varlen_shape_anyg(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, fa2d::PagedGeometry* g,
                                     long long* slots) {
  if (B <= 0 || total_q <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  const int rc = geometry_anyg(Hq, Hkv, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if (D != 64 && D != 128) return CLN_ERR_UNSUPPORTED;
  const long long R = (long long)total_q * g->group;
  *slots = R / fa2pp::kRowTile + B;
  if (R > 0x7fffffffLL || *slots > 0xffffffffLL / fa2d::kThreads / Hkv) return CLN_ERR_UNSUPPORTED;
  return CLN_OK;
}
// The tokens a prefill tile of 128 rows covers at most, for a describe text: a tile starts at row 128 i of its sequence, inside token 128 i / G at
// offset o = 128 i mod G, and its rows o ... o + 127 touch floor((o + 127) / G) + 1 tokens. o is a multiple of d = gcd(G, 128) = the lowest set
// bit of G (G <= 16) and reaches G - d. Where G divides 128, o = 0: 128 / G, the siblings' number; at G = 7 it is 20, where 128 / G is 18.
inline int prefill_tile_tokens_anyg(int G) { return (G - (G & -G) + fa2pp::kRowTile - 1) / G + 1; }
static_assert(fa2pp::kRowTile == 128, "the lowest set bit of G <= 16 is gcd(G, kRowTile)");
// multi_window_plan on it: the same fa2d::split_plan of the same numbers, so for G in {1, 2, 4, 8} the sibling's plan. The T G rows of a
// (sequence, KV head) are at most 4 row tiles of 16: T <= 8 and T G <= 64, else -2.
constexpr int kMaxRowsAnyG = 64;
inline int multi_window_plan_anyg(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window, fa2d::PagedGeometry* g,
                                  fa2d::Plan* p) {
  if (B <= 0 || T <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  int rc = geometry_anyg(Hq, Hkv, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if ((D != 64 && D != 128) || T > fa2pm::kMaxT || T * g->group > kMaxRowsAnyG) return CLN_ERR_UNSUPPORTED;
  rc = window_arg(window);
  if (rc != CLN_OK) return rc;
  return fa2d::split_plan((long long)B * Hkv, (long long)B * T * Hq, multi_window_span(T, page, window, g->Nmax), multi_window_unit(page), D, p);
}
// multi_tiles serves it as it is: ceil(T G / 16), 1 ... 4

// ---------------------------------------------------------------- softmax scale and logit soft-capping (the *_softcap_* entries)
// The two floats of a *_softcap_* entry, checked before anything else is looked at: softmax_scale == 0 means 1 / sqrt(D), softcap == 0 means no
// cap; any other value is finite and > 0, else -1 (a NaN fails every comparison). With x = the scale in use, what the kernels take:
//   mult  x log2(e): the score multiplier without a cap, and with one the multiplier of the small-argument branch (cap2 y = q.k mult). For
//         softmax_scale == 0 it is fa2d::scale_log2(D) itself, the number the siblings pass, else (float)((double)softmax_scale log2(e)).
//   pre   2 log2(e) x / cap: q.k pre = 2 log2(e) y is the exponent of exp2 in tanh(y) = 1 - 2 / (1 + e^(2 y)), y = q.k x / cap
//   cap2  cap log2(e): the capped score in the log2 units of the softmax
// mult and pre are clamped to FLT_MAX, cap2 to half of it: 0 times either stays 0. D <= 0 is the shape check's to refuse; no number is formed from it here.
struct SoftCap {
  float mult, pre, cap2;
  bool cap;
};
inline int softcap_arg(float softmax_scale, float softcap, int D, SoftCap* s) {
  if (!(softmax_scale >= 0.0f) || !(softcap >= 0.0f) || std::isinf(softmax_scale) || std::isinf(softcap)) return CLN_ERR_BAD_ARG;
  constexpr double kLog2e = 1.4426950408889634, kMax = 3.4028234663852886e38;
  const double x = softmax_scale != 0.0f ? (double)softmax_scale : D > 0 ? 1.0 / sqrt((double)D) : 1.0;
  const double mult = x * kLog2e;
  s->cap = softcap != 0.0f;
  s->mult = softmax_scale != 0.0f ? (float)(mult < kMax ? mult : kMax) : D > 0 ? fa2d::scale_log2(D) : 1.0f;
  const double pre = s->cap ? 2.0 * mult / (double)softcap : 0.0;
  s->pre = (float)(pre < kMax ? pre : kMax);
  const double cap2 = (double)softcap * kLog2e;
  s->cap2 = (float)(cap2 < kMax / 2 ? cap2 : kMax / 2);  // the kernels form 2 cap2
  return CLN_OK;
}
// The head of a *_softcap_* describe text, in front of the any-G sibling's text: the kernel, the scale in use and, with a cap, the cap clause --
// where the cap sits relative to the mask and the sink. Returns the characters written (< len), or len - 1 when the text did not fit.
inline int softcap_describe(char* buf, int len, const char* kernel, int D, float softmax_scale, float softcap, const SoftCap& s, bool fp8) {
  int n = snprintf(buf, len, "%s<D=%d,CAP=%d> softmax_scale=%.9g (%s), score multiplier x log2(e) = %.9g%s; ", kernel, D, s.cap ? 1 : 0,
                   softmax_scale != 0.0f ? (double)softmax_scale : 1.0 / sqrt((double)D),
                   softmax_scale != 0.0f ? "the caller's" : "the default 1 / sqrt(D)", (double)s.mult, fp8 ? " times k_scale" : "");
  if (n < len && s.cap)
    n += snprintf(buf + n, len - n,
                  "softcap=%.9g: every score is cap tanh(q.k x / cap)%s in fp32 (1 - 2 / (1 + exp2) on v_exp_f32 and v_rcp_f32; below |q.k x / cap| "
                  "= 2^-5 the series q.k x (1 - y^2 / 3)), capped before the window and causal mask (a hidden key is -inf, not -cap), the sink "
                  "neither scaled nor capped; ",
                  (double)softcap, fp8 ? " with k_scale inside the tanh" : "");
  if (n < len && !s.cap) n += snprintf(buf + n, len - n, "no cap: the any-G body with this multiplier; ");
  if (n < len) n += snprintf(buf + n, len - n, "otherwise ");
  return n < len ? n : len - 1;
}

// ---------------------------------------------------------------- head dim 256 (the *_d256_* entries)
// Siblings of append_shape, prefill_varlen_shape_anyg and multi_window_plan_anyg that take D = 256 and no other head dim: the same checks in the
// same order with the same status codes, so an argument that is wrong for the sibling is wrong here in the same way. The functions above and
// for_head_dim stay as they are: no existing entry takes 256.
constexpr int kHeadDim256 = 256;
template <class F>
int for_head_dim_256(int D, F&& f) { return pick<kHeadDim256>(D, f); }
inline int append_shape_d256(bool packed, int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int rope_mode, bool has_q, int* page_shift,
                             long long* y) {
  if (B <= 0 || T <= 0 || D <= 0 || Hq <= 0 || Hkv <= 0 || max_pages <= 0 || page <= 0 || Hq % Hkv != 0) return CLN_ERR_BAD_ARG;
  if (D != kHeadDim256 || rope_mode < 0 || rope_mode > 2) return CLN_ERR_UNSUPPORTED;
  fa2d::PagedGeometry g;
  const int rc = fa2d::paged_geometry(1, 1, max_pages, page, &g);
  if (rc != CLN_OK) return rc;
  *page_shift = g.page_shift;
  *y = kva::grid_y(packed ? 1 : B, T, Hq, Hkv, has_q, D, rope_mode);  // generic in D: 16 threads per row with the half-split pairs, else 32
  return *y > 0 ? CLN_OK : CLN_ERR_UNSUPPORTED;
}
// the prefill keeps the 128-row tile: slots = total_q G / 128 + B
inline int prefill_varlen_shape_anyg_d256(int B, int total_q, int Hq, int Hkv, int max_pages, int page, int D, fa2d::PagedGeometry* g,
                                          long long* slots) {
  if (B <= 0 || total_q <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  const int rc = geometry_anyg(Hq, Hkv, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if (D != kHeadDim256) return CLN_ERR_UNSUPPORTED;
  const long long R = (long long)total_q * g->group;
  *slots = R / fa2pp::kRowTile + B;
  if (R > 0x7fffffffLL || *slots > 0xffffffffLL / fa2d::kThreads / Hkv) return CLN_ERR_UNSUPPORTED;
  return CLN_OK;
}
// The decode at D = 256 gives a wave one 16-key block per step, so its workgroup step is 64 keys and not fa2pm::kKeyStep: the unit and the span
// are multi_window_unit / multi_window_span with that step. At most two row tiles: T <= 8 and T G <= 32, else -2.
constexpr int kKeyStepD256 = 64, kMaxRowsD256 = 32;
inline long long multi_window_unit_d256(int page) { return page > kKeyStepD256 ? page : kKeyStepD256; }
inline long long multi_window_span_d256(int T, int page, int window, long long Nmax) {
  const long long U = multi_window_unit_d256(page), reach = ((long long)window + T - 1 + U - 1) / U * U + U;
  return reach < Nmax ? reach : Nmax;
}
inline int multi_window_plan_anyg_d256(int B, int T, int Hq, int Hkv, int max_pages, int page, int D, int window, fa2d::PagedGeometry* g,
                                       fa2d::Plan* p) {
  if (B <= 0 || T <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  int rc = geometry_anyg(Hq, Hkv, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if (D != kHeadDim256 || T > fa2pm::kMaxT || T * g->group > kMaxRowsD256) return CLN_ERR_UNSUPPORTED;
  rc = window_arg(window);
  if (rc != CLN_OK) return rc;
  return fa2d::split_plan((long long)B * Hkv, (long long)B * T * Hq, multi_window_span_d256(T, page, window, g->Nmax),
                          multi_window_unit_d256(page), D, p);
}
template <class F>
int for_row_tiles_d256(int tiles, F&& f) { return pick<2, 1>(tiles, f); }

// ---------------------------------------------------------------- multi-head latent attention (the *_mla_* entries)
// One pool of latent rows [P, page, 576] = [c (512) | k_pe (64)], shared by every query head: Hkv = 1 by construction, the key has 576 dims and
// the value the first 512 of them. Nothing above changes: no existing entry takes these shapes.
constexpr int kMlaDc = 512, kMlaDr = 64, kMlaDk = kMlaDc + kMlaDr, kMlaMaxHq = 128, kMlaRowGroup = 64, kMlaKeyStep = 64;
// The softmax scale of the decode entry has no default (the models use 192^-1/2 mscale^2, not 576^-1/2): finite and > 0, else -1 (a NaN
// fails the comparison). *mult = x log2(e), formed in double and rounded once, as softcap_arg forms it for a scale of the caller's.
inline int mla_scale_arg(float softmax_scale, float* mult) {
  if (!(softmax_scale > 0.0f) || std::isinf(softmax_scale)) return CLN_ERR_BAD_ARG;
  constexpr double kLog2e = 1.4426950408889634, kMax = 3.4028234663852886e38;
  const double x = (double)softmax_scale * kLog2e;
  *mult = (float)(x < kMax ? x : kMax);
  return CLN_OK;
}
// The split plan of the decode: a workgroup serves one (sequence, split, row group of 64 of the R = T Hq query rows), so
// fa2d::split_plan(bk = B ceil(R / 64), rows = B R, Nmax, unit = max(page, 64), D = 512): a function of the shape only. -1 for a non-positive
// dimension, -2 for T > 8, Hq > 128, another page, max_pages page >= 2^31 or a grid that does not fit.
inline int mla_plan(int B, int T, int Hq, int max_pages, int page, fa2d::PagedGeometry* g, fa2d::Plan* p) {
  if (B <= 0 || T <= 0 || Hq <= 0) return CLN_ERR_BAD_ARG;
  const int rc = fa2d::paged_geometry(1, 1, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  if (T > fa2pm::kMaxT || Hq > kMlaMaxHq) return CLN_ERR_UNSUPPORTED;
  const long long R = (long long)T * Hq, row_groups = (R + kMlaRowGroup - 1) / kMlaRowGroup;
  return fa2d::split_plan(B * row_groups, B * R, g->Nmax, page > kMlaKeyStep ? page : kMlaKeyStep, kMlaDc, p);
}
// The split plan of the SPARSE decode (the *_mla_sparse_* entries): a workgroup serves one (sequence, query token, group of 64
// heads, split of the token's topk index slots), so fa2d::split_plan(bk = B T ceil(Hq / 64), rows = B T Hq, Nmax = topk, unit = 64, D = 512):
// the splits divide the index slots, not the context, and T has no cap. -1 for a non-positive dimension, -2 for Hq > 128, another page,
// max_pages page >= 2^31, B T Hq >= 2^31 or a grid that does not fit.
inline int mla_sparse_plan(int B, int T, int Hq, int topk, int max_pages, int page, fa2d::PagedGeometry* g, fa2d::Plan* p) {
  if (B <= 0 || T <= 0 || Hq <= 0 || topk <= 0) return CLN_ERR_BAD_ARG;
  const int rc = fa2d::paged_geometry(1, 1, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  const long long tokens = (long long)B * T;
  if (Hq > kMlaMaxHq || tokens > 0x7fffffffLL) return CLN_ERR_UNSUPPORTED;
  return fa2d::split_plan(tokens * ((Hq + kMlaRowGroup - 1) / kMlaRowGroup), tokens * Hq, topk, kMlaKeyStep, kMlaDc, p);
}
// The prologue of the three decode describes in the order of its status codes: the buffer, the scale (*mult as above), the entry's plan.
inline int mla_describe_args(const char* buf, int len, float softmax_scale, float* mult, int plan_rc) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  const int rc = mla_scale_arg(softmax_scale, mult);
  return rc != CLN_OK ? rc : plan_rc;
}
// The pointers of the two appends and what goes with them, all -1: c_new, k_pe_new, pool, q and q_out 16-byte aligned, the int32 arrays,
// kv_scale and rope_table 4-byte; q, q_out and rope_table may be null, kv_scale is required only where fp8 (the bf16 entry passes null). No
// output (pool, q_out) is an input or the other output, but q_out may be q: a thread reads its pairs before it writes. append_args does not
// serve: there is one pool, and unlike there rope_mode 0 takes q with q_out (the query rows are then copied bit for bit); a table goes with a
// rotation and max_pos > 0, never with rope_mode 0.
inline int mla_append_args(const void* c_new, const void* k_pe_new, const void* pool, const int* block_table, const int* seqlens, const int* cu_q,
                           const float* kv_scale, bool fp8, const void* q, const void* q_out, const float* rope_table, int P, int max_pos,
                           int rope_mode) {
  if (!c_new || !k_pe_new || !pool || !block_table || !seqlens || !cu_q || (fp8 && !kv_scale)) return CLN_ERR_BAD_ARG;
  if (!cln_aligned16(c_new) || !cln_aligned16(k_pe_new) || !cln_aligned16(pool) || !cln_aligned16(q) || !cln_aligned16(q_out))
    return CLN_ERR_BAD_ARG;
  if (!cln_aligned(block_table, 4) || !cln_aligned(seqlens, 4) || !cln_aligned(cu_q, 4) || !cln_aligned(kv_scale, 4) || !cln_aligned(rope_table, 4))
    return CLN_ERR_BAD_ARG;
  const void* const in[] = {c_new, k_pe_new, block_table, seqlens, cu_q, kv_scale, rope_table};
  for (const void* p : in)
    if (p && (p == pool || p == q_out)) return CLN_ERR_BAD_ARG;
  if (pool == q || pool == q_out) return CLN_ERR_BAD_ARG;
  if (P <= 0 || (q == nullptr) != (q_out == nullptr)) return CLN_ERR_BAD_ARG;
  if (rope_mode == 0 && rope_table) return CLN_ERR_BAD_ARG;
  if ((rope_mode == 1 || rope_mode == 2) && (!rope_table || max_pos <= 0)) return CLN_ERR_BAD_ARG;
  return CLN_OK;
}
// The append: a thread per 16-byte piece; per token one pool row and, with q, Hq query rows of 64 copied pieces and the rotary pieces (4 with
// the half-split pairs, which a thread moves two at a time, else 8). *y = the workgroups per token.
inline int mla_append_pieces(int rope_mode) { return kMlaDc / 8 + (rope_mode == 1 ? kMlaDr / 16 : kMlaDr / 8); }
inline int mla_append_shape(int B, int total_q, int Hq, int max_pages, int page, int rope_mode, bool has_q, int* page_shift, long long* y) {
  if (B <= 0 || total_q <= 0 || Hq <= 0 || max_pages <= 0 || page <= 0) return CLN_ERR_BAD_ARG;
  if (rope_mode < 0 || rope_mode > 2) return CLN_ERR_UNSUPPORTED;
  fa2d::PagedGeometry g;
  const int rc = fa2d::paged_geometry(1, 1, max_pages, page, &g);
  if (rc != CLN_OK) return rc;
  *page_shift = g.page_shift;
  *y = ((1LL + (has_q ? Hq : 0)) * mla_append_pieces(rope_mode) + kva::kThreads - 1) / kva::kThreads;
  return *y <= 65535 ? CLN_OK : CLN_ERR_UNSUPPORTED;
}

// ---------------------------------------------------------------- MLA prefill, state merge and gather
// The un-absorbed prompt path: per head a key of 192 dims [k_nope 128 | k_pe 64] and a value of 128, Hkv = Hq, nothing paged. Nothing above
// changes.
constexpr int kMlaDn = 128, kMlaDq = kMlaDn + kMlaDr, kMlaDv = 128;
// The prefill's pointers: q, kv, k_pe 16-byte aligned, cu_q and cu_k 4-byte, all required; o 16-byte aligned; lse may be null, 4-byte aligned;
// no output is an input or the other output.
inline int mla_prefill_args(const void* q, const void* kv, const void* k_pe, const int* cu_q, const int* cu_k, const void* o, const float* lse) {
  const void* const in[] = {q, kv, k_pe, cu_q, cu_k};
  for (int i = 0; i < 5; ++i)
    if (!in[i] || !cln_aligned(in[i], i >= 3 ? 4 : 16)) return CLN_ERR_BAD_ARG;
  if (!o || !cln_aligned16(o) || !cln_aligned(lse, 4) || (const void*)lse == o) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < 5; ++i)
    if (o == in[i] || (lse && (const void*)lse == in[i])) return CLN_ERR_BAD_ARG;
  return CLN_OK;
}
// -1 for a non-positive dimension, -2 for Hq > 128, a causal flag that is neither 0 nor 1, or a grid that does not fit. *slots = the workgroups
// per head, total_q / 128 + B (prefill_varlen_shape at G = 1): the offsets stay on the device.
inline int mla_prefill_shape(int B, int total_q, int total_k, int Hq, int causal, long long* slots) {
  if (B <= 0 || total_q <= 0 || total_k <= 0 || Hq <= 0) return CLN_ERR_BAD_ARG;
  if (Hq > kMlaMaxHq || (causal != 0 && causal != 1)) return CLN_ERR_UNSUPPORTED;
  *slots = (long long)total_q / fa2pp::kRowTile + B;
  return *slots > 0xffffffffLL / fa2d::kThreads / Hq ? CLN_ERR_UNSUPPORTED : CLN_OK;
}
// The merge of two attention states: a workgroup of 256 threads serves 256 / (D / 8) whole rows, a thread per 16-byte piece. -1 for a
// non-positive dimension, -2 for a D outside 8 ... 512 or no multiple of 8, or a grid that does not fit. *rows_per_wg, *wgs: the launch.
constexpr int kMergeThreads = 256, kMergeMaxD = 512;
inline int merge_shape(long long rows, int D, int* rows_per_wg, long long* wgs) {
  if (rows <= 0 || D <= 0) return CLN_ERR_BAD_ARG;
  if (D % 8 != 0 || D > kMergeMaxD) return CLN_ERR_UNSUPPORTED;
  *rows_per_wg = kMergeThreads / (D / 8);
  *wgs = (rows + *rows_per_wg - 1) / *rows_per_wg;
  return *wgs > 0x7fffffffLL ? CLN_ERR_UNSUPPORTED : CLN_OK;
}
// The gather out of the latent pool: the append's launch shape without q, a packed row x the 72 pieces of its latent row.
inline int mla_gather_shape(int B, int total_k, int max_pages, int page, int* page_shift, long long* y) {
  return mla_append_shape(B, total_k, 1, max_pages, page, 0, false, page_shift, y);
}
// The pointers of the two gathers, all -1: pool and out 16-byte aligned, block_table, starts, cu_k and kv_scale 4-byte; starts may be null,
// kv_scale is required only where fp8 (the bf16 entry passes null); the output is no input. Then P.
inline int mla_gather_args(const void* pool, const int* block_table, const int* starts, const int* cu_k, const float* kv_scale, bool fp8,
                           const void* out, int P) {
  if (!pool || !block_table || !cu_k || (fp8 && !kv_scale) || !out) return CLN_ERR_BAD_ARG;
  if (!cln_aligned16(pool) || !cln_aligned16(out) || !cln_aligned(block_table, 4) || !cln_aligned(starts, 4) || !cln_aligned(cu_k, 4) ||
      !cln_aligned(kv_scale, 4))
    return CLN_ERR_BAD_ARG;
  const void* const in[] = {pool, block_table, starts, cu_k, kv_scale};
  for (const void* p : in)
    if (p == out) return CLN_ERR_BAD_ARG;
  return P <= 0 ? CLN_ERR_BAD_ARG : CLN_OK;
}

// The arguments of a decode entry in the order of their status codes: the pointers (fa2d::check_pointers), P, the status of the entry's plan
// and, where the plan splits the keys, the workspace. The *_sink_* entries put their fp32 sinks [Hq] last in `in`, behind seqlens. first_int =
// the leading inputs that are 16-byte aligned: q and the two pools, or for the MLA entries, which have one pool, 2.
inline int decode_args(const void* const* in, int n_in, const void* const (&out)[3], long long workspace_bytes, int P, int plan_rc,
                       const fa2d::Plan& p, int first_int = 3) {
  const int rc = fa2d::check_pointers(in, n_in, first_int, out);
  if (rc != CLN_OK) return rc;
  if (P <= 0) return CLN_ERR_BAD_ARG;
  if (plan_rc != CLN_OK) return plan_rc;
  return fa2d::workspace_fits(p, out[2], workspace_bytes) ? CLN_OK : CLN_ERR_BAD_ARG;
}

// ---------------------------------------------------------------- the windowed bf16-query entries
// One entry body, one plan body and one describe text per family for the sixteen units flash_attn_prefill_paged_varlen_window*.hip and
// flash_attn_decode_paged_multi_window*.hip. A unit says what it is -- its pools KV (fa2b::PagedKV, or fa2d::PagedKV8 with the two scales), its
// group sizes GR, its inputs in the order in which they are checked -- and launches its own kernel; the protocol is here.
enum Groups { kPow2G, kAnyG, kAnyGD256 };                 // G in {1, 2, 4, 8}; any G in 1 ... 16; any G at D = 256 and no other head dim
enum Sinks { kNoSinks, kSinksRequired, kSinksOptional };  // for a describe text: a launching entry counts sinks into its inputs or leaves it out
// the numbers of an entry; T = the tokens of a sequence, or total_q of a packed prefill; the two floats are 0 where the entry has none
struct WindowArgs {
  int B, T, Hq, Hkv, max_pages, page, D, window;
  float softmax_scale = 0.0f, softcap = 0.0f;
};
// what the checks work out for a launcher: slots for a prefill, p for a decode
struct WindowLaunch {
  fa2d::PagedGeometry g;
  long long slots;
  fa2d::Plan p;
  SoftCap sc;
};
template <Groups GR>
int window_prefill_shape(const WindowArgs& a, fa2d::PagedGeometry* g, long long* slots) {
  constexpr auto shape = GR == kPow2G ? prefill_varlen_shape : GR == kAnyG ? prefill_varlen_shape_anyg : prefill_varlen_shape_anyg_d256;
  const int rc = shape(a.B, a.T, a.Hq, a.Hkv, a.max_pages, a.page, a.D, g, slots);
  return rc != CLN_OK ? rc : window_arg(a.window);
}
template <Groups GR>
int window_plan(const WindowArgs& a, fa2d::PagedGeometry* g, fa2d::Plan* p) {
  constexpr auto plan = GR == kPow2G ? multi_window_plan : GR == kAnyG ? multi_window_plan_anyg : multi_window_plan_anyg_d256;
  return plan(a.B, a.T, a.Hq, a.Hkv, a.max_pages, a.page, a.D, a.window, g, p);
}
// a *_plan entry: a refusal leaves the three out-parameters alone
template <Groups GR>
int window_plan_entry(const WindowArgs& a, int* splits, int* chunk, long long* workspace_bytes) {
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  return fa2d::plan_out(window_plan<GR>(a, &g, &p), p, splits, chunk, workspace_bytes);
}

// FP8 pools are the ones with scales. Every entry's inputs begin q, k_pages, v_pages, block_table; the two scales stand at in[scales].
template <class KV, class = void>
constexpr bool kFp8Pools = false;
template <class KV>
constexpr bool kFp8Pools<KV, std::void_t<decltype(KV::k_scale)>> = true;
template <class KV>
KV pool_view(const void* const* in, int scales, int Hkv, int max_pages, int page_shift) {
  using E = decltype(KV::k);
  if constexpr (kFp8Pools<KV>)
    return {(E)in[1], (E)in[2], (const float*)in[scales], (const float*)in[scales + 1], (const int*)in[3], Hkv, max_pages, page_shift};
  else
    return {(E)in[1], (E)in[2], (const int*)in[3], Hkv, max_pages, page_shift};
}
template <Groups GR, class F>
int for_head_dim_of(int D, F&& f) {
  if constexpr (GR == kAnyGD256) return for_head_dim_256(D, f);
  else return for_head_dim(D, f);
}
template <Groups GR, class F>
int for_row_tiles_of(int tiles, F&& f) {
  static_assert(kMaxRowsAnyG == 4 * 16 && kMaxRowsD256 == 2 * 16, "for_row_tiles has 1 ... 4 row tiles of 16, for_row_tiles_d256 1 or 2");
  if constexpr (GR == kAnyGD256) return for_row_tiles_d256(tiles, f);
  else return for_row_tiles(tiles, f);
}
// f(std::true_type()) with a cap, else f(std::false_type()): an entry without the two floats has no cap, and its launcher ignores the argument
template <class F>
int for_cap(bool cap, F&& f) { return cap ? f(std::true_type()) : f(std::false_type()); }
// the two floats of the entry into w->sc; a launcher passes sc.mult, sc.pre, sc.cap2, and without a cap the last two are +0 (softcap may be -0)
inline int window_softcap(const WindowArgs& a, WindowLaunch* w) {
  const int rc = softcap_arg(a.softmax_scale, a.softcap, a.D, &w->sc);
  if (!w->sc.cap) w->sc.pre = w->sc.cap2 = 0.0f;
  return rc;
}

// A packed prefill entry, in the order of its status codes: the two floats (paged::softcap_arg, before any pointer is looked at), the pointers
// and P (paged::prefill_args on the n_in inputs q, k_pages, v_pages, block_table, seqlens, cu_q[, k_scale, v_scale][, sinks]; sinks is counted
// where it is required or given), the shape, the window. Then launch(d, cap, kv, w) for the head dim and CAP as integral constants.
template <class KV, Groups GR, class F>
int window_prefill(const void* const* in, int n_in, void* o, float* lse, int P, const WindowArgs& a, F&& launch) {
  WindowLaunch w = {};
  int rc = window_softcap(a, &w);
  if (rc == CLN_OK) rc = prefill_args(in, n_in, o, lse, P);
  if (rc == CLN_OK) rc = window_prefill_shape<GR>(a, &w.g, &w.slots);
  if (rc != CLN_OK) return rc;
  const KV kv = pool_view<KV>(in, 6, a.Hkv, a.max_pages, w.g.page_shift);
  return for_head_dim_of<GR>(a.D, [&](auto d) { return for_cap(w.sc.cap, [&](auto cap) { return launch(d, cap, kv, w); }); });
}
// A multi-token decode entry likewise: the two floats, then paged::decode_args on q, k_pages, v_pages, block_table, seqlens[, k_scale,
// v_scale][, sinks] with the plan of its group sizes. Then launch(d, mt, cap, kv, w), mt = the row tiles of 16.
template <class KV, Groups GR, class F>
int window_decode(const void* const* in, int n_in, void* o, float* lse, void* workspace, long long workspace_bytes, int P, const WindowArgs& a,
                  F&& launch) {
  WindowLaunch w = {};
  int rc = window_softcap(a, &w);
  if (rc == CLN_OK) rc = decode_args(in, n_in, {o, lse, workspace}, workspace_bytes, P, window_plan<GR>(a, &w.g, &w.p), w.p);
  if (rc != CLN_OK) return rc;
  const KV kv = pool_view<KV>(in, 5, a.Hkv, a.max_pages, w.g.page_shift);
  return for_head_dim_of<GR>(a.D, [&](auto d) {
    return for_row_tiles_of<GR>(multi_tiles(a.T, w.g), [&](auto mt) {
      return for_cap(w.sc.cap, [&](auto cap) { return launch(d, mt, cap, kv, w); });
    });
  });
}

// A describe text in pieces: each is written behind the last while the text fits, so a short buffer gets the head of the whole text.
struct Text {
  char* buf;
  int len, n;
  __attribute__((format(printf, 2, 3))) void add(const char* fmt, ...) {
    if (n >= len) return;
    va_list ap;
    va_start(ap, fmt);
    n += vsnprintf(buf + n, len - n, fmt, ap);
    va_end(ap);
  }
  int end() const { return n < len ? n : len - 1; }  // the characters written
};
// The text of a packed prefill entry; the clauses that vary are the kernel's name, the group sizes, the pools and the sink. The D = 256 unit
// words its own text.
template <class KV, Groups GR>
int window_prefill_describe(const char* kernel, Sinks sinks, const WindowArgs& a, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  long long slots = 0;
  const int rc = window_prefill_shape<GR>(a, &g, &slots);
  if (rc != CLN_OK) return rc;
  constexpr bool fp8 = kFp8Pools<KV>, anyg = GR != kPow2G;
  constexpr int kRows = fa2pp::kRowTile, kKeys = fa2pp::kKeyStep;
  // the keys a tile walks at most: the window of its first token, the tokens of its rows (128 / G where G divides the tile; else a tile may
  // start inside a token), and the two steps its ends are aligned to
  const long long span = (long long)a.window + prefill_tile_tokens_anyg(g.group) + 2 * kKeys;
  Text t = {buf, len, 0};
  t.add(anyg ? "%s<D=%d> G=%d" : "%s<D=%d,G=%d>", kernel, a.D, g.group);
  t.add(" B=%d total_q=%d page=%d rows=%d keys=%d W=%d: one launch, no workspace; %lld workgroups of 256 threads (%d KV heads x %lld slots = "
        "total_q G / %d + B, at most B of them empty), sequence b owns the slots from cu_q[b] G / %d + b, found by binary search over the "
        "device-side offsets; a slot is a tile of %d of the T_b G query rows t G + g of its sequence, ",
        a.B, a.T, a.page, kRows, kKeys, a.window, (long long)a.Hkv * slots, a.Hkv, slots, kRows, kRows, kRows);
  if (anyg) t.add("(t, g) = (r / G, r mod G) by division outside the key loop, any G in 1 ... %d, ", kMaxGroupAnyG);
  t.add("32 rows per wave, and walks the keys from the step that holds the lower edge p - W + 1 of its first token to the causal edge of its "
        "last in steps of %d, a span of at most %lld keys whatever the length; %s no table entry and no row below that first step; S^T = K Q^T "
        "and O^T = V^T P^T on v_mfma_f32_16x16x32_bf16, V through ds_read_b64_tr_b16, fp32 scores%s, window and causal mask by select on the "
        "steps that cross an edge, online softmax, %sno split over the keys (S=1, C=the span)",
        kKeys, span < g.Nmax ? span : g.Nmax,
        fp8 ? "e4m3 K and V rows through the block table, 8 bytes per thread and row, converted to bf16 once on their way to LDS "
              "(v_cvt_scalef32_pk_bf16_fp8, exact), once per workgroup,"
            : "K and V rows through the block table to LDS once per workgroup,",
        fp8 ? " times k_scale" : "", fp8 ? "the normalisation times v_scale, " : "");
  if (sinks != kNoSinks)
    t.add("; the sink of a row's head (fp32, natural log, unscaled%s) is folded into the fp32 (m, l) of the finished row in the epilogue, once, "
          "and a row that sees no key stays O = 0, LSE = -inf",
          sinks == kSinksOptional ? "; none when sinks is NULL" : "");
  t.add("; deterministic");
  return t.end();
}
// The text of a multi-token decode entry, with the same clauses.
template <class KV, Groups GR>
int window_decode_describe(const char* kernel, Sinks sinks, const WindowArgs& a, char* buf, int len) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  fa2d::Plan p;
  const int rc = window_plan<GR>(a, &g, &p);
  if (rc != CLN_OK) return rc;
  constexpr bool fp8 = kFp8Pools<KV>, anyg = GR != kPow2G;
  const int tiles = multi_tiles(a.T, g);
  const char* const none = sinks == kSinksOptional ? "; none when sinks is NULL" : "";
  Text t = {buf, len, 0};
  t.add("%s<D=%d,MT=%d> T=%d G=%d W=%d span=%lld S=%d C=%d page=%d: the S splits of C keys divide the span from base = align_down(max(0, len - T "
        "- W + 1), %lld) on, no table entry and no row below base; 4 waves split the %d-key steps, %s, each row loaded once for the %d query rows "
        "(T x G, %d tiles of 16",
        kernel, a.D, tiles, a.T, g.group, a.window, multi_window_span(a.T, a.page, a.window, g.Nmax), p.splits, p.chunk, a.page,
        multi_window_unit(a.page), fa2pm::kKeyStep,
        fp8 ? "e4m3 K and V rows through the block table to registers, 16 bytes per lane, converted to bf16 once (v_cvt_scalef32_pk_bf16_fp8, "
              "exact): K to MFMA fragments, V through a transposed LDS read"
            : "K rows through the block table straight to MFMA fragments, V rows through a transposed LDS read",
        a.T * g.group, tiles);
  if (anyg) t.add("; (t, g) = (r / G, r mod G) by division outside the key loop, any G in 1 ... %d with T G <= %d", kMaxGroupAnyG, kMaxRowsAnyG);
  t.add(") of its KV head, S^T = K Q^T and O^T = V^T P^T on v_mfma_f32_16x16x32_bf16, fp32 scores%s, window and causal mask by select, online "
        "softmax%s",
        fp8 ? " times k_scale" : "", fp8 ? ", the partial times v_scale" : "");
  if (p.splits == 1 && sinks != kNoSinks)
    t.add("; the sink of a row's head (fp32, natural log, unscaled%s) is folded into the fp32 (m, l) of the finished row at its final store, "
          "once, and a row that sees no key stays O = 0, LSE = -inf",
          none);
  if (p.splits > 1) {
    t.add("; then fa2_decode_combine_window%s_bf16_rows<D=%d> merges the live splits ceil((len - base) / C) of a query row by log-sum-exp in "
          "ascending order (workspace %lld bytes)",
          sinks != kNoSinks ? "_sink" : "", a.D, p.ws_bytes);
    if (sinks != kNoSinks) {
      t.add(" and folds the sink of the row's head (fp32, natural log, unscaled%s", none);
      if (sinks == kSinksOptional) t.add(": fa2_decode_combine_window_bf16_rows<D=%d> then", a.D);
      t.add(") into the merged fp32 (m, l), once: the splits store raw partials, and a row that sees no key stays O = 0, LSE = -inf");
    }
  }
  t.add("; deterministic");
  return t.end();
}
// A *_softcap_* describe: the buffer, the two floats, then paged::softcap_describe as the head of the text and behind it the any-G sibling's,
// which rest(buf, len) writes; a refusal of the sibling's is this entry's.
template <class F>
int softcap_describe_then(char* buf, int len, const char* kernel, const WindowArgs& a, bool fp8, F&& rest) {
  if (!buf || len <= 0) return CLN_ERR_BAD_ARG;
  SoftCap sc;
  int rc = softcap_arg(a.softmax_scale, a.softcap, a.D, &sc);
  if (rc != CLN_OK) return rc;
  const int n = softcap_describe(buf, len, kernel, a.D, a.softmax_scale, a.softcap, sc, fp8);
  rc = rest(buf + n, len - n);
  return rc < 0 ? rc : n + rc;
}

// ---------------------------------------------------------------- the DSA indexer (the *_index_* entries)
// DeepSeek-V3.2's indexer in front of the sparse decode: one pool of index keys [P, page, 128] behind the block table of the latent cache, up
// to 64 index heads, fp32 logits [B, T, ld] and the exact top-k of a row. Nothing above changes: no existing entry takes these shapes.
constexpr int kIdxDim = 128, kIdxMaxHeads = 64, kIdxChunk = 1024, kIdxRowsPerWg = kva::kThreads / (kIdxDim / 8);
constexpr int kTopkThreads = 1024, kTopkBlock = 4 * kTopkThreads;
// n inputs, all required, 16-byte aligned where al16[i], else 4-byte; the one output with its alignment; the output is no input
inline int index_args(const void* const* in, const int* al16, int n, const void* out, int out_align) {
  for (int i = 0; i < n; ++i)
    if (!in[i] || !cln_aligned(in[i], al16[i] ? 16 : 4)) return CLN_ERR_BAD_ARG;
  if (!out || !cln_aligned(out, out_align)) return CLN_ERR_BAD_ARG;
  for (int i = 0; i < n; ++i)
    if (out == in[i]) return CLN_ERR_BAD_ARG;
  return CLN_OK;
}
// The append of index keys: a thread per 16-byte piece, 16 pieces a row, 16 packed rows a workgroup. -1 for a non-positive dimension, -2 for
// another page or max_pages page >= 2^31. *wgs = the workgroups.
inline int index_append_shape(int B, int total_q, int max_pages, int page, int* page_shift, long long* wgs) {
  if (B <= 0 || total_q <= 0 || max_pages <= 0 || page <= 0) return CLN_ERR_BAD_ARG;
  fa2d::PagedGeometry g;
  const int rc = fa2d::paged_geometry(1, 1, max_pages, page, &g);
  if (rc != CLN_OK) return rc;
  *page_shift = g.page_shift;
  *wgs = ((long long)total_q + kIdxRowsPerWg - 1) / kIdxRowsPerWg;
  return CLN_OK;
}
// The logits: a workgroup serves one (sequence, query token, chunk of kIdxChunk keys); the grid is sized from cap = min(max_pages page, ld),
// the lengths stay on the device. -1 for a non-positive dimension, -2 for Hi > 64, another page, max_pages page >= 2^31, B T >= 2^31 or a
// grid that does not fit. *cap, *chunks = the chunks of a token, *wgs = B T chunks.
inline int index_logits_shape(int B, int T, int Hi, long long ld, int max_pages, int page, fa2d::PagedGeometry* g, int* cap, int* chunks,
                              long long* wgs) {
  if (B <= 0 || T <= 0 || Hi <= 0 || ld <= 0) return CLN_ERR_BAD_ARG;
  const int rc = fa2d::paged_geometry(1, 1, max_pages, page, g);
  if (rc != CLN_OK) return rc;
  const long long tokens = (long long)B * T;
  if (Hi > kIdxMaxHeads || tokens > 0x7fffffffLL) return CLN_ERR_UNSUPPORTED;
  *cap = (int)(g->Nmax < ld ? g->Nmax : ld);
  *chunks = (*cap + kIdxChunk - 1) / kIdxChunk;
  *wgs = tokens * *chunks;
  return *wgs > 0xffffffffLL / fa2d::kThreads ? CLN_ERR_UNSUPPORTED : CLN_OK;
}
// The top-k: one workgroup of kTopkThreads per (sequence, query token) row. -1 for a non-positive dimension, -2 for ld >= 2^31, B T >= 2^31,
// topk B T past 2^61 (the bytes of indices fit a long long) or a grid that does not fit (B T kTopkThreads >= 2^32).
inline int index_topk_shape(int B, int T, long long ld, int topk, long long* tokens) {
  if (B <= 0 || T <= 0 || ld <= 0 || topk <= 0) return CLN_ERR_BAD_ARG;
  *tokens = (long long)B * T;
  if (ld > 0x7fffffffLL || *tokens > 0x7fffffffLL || *tokens > (1LL << 61) / topk || *tokens > 0xffffffffLL / kTopkThreads)
    return CLN_ERR_UNSUPPORTED;
  return CLN_OK;
}

// ---------------------------------------------------------------- the packed DSA step (the *_varlen_* indexer and sparse entries)
// The three calls behind the append for a packed batch: [total_q, ...] rows and the device-side offsets cu_q [B + 1]. A workgroup's job is a
// packed row where the fixed-T entries have (sequence, query token), so each shape is its sibling's with total_q in the place of B T -- a
// packed call with cu_q = [0, T, 2 T, ...] has the sibling's grid and the sibling's plan -- and B > 0 is all that is asked of B: the offsets
// stay on the device. The status codes are the siblings'. Nothing above changes.
inline int index_logits_varlen_shape(int B, int total_q, int Hi, long long ld, int max_pages, int page, fa2d::PagedGeometry* g, int* cap,
                                     int* chunks, long long* wgs) {
  if (B <= 0) return CLN_ERR_BAD_ARG;
  return index_logits_shape(1, total_q, Hi, ld, max_pages, page, g, cap, chunks, wgs);
}
inline int index_topk_varlen_shape(int B, int total_q, long long ld, int topk, long long* tokens) {
  if (B <= 0) return CLN_ERR_BAD_ARG;
  return index_topk_shape(1, total_q, ld, topk, tokens);
}
// the plan has no B: a function of the packed rows only
inline int mla_sparse_varlen_plan(int total_q, int Hq, int topk, int max_pages, int page, fa2d::PagedGeometry* g, fa2d::Plan* p) {
  return mla_sparse_plan(1, total_q, Hq, topk, max_pages, page, g, p);
}
// ... and what an entry that takes B passes to decode_args and mla_describe_args as the status of its plan
inline int mla_sparse_varlen_shape(int B, int total_q, int Hq, int topk, int max_pages, int page, fa2d::PagedGeometry* g, fa2d::Plan* p) {
  if (B <= 0) return CLN_ERR_BAD_ARG;
  return mla_sparse_varlen_plan(total_q, Hq, topk, max_pages, page, g, p);
}

}  // namespace paged
