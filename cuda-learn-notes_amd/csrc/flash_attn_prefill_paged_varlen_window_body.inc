// The statements of the bf16 sliding-window packed variable-length prefill kernels over a paged KV cache, included once into the body of each
// __global__ kernel of flash_attn_prefill_paged_varlen_window*.cuh (flash_attn_prefill_paged_varlen_window_body.cuh says what they do, what a
// kernel chooses and why this is an inclusion and not a function). In scope at the point of inclusion: the kernel's parameters q, kv, seqlens,
// cu_q, sinks, o, lse, B, total_q, slots, W, scale_log2, pre, cap2 (a kernel without sinks or without the cap's multipliers declares constants
// of these names), and D, CAP, GM, SINKS, ga.
  using PL = Pool<typename std::remove_cv<decltype(kv)>::type>;
  constexpr int KS = D / 32;             // k-steps of S^T = the 16-byte (FP8: 8-byte) pieces a thread stages per step and tensor
  constexpr int DB = D / 16;             // 16-dim blocks of O^T
  constexpr int ROWB = 2 * D + 32;       // bytes of a K or V row in LDS
  constexpr int LPR = D / 8;             // threads per staged row
  constexpr int PASS = kThreads / LPR;   // rows one pass of the workgroup stages
  static_assert(PASS * KS == kKeyStep, "staging covers the step");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kKeyStep * ROWB];
  unsigned char* const sk = smem;
  unsigned char* const sv = smem + kKeyStep * ROWB;

  // workgroup blockIdx.x = h slots + x: slot x of KV head h. The sequence and the tile of a slot: seq_of_slot (workgroup-uniform, scalar loads)
  fa2d::Split sp;
  sp.h = blockIdx.x / slots;
  const unsigned slot = blockIdx.x - sp.h * slots;
  int c0, T;
  const int bs = GM::seq_of_slot(cu_q, B, total_q, ga, slot, c0, T);
  if (bs < 0) return;  // a slot in front of the first sequence
  sp.b = (unsigned)bs, sp.bh = sp.b * (unsigned)kv.Hkv + sp.h, sp.s = 0, sp.lo = 0;
  const int gsz = GM::size(ga), R = GM::times(T, ga), Hq = GM::times(kv.Hkv, ga);
  const unsigned tile = slot - GM::slot_of(c0, ga, bs);
  if (tile >= (unsigned)((R + kRowTile - 1) / kRowTile)) return;               // a slot behind the sequence's last tile (T = 0: every one)
  const int len = min(max(seqlens[sp.b], 0), kv.nmax());
  const int row0 = (int)tile * kRowTile;                                        // < R
  const int rows = min(kRowTile, R - row0);
  const int n_end = len - (T - 1 - GM::tok(row0 + rows - 1, ga));               // the keys the tile's last token sees
  const size_t row_bt = (size_t)c0 * Hq + (size_t)sp.h * gsz;                     // packed output row of (t, g): row_bt + t Hq + g

  if (n_end <= 0) {  // no row of the tile sees a key
    for (int idx = threadIdx.x; idx < rows * LPR; idx += kThreads) {
      const int r = row0 + idx / LPR, t = GM::tok(r, ga);
      const size_t row = row_bt + (size_t)t * Hq + GM::head(r, t, gsz);
      *reinterpret_cast<b8*>(o + row * D + 8 * (idx % LPR)) = b8{};
      if (lse && idx % LPR == 0) lse[row] = FA2D_NEG_INF;
    }
    return;
  }
  const unsigned n = (unsigned)n_end;
  // the first step any row of the tile needs: the one that holds the lower edge of its first token; < n, as that token's edge is below its keys
  const unsigned k_begin = (unsigned)window_edge(len - (T - 1 - GM::tok(row0, ga)), W) & ~(unsigned)(kKeyStep - 1);

  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i16 = lane & 15, g4 = lane >> 4;
  const int wr0 = row0 + w * kWaveRows;  // the wave's first row; wave-uniform from here on
  const int n_wave = wr0 < R ? len - (T - 1 - GM::tok(min(wr0 + kWaveRows, R) - 1, ga)) : 0;  // the keys its last token sees
  const int lo_wave = wr0 < R ? window_edge(len - (T - 1 - GM::tok(wr0, ga)), W) : 0;         // the lower edge of its first token

  // the query fragments, the keys each lane's query sees (lo_q <= key < nq), and per row tile the keys its first token sees (0 for a tile with
  // rows >= R: those always take the select) and the lower edge of its last
  b8 qf[kMT][KS];
  unsigned nq[kMT], lo_q[kMT], n_tile[kMT], lo_tile[kMT];
#pragma unroll
  for (int qb = 0; qb < kMT; ++qb) {
    const int rf = wr0 + 16 * qb, r = rf + i16;
    const int t = GM::tok(r, ga), g = GM::head(r, t, gsz);
    nq[qb] = r < R ? (unsigned)max(len - (T - 1 - t), 0) : 0u;
    lo_q[qb] = (unsigned)window_edge((int)nq[qb], W);
    n_tile[qb] = rf + 16 <= R ? (unsigned)max(len - (T - 1 - GM::tok(rf, ga)), 0) : 0u;
    lo_tile[qb] = rf + 16 <= R ? (unsigned)window_edge(len - (T - 1 - GM::tok(rf + 15, ga)), W) : 0u;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      b8 x = {};
      if (r < R) x = *reinterpret_cast<const b8*>(q + (row_bt + (size_t)t * Hq + g) * D + 32 * ks + 8 * g4);
      qf[qb][ks] = x;
    }
  }

  // staging: this thread's column 8 (tid % LPR) .. + 7 of the rows tid / LPR + PASS i of a step
  const int s_row = threadIdx.x / LPR, s_col = threadIdx.x % LPR;
  const auto at = PL::at(kv, sp, D, 8 * s_col);
  if constexpr (PL::kFp8) scale_log2 *= PL::k_scale(kv, sp.h);  // the scale of the stored K codes goes into the score multiplier, once per workgroup
  // CAP only. FP8: k_scale inside the tanh; finite, so 0 pre = 0
  const SoftCapMul cm = {scale_log2, PL::kFp8 ? fminf(pre * PL::k_scale(kv, sp.h), 3.4028234664e38f) : pre, cap2};
  const float v_mul = PL::v_scale(kv, sp.h);                    // FP8 only
  using Piece = typename PL::Piece;
  struct Rows {
    Piece k[KS], v[KS];
  };
  auto lookup = [&](int (&pg)[KS], unsigned k0) {
#pragma unroll
    for (int i = 0; i < KS; ++i) pg[i] = kv.lookup(at, k0 + s_row + PASS * i, n);
  };
  auto load = [&](Rows& d, const int (&pg)[KS], unsigned k0) {
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      const unsigned r = k0 + s_row + PASS * i;
      PL::clear(d.k[i]), PL::clear(d.v[i]);
      if (r < n) {
        const size_t e = kv.elem(at, pg[i], r, D);
        d.k[i] = *reinterpret_cast<const Piece*>(at.k + e);
        d.v[i] = *reinterpret_cast<const Piece*>(at.v + e);
      }
    }
  };
  const int s_off = s_row * ROWB + 16 * s_col;                                          // + PASS i rows
  const unsigned char* k_ld = sk + i16 * ROWB + 16 * g4;                                // + 16 kb rows, + 64 ks bytes
  const unsigned char* v_ld = sv + (4 * g4 + (i16 >> 2)) * ROWB + 8 * (i16 & 3);       // transposing read: key rows 4 g4 .. + 3 (+ 16), dims 16 db + i16

  float m[kMT], l[kMT];
  f4 acc[kMT][DB];
#pragma unroll
  for (int qb = 0; qb < kMT; ++qb) {
    m[qb] = FA2D_NEG_INF, l[qb] = 0.0f;
#pragma unroll
    for (int db = 0; db < DB; ++db) acc[qb][db] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  }

  Rows cur;
  int pg[KS];
  lookup(pg, k_begin);
  load(cur, pg, k_begin);
  lookup(pg, k_begin + kKeyStep);
  for (unsigned k0 = k_begin; k0 < n; k0 += kKeyStep) {
    __syncthreads();  // every wave has read the step before
#pragma unroll
    for (int i = 0; i < KS; ++i) {
      *reinterpret_cast<b8*>(sk + s_off + PASS * i * ROWB) = PL::to_b8(cur.k[i]);  // FP8: the one conversion of an element
      *reinterpret_cast<b8*>(sv + s_off + PASS * i * ROWB) = PL::to_b8(cur.v[i]);
    }
    __syncthreads();
    Rows nxt;
    load(nxt, pg, k0 + kKeyStep);  // behind the last step every predicate is false: zeros, no access
    lookup(pg, k0 + 2 * kKeyStep);
    if ((int)k0 < n_wave && (int)(k0 + kKeyStep) > lo_wave) {  // wave-uniform: the step holds a key some row of the wave sees
      f4 st[kMT][kKB];
#pragma unroll
      for (int kb = 0; kb < kKB; ++kb) {
        b8 kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = *reinterpret_cast<const b8*>(k_ld + 16 * kb * ROWB + 64 * ks);
#pragma unroll
        for (int qb = 0; qb < kMT; ++qb) {
          st[qb][kb] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) st[qb][kb] = mfma(kf[ks], qf[qb][ks], st[qb][kb]);
        }
      }
      b8 pf[kMT][2];
#pragma unroll
      for (int qb = 0; qb < kMT; ++qb) {
        float alpha;
        // wave-uniform: every key of the step is inside the window of every row of the tile -- at or above the lower edge of its last row and
        // below the causal edge of its first
        const bool inside = k0 >= lo_tile[qb] && k0 + kKeyStep <= n_tile[qb];
        if constexpr (CAP) {
          if (inside)
            softmax_step_window_cap<false>(st[qb], k0 + 4 * g4, lo_q[qb], nq[qb], cm, m[qb], l[qb], alpha, pf[qb]);
          else
            softmax_step_window_cap<true>(st[qb], k0 + 4 * g4, lo_q[qb], nq[qb], cm, m[qb], l[qb], alpha, pf[qb]);
        } else {
          if (inside)
            softmax_step_window<false>(st[qb], k0 + 4 * g4, lo_q[qb], nq[qb], scale_log2, m[qb], l[qb], alpha, pf[qb]);
          else
            softmax_step_window<true>(st[qb], k0 + 4 * g4, lo_q[qb], nq[qb], scale_log2, m[qb], l[qb], alpha, pf[qb]);
        }
#pragma unroll
        for (int db = 0; db < DB; ++db) acc[qb][db] *= alpha;
      }
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          const unsigned char* a = v_ld + 32 * c * ROWB + 32 * db;
          const b8 vf = b8_cat(lds_read_tr(a), lds_read_tr(a + 16 * ROWB));
#pragma unroll
          for (int qb = 0; qb < kMT; ++qb) acc[qb][db] = mfma(vf, pf[qb][c], acc[qb][db]);
        }
    }
    cur = nxt;
  }

  // the row sums of the four lanes of a query, in a fixed order (both partners of a swap add the same pair); lane (g4, i16) holds dims
  // 16 db + 4 g4 .. + 3 of query i16. Then the sink of the row's head sp.h G + g, if there are sinks, joins the finished row (fold_sink), once,
  // and over FP8 pools v_scale multiplies the normalisation.
#pragma unroll
  for (int qb = 0; qb < kMT; ++qb) {
    float a, c;
    fa2d::swap_pair<16>(l[qb], a, c);
    l[qb] = a + c;
    fa2d::swap_pair<32>(l[qb], a, c);
    l[qb] = a + c;
    const int r = wr0 + 16 * qb + i16;
    if (r < R) {
      const int t = GM::tok(r, ga), g = GM::head(r, t, gsz);
      const size_t row = row_bt + (size_t)t * Hq + g;
      float f = 1.0f;  // kNone only
      if constexpr (SINKS == Sinks::kRequired) f = fold_sink(m[qb], l[qb], sink_log2(sinks, sp.h * gsz + g));
      if constexpr (SINKS == Sinks::kOptional) f = fold_sink(m[qb], l[qb], sink_log2_or_none(sinks, sp.h * gsz + g));
      float inv = l[qb] > 0.0f ? 1.0f / l[qb] : 0.0f;  // no visible key: O = 0, LSE = -inf
      if constexpr (PL::kFp8) inv *= v_mul;
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        if constexpr (SINKS == Sinks::kNone)
          *reinterpret_cast<b4*>(o + row * D + 16 * db + 4 * g4) = round4(acc[qb][db] * inv);
        else
          *reinterpret_cast<b4*>(o + row * D + 16 * db + 4 * g4) = round4(acc[qb][db] * f * inv);
      }
      if (lse && g4 == 0) lse[row] = l[qb] > 0.0f ? (m[qb] + __builtin_log2f(l[qb])) * 0.6931471805599453f : FA2D_NEG_INF;
    }
  }
