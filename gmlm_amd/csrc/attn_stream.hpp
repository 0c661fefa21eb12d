// Device bodies of the streaming attention kernels (K5/K7): forward, delta, dQ and dK/dV, written once for every head dim.
// The __global__ entry points of attn_kernels.hip (d = 64 / 96, two-dimensional grids) and attn_d128.hip (d = 128, 1-D grids)
// decode their grid into (tile, b, hd) and call one of these; tile sizes and the double-buffer switch are template arguments.
//   tile     : index of the workgroup's block of NW * 32 query rows (forward, dQ) or key rows (dK/dV)
//   b, hd    : batch (or packed sequence) and head
//   o_stride : row stride of out / out_lo / dout in elements (h * D)
#pragma once
#include "attn_common.hpp"

namespace gmlm {

// Tiling of the 4-wave families at head dim 64 and 128 (128 query rows per workgroup): bf16 streams 64-row K / V tiles double-
// buffered, fp32 32-row tiles in one buffer; dK/dV stages 32 query rows at a time.  attn_d32.hip has its own (QT = 64).
template <typename T> struct Cfg;
template <> struct Cfg<bf16_t> { static constexpr int KT = 64, QT = 32; static constexpr bool DBUF = true; };
template <> struct Cfg<float> { static constexpr int KT = 32, QT = 32; static constexpr bool DBUF = false; };

// Operands of the DISENT score mode (disentangled attention, attn_disent.hip): two fp32 tables [h, rows, w] with one row of `w`
// columns per (head, token), rows = all token rows of the call in memory order (what a GEMM batched over the heads writes), and
// the column table col[2m - 1], col[m - 1 + (i - j)] = the column that query i and key j of one sequence read in BOTH tables.
// An index past the column table and a column past the row are clamped: whatever the table holds, no load leaves the operands.
struct DisentTabs {
  const float* c;        // [h, rows, w]  content-to-position: row of the query
  const float* pt;       // [h, rows, w]  position-to-content: row of the key
  const int32_t* col;    // [2m - 1]
  int m, w;
};
__device__ __forceinline__ int disent_col(const DisentTabs& t, int delta) {
  int idx = t.m - 1 + delta;
  idx = idx < 0 ? 0 : (idx > 2 * t.m - 2 ? 2 * t.m - 2 : idx);
  const int c = t.col[idx];
  return c < 0 ? 0 : (c > t.w - 1 ? t.w - 1 : c);
}
// element offset of the table row of head hd and token row `row` (counted over the whole call: qbase + position)
__device__ __forceinline__ int64_t disent_row(const AttnParams& p, const DisentTabs& t, int64_t hd, int64_t row) {
  return (hd * (p.cu ? p.lq : p.b * p.lq) + row) * t.w;
}
// C[query row][col] + Pt[key row][col]; crow / prow point at the two rows
__device__ __forceinline__ float disent_term(const DisentTabs& t, const float* crow, const float* prow, int delta) {
  const int c = disent_col(t, delta);
  return crow[c] + prow[c];
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// CAUSAL (lq == lk, padded layout): query i sees the keys <= i below kv_len; the key loop ends at the workgroup's last query,
//   tiles wholly below the diagonal keep the compare-free path, a wave skips the arithmetic (never a barrier) of tiles past
//   its rows.  A wave computes a tile only if the tile's first key is <= its first query (both multiples of 32), so every
//   row of a computing wave has a valid key in every tile it computes: the running max stays finite.
// GQA: K / V are read from head `kvh` (query head hd / group) instead of hd.
// WINDOW (lq == lk, no dropout): query i sees the keys j with |i - j| <= window below kv_len.  The key loop covers
//   [q_tile0 - window, q_tile_end + window] within [0, kv_len) (block-uniform bounds); a wave skips the arithmetic (never a
//   barrier) of tiles outside the band of its 32 rows; tiles wholly inside that band and below kv_len keep the compare-free
//   path.  Unlike CAUSAL, a row can meet computed tiles in which it sees no key before the tile of its own diagonal (and, past
//   kv_len + window, in all of them): its running max is then -inf, and both exponentials are guarded to give 0, not NaN.
// BIAS (lq == lk): the score of query i and key j gets the additive term rel_bias[hd][rel_m - 1 + (j - i)] (fp32 table
//   [h, 2 * rel_m - 1], rel_m >= the longest sequence), read through the vector cache.  The scores are moved into the log2
//   domain right behind the QK^T chain, s' = s * scale * log2 e + bias * log2 e, and everything after it (running max,
//   deferral, exponentials) works on s' with a unit factor.  An index past the table (a padded query row or key) is clamped;
//   such a pair is masked or never stored.
// DISENT (lq == lk): the score of query i and key j gets C[row i][col[i - j]] + Pt[row j][col[i - j]] BEFORE the scale (struct
//   DisentTabs above), s' = (s + C + Pt) * scale * log2 e right behind the QK^T chain, and everything after it works on s' as
//   with BIAS.  The row of a query or key past its sequence is clamped into the sequence; such a pair is masked or never stored.
//   Dropout (DISENT and BIAS): the P V product takes P * (0 or 1) and the keep scale multiplies the output once, with 1 / l (bf16: the scaled
//   probability is never rounded, so O and the backward's delta = rowsum(dO * O) agree with D * dP to fp32 rounding; a row
//   with one key, P = 1, then has dS = 0 as it must).  Folded into the probabilities, the largest one of every row, exp2(0) = 1, would
//   become bf16(keep scale) each time, e.g. 256 / 230 -> 1.109375: 3.3e-3 low in every row, which biases delta and with it the
//   gradients of the tables that BIAS and DISENT add to the scores.
template <typename T, int D, int NW, bool DROP, int KT, bool DBUF, bool CAUSAL = false, bool GQA = false, bool WINDOW = false,
          bool BIAS = false, bool DISENT = false>
__device__ __forceinline__ void attn_fwd_body(const AttnParams& p, int64_t tile, int64_t b, int64_t hd, int64_t o_stride,
                                              int64_t kvh = 0, int64_t window = 0, const float* rel_bias = nullptr,
                                              int rel_m = 0, const DisentTabs* dt = nullptr) {
  static_assert(!(WINDOW && (CAUSAL || DROP)), "the band mask has no causal or dropout form");
  static_assert(!(BIAS && (CAUSAL || GQA || WINDOW)), "the relative-position bias has no causal, grouped or band form");
  static_assert(!(DISENT && (CAUSAL || GQA || WINDOW || BIAS)), "the disentangled terms have no causal, grouped, band or bias form");
  constexpr bool PRE = BIAS || DISENT;       // the scores are in the log2 domain before the running max
  constexpr int KB = KT / 32, NT = NW * 64, PITCH = D + Pad<T>::v, DB = D / 32, NBUF = DBUF ? 2 : 1;
  __shared__ __attribute__((aligned(16))) T ks[NBUF][KT * PITCH];
  __shared__ __attribute__((aligned(16))) T vs[NBUF][KT * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  int64_t lq_, lk_, qbase, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, qbase, kbase, lse_base);
  if (tile * (NW * 32) >= (false ? lk_ : lq_)) return;   // varlen: tile past this sequence (block-uniform)
  const int64_t q_row = tile * (NW * 32) + w * 32 + r;
  const bool q_ok = q_row < lq_;
  // a wave whose 32 queries all lie past the sequence (short packed sequences) only helps staging K/V
  const bool wave_live = tile * (NW * 32) + w * 32 < lq_;
  const int64_t kvlen = clamp_kvlen(p, b, lk_);
  const T* qg = static_cast<const T*>(p.q) + (qbase + (q_ok ? q_row : 0)) * p.q_stride + hd * D;
  const int64_t khd = GQA ? kvh : hd;
  const T* kg = static_cast<const T*>(p.k) + kbase * p.k_stride + khd * D;
  const T* vg = static_cast<const T*>(p.v) + kbase * p.v_stride + khd * D;
  RowFrag<T, D> qf;
  qf.load(qg, q_ok, h);
  f32x16 o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[d][i] = 0.f;
  float m = -INFINITY, l = 0.f;              // running max / sum in the log2 domain (scores * scale * log2 e)
  const float sl2 = p.scale * kLog2e;
  // dropout hash input of this lane's query (+ 2h: the lane half's keys sit 4 further on, i.e. 2 key pairs)
  const uint32_t dq_u = drop_base(attn_seed(p), lse_base) + (uint32_t)(q_row >> 1) * kDropC1 + (uint32_t)(2 * h) * kDropC2;
  const int q_odd = (int)(q_row & 1);
  const int64_t q_tile0 = tile * (NW * 32), q_wave0 = q_tile0 + w * 32;
  int64_t kv_end = CAUSAL && q_tile0 + NW * 32 < kvlen ? q_tile0 + NW * 32 : kvlen;   // keys this workgroup can see
  if (WINDOW && q_tile0 + NW * 32 + window < kv_end) kv_end = q_tile0 + NW * 32 + window;   // last query NW*32 - 1 sees up to + window
  const int t0 = WINDOW && q_tile0 > window ? (int)((q_tile0 - window) / KT) : 0;          // first key tile inside the band
  const int ntiles = (int)((kv_end + KT - 1) / KT);
  TileRegs<T, D, KT, NT> kr, vr;
  kr.init(p.k_stride, tid);
  vr.init(p.v_stride, tid);
  if (ntiles > t0) {
    kr.load(kg, p.k_stride, (int64_t)t0 * KT, lk_, tid);
    vr.load(vg, p.v_stride, (int64_t)t0 * KT, lk_, tid);
    kr.store(ks[0], tid);
    vr.store(vs[0], tid);
  }
  __syncthreads();
  for (int t = t0; t < ntiles; ++t) {
    const int64_t kv0 = (int64_t)t * KT;
    const int cur = DBUF ? ((t - t0) & 1) : 0;
    const bool more = t + 1 < ntiles;
    if (DBUF && more) {
      kr.load(kg, p.k_stride, kv0 + KT, lk_, tid);
      vr.load(vg, p.v_stride, kv0 + KT, lk_, tid);
    }
    if (wave_live && (!CAUSAL || kv0 <= q_wave0) && (!WINDOW || (kv0 <= q_wave0 + 31 + window && kv0 + KT - 1 + window >= q_wave0))) {
    f32x16 s[KB];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) s[kb][i] = 0.f;
      mma_rows<D>(ks[cur], PITCH, kb * 32, qf, s[kb], r, h);
      if constexpr (BIAS) {
        const float* bh = rel_bias + hd * (2 * rel_m - 1) + (rel_m - 1);      // entry 0 = the diagonal
        const int rel0 = (int)(kv0 - q_row) + kb * 32;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          int rel = rel0 + acc_row(i, h);
          rel = rel < 1 - rel_m ? 1 - rel_m : (rel > rel_m - 1 ? rel_m - 1 : rel);
          s[kb][i] = fmaf(s[kb][i], sl2, bh[rel] * kLog2e);
        }
      }
      if constexpr (DISENT) {
        const float* crow = dt->c + disent_row(p, *dt, hd, qbase + (q_ok ? q_row : 0));
        const int qi_ = (int)(q_row < (1 << 30) ? q_row : (1 << 30));
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = (int)kv0 + kb * 32 + acc_row(i, h), kc = key < (int)lk_ ? key : (int)lk_ - 1;   // lk_ > 0 inside the loop
          s[kb][i] = (s[kb][i] + disent_term(*dt, crow, dt->pt + disent_row(p, *dt, hd, kbase + kc), qi_ - key)) * sl2;
        }
      }
    }
    float rmax = -INFINITY;
    // whole tile valid (block-uniform; causal: and below the diagonal; window: and inside the band of all 32 rows of the
    // wave, wave-uniform): no per-key compare
    if (kv0 + KT <= kvlen && (!CAUSAL || kv0 + KT - 1 <= q_tile0) &&
        (!WINDOW || (kv0 + window >= q_wave0 + 31 && kv0 + KT - 1 <= q_wave0 + window))) {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) rmax = fmaxf(rmax, s[kb][i]);
    } else {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int64_t key = kv0 + kb * 32 + acc_row(i, h);
          const float v = (key < kvlen && (!CAUSAL || key <= q_row) && (!WINDOW || (key <= q_row + window && key + window >= q_row))) ? s[kb][i] : -INFINITY;
          s[kb][i] = v;
          rmax = fmaxf(rmax, v);
        }
    }
    rmax = xhalf_max(rmax);
    // deferred rescale: keep the old reference max while the new one exceeds it by < 2^kDefer (probabilities
    // then stay <= 2^kDefer, harmless in fp32 / bf16); the O and l rescale is skipped for the whole wave then
    float m_new = fmaxf(m, PRE ? rmax : rmax * sl2);             // finite: key kv0 is always valid (WINDOW: -inf while the row has seen no key)
    // WINDOW: a row still at -inf that stays there changes nothing (-inf - -inf would be NaN and end the deferral for the wave)
    const bool keep = __all((WINDOW && m_new == -INFINITY) || m_new - m <= kDefer);   // m = -inf (first tile) -> false
    float alpha = 1.f;
    if (keep) m_new = m;
    else alpha = (WINDOW && m == -INFINITY) ? 0.f : fast_exp2(m - m_new);   // m = -inf -> 0 (WINDOW: also when m_new = -inf)
    const float m_ref = (WINDOW && m_new == -INFINITY) ? 0.f : m_new;       // exponent reference: exp2(-inf - 0) = 0 for a row with no key yet
    float rsum = 0.f;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int i = 0; i < 16; i += 2) {
        const float e0 = fast_exp2(PRE ? s[kb][i] - m_ref : fmaf(s[kb][i], sl2, -m_ref));       // masked: exp2(-inf) = 0
        const float e1 = fast_exp2(PRE ? s[kb][i + 1] - m_ref : fmaf(s[kb][i + 1], sl2, -m_ref));
        rsum += e0 + e1;                                               // the normaliser uses the un-dropped probabilities
        if (DROP) {
          float m0, m1;                                // keys (k, k+1): (kv0 + kb*32 + acc_row(i, 0)) >> 1 pairs on from the tile start
          drop_pair_q(dq_u + ((uint32_t)(t * (KT / 2)) + (uint32_t)((kb * 32 + acc_row(i, 0)) >> 1)) * kDropC2, q_odd, p.drop_thresh, (DISENT || BIAS) ? 1.f : p.keep_scale, m0, m1);
          s[kb][i] = e0 * m0;
          s[kb][i + 1] = e1 * m1;
        } else {
          s[kb][i] = e0;
          s[kb][i + 1] = e1;
        }
      }
    rsum = xhalf_sum(rsum);
    l = l * alpha + rsum;
    m = m_new;
    if (!keep) {
#pragma unroll
      for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[d][i] *= alpha;
    }
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) mma_acc<D>(vs[cur], PITCH, kb * 32, s[kb], o, lane);
    }
    if (DBUF) {
      if (more) {
        kr.store(ks[cur ^ 1], tid);
        vr.store(vs[cur ^ 1], tid);
      }
      __syncthreads();
    } else if (more) {
      __syncthreads();
      kr.load(kg, p.k_stride, kv0 + KT, lk_, tid);
      vr.load(vg, p.v_stride, kv0 + KT, lk_, tid);
      kr.store(ks[0], tid);
      vr.store(vs[0], tid);
      __syncthreads();
    }
  }
  if (q_ok) {
    const float inv = l > 0.f ? ((DISENT || BIAS) && DROP ? p.keep_scale : 1.f) / l : 0.f;
    T* og = static_cast<T*>(p.o_w) + (qbase + q_row) * o_stride + hd * D;
#pragma unroll
    for (int d = 0; d < DB; ++d) store_t<T>(og + d * 32, o[d], inv, h);
    if constexpr (sizeof(T) == 2) {
      if (p.o_lo_w) {
        T* olg = static_cast<T*>(p.o_lo_w) + (qbase + q_row) * o_stride + hd * D;
#pragma unroll
        for (int d = 0; d < DB; ++d) store_t_lo(olg + d * 32, o[d], inv, h);
      }
    }
    if (h == 0 && p.lse_w) p.lse_w[lse_base + q_row] = l > 0.f ? (m + __log2f(l)) * kLn2 : -INFINITY;
  }
}

// ------------------------------------------------------------------------------------------------
// backward: delta[b,h,q] = sum_d dO * O   (O = o + o_lo when the forward stored the bf16 residual of its output)
// ------------------------------------------------------------------------------------------------
// a group of d/V lanes owns one (b, q, h) row: the wave reads 64 x 16 contiguous bytes per instruction
template <typename T>
__device__ __forceinline__ void attn_delta_body(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                int64_t rows /* b*lq*h */, int d, int64_t lq, int64_t hn,
                                                float* __restrict__ delta) {
  constexpr int V = Store<T>::kVec;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lanes = d / V <= 8 ? 8 : (d / V <= 16 ? 16 : 32);
  const int64_t row = gid / lanes;
  const int c = (int)(gid % lanes);
  float acc = 0.f;
  if (row < rows && c < d / V) {
    float a[V], g[V];
    Store<T>::ldv(o + row * d + c * V, a);
    Store<T>::ldv(dout + row * d + c * V, g);
    if (o_lo) {
      float al[V];
      Store<T>::ldv(o_lo + row * d + c * V, al);
#pragma unroll
      for (int v = 0; v < V; ++v) a[v] += al[v];
    }
#pragma unroll
    for (int v = 0; v < V; ++v) acc += a[v] * g[v];
  }
  for (int off = lanes >> 1; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (row < rows && c == 0) {
    const int64_t hd = row % hn, bq = row / hn, q = bq % lq, b = bq / lq;
    delta[(b * hn + hd) * lq + q] = acc;         // packed mode passes b = 1, lq = total rows: [h, total_rows]
  }
}

// ------------------------------------------------------------------------------------------------
// backward: dQ.  workgroup = NW*32 queries, loop over key tiles.
//   S^T = K Q^T, P^T = exp(scale*S^T - lse[q]), dP^T = V dO^T, dS^T = P^T*(dP^T - delta[q]),
//   dQ^T += K^T dS^T  (all with the query on the lane)
// ------------------------------------------------------------------------------------------------
// d128::dq_kernel (attn_d128.hip) keeps a copy of this text for its register budget: a change here belongs there too.
// CAUSAL / GQA as in attn_fwd_body.  The bf16 extra contraction step cannot express a causal mask (it is not rank-1): the one
// 32-key block that crosses a wave's diagonal selects P = 0 explicitly before dS (a select, not a product: a score above
// the diagonal is not bounded by lse and may have overflowed).
// WINDOW as in attn_fwd_body: the same key loop; a 32-key block outside the band of the wave's rows is skipped, one that the
// band edge crosses selects P = 0 explicitly before dS, exactly as the diagonal block does.  A query that saw no key has
// lse = -inf: it is given probability 0 everywhere, like a row past the sequence (dQ = 0).
// BIAS as in attn_fwd_body: bias * log2 e is added to the exponent (bf16: to what leaves the MFMA chain, where a masked key
// still sits near -2^100); dQ itself has no bias term.  The gradient of the table is a kernel of its own (attn_relbias.hip).
// DISENT as in attn_fwd_body: (C + Pt) * scale * log2 e takes the place of bias * log2 e; dQ is the content-content part only,
// the gradients of the two tables are kernels of their own (attn_disent.hip).
template <typename T, int D, int NW, bool DROP, int KT, bool DBUF, bool CAUSAL = false, bool GQA = false, bool WINDOW = false,
          bool BIAS = false, bool DISENT = false>
__device__ __forceinline__ void attn_dq_body(const AttnParams& p, int64_t tile, int64_t b, int64_t hd, int64_t o_stride,
                                             int64_t kvh = 0, int64_t window = 0, const float* rel_bias = nullptr,
                                             int rel_m = 0, const DisentTabs* dt = nullptr) {
  static_assert(!(WINDOW && (CAUSAL || DROP)), "the band mask has no causal or dropout form");
  static_assert(!(BIAS && (CAUSAL || GQA || WINDOW)), "the relative-position bias has no causal, grouped or band form");
  static_assert(!(DISENT && (CAUSAL || GQA || WINDOW || BIAS)), "the disentangled terms have no causal, grouped, band or bias form");
  constexpr bool PRE = BIAS || DISENT;       // an additive exponent term b0 / b1 per score
  constexpr int KB = KT / 32, NT = NW * 64, PITCH = D + Pad<T>::v, DB = D / 32, NBUF = DBUF ? 2 : 1;
  __shared__ __attribute__((aligned(16))) T ks[NBUF][KT * PITCH];
  __shared__ __attribute__((aligned(16))) T vs[NBUF][KT * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  int64_t lq_, lk_, qbase, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, qbase, kbase, lse_base);
  if (tile * (NW * 32) >= (false ? lk_ : lq_)) return;   // varlen: tile past this sequence (block-uniform)
  const int64_t q_row = tile * (NW * 32) + w * 32 + r;
  const bool q_ok = q_row < lq_;
  const bool wave_live = tile * (NW * 32) + w * 32 < lq_;   // else: staging helper only
  const int64_t kvlen = clamp_kvlen(p, b, lk_);
  const int64_t qr = q_ok ? q_row : 0;
  const int64_t khd = GQA ? kvh : hd;
  const T* kg = static_cast<const T*>(p.k) + kbase * p.k_stride + khd * D;
  const T* vg = static_cast<const T*>(p.v) + kbase * p.v_stride + khd * D;
  RowFrag<T, D> qf, dof;
  qf.load(static_cast<const T*>(p.q) + (qbase + qr) * p.q_stride + hd * D, q_ok, h);
  dof.load(static_cast<const T*>(p.dout) + (qbase + qr) * o_stride + hd * D, q_ok, h);
  const float sl2 = p.scale * kLog2e;
  const float lse_q = q_ok ? p.lse[lse_base + q_row] : INFINITY;
  const bool q_on = q_ok && !(WINDOW && lse_q == -INFINITY);   // WINDOW: a query with no visible key
  const float lse2 = q_on ? lse_q * kLog2e : INFINITY;
  const float dl = q_ok ? p.delta[lse_base + q_row] : 0.f;
  const int kvl = (int)(kvlen < (1 << 30) ? kvlen : (1 << 30));
  const uint32_t dq_u = drop_base(attn_seed(p), lse_base) + (uint32_t)(q_row >> 1) * kDropC1 + (uint32_t)(2 * h) * kDropC2;
  const int q_odd = (int)(q_row & 1);
  // bf16: the per-score fma / compare / select work rides in the MFMA chains (as in the pipelined forward).  Q is
  // pre-multiplied by scale * log2 e (the SAME rounding the forward applies), and each chain starts with one extra
  // contraction step  [1 1 m 0 ..] x [-lse_hi -lse_lo -2^100 0 ..]^T  (m = 1 for a masked key): scores leave the
  // chain as s*scale*log2e - lse, masked keys at about -1.3e30, so P = exp2(.) with no further arithmetic; without
  // dropout the dP chain starts from  [1 1 0 ..] x [-delta_hi -delta_lo 0 ..]^T  and dS = P * (dP - delta) is one multiply.
  // lse / delta are split into two bf16 terms (hi + lo: relative error 2^-17).
  constexpr bool FOLD = sizeof(T) == 2;
  bf16x8 ones_a, ext_s, ext_dp;
  if constexpr (FOLD) {
#pragma unroll
    for (int s_ = 0; s_ < D / 16; ++s_)
#pragma unroll
      for (int j = 0; j < 8; ++j) qf.v[s_][j] = (__bf16)((float)qf.v[s_][j] * sl2);
    const float l2 = q_on ? lse2 : 0x1p100f;                 // a row past the sequence: probability 0 everywhere
    const float lh = (float)(__bf16)l2, ll = (float)(__bf16)(l2 - lh);
    const float dh = (float)(__bf16)dl, dlo = (float)(__bf16)(dl - dh);
#pragma unroll
    for (int j = 0; j < 8; ++j) { ones_a[j] = (__bf16)0.f; ext_s[j] = (__bf16)0.f; ext_dp[j] = (__bf16)0.f; }
    if (h == 0) {
      ones_a[0] = (__bf16)1.f; ones_a[1] = (__bf16)1.f;
      ext_s[0] = (__bf16)(-lh); ext_s[1] = (__bf16)(-ll); ext_s[2] = (__bf16)(-0x1p100f);
      ext_dp[0] = (__bf16)(-dh); ext_dp[1] = (__bf16)(-dlo);
    }
  }
  f32x16 dq[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[d][i] = 0.f;
  const int64_t q_tile0 = tile * (NW * 32), q_wave0 = q_tile0 + w * 32;
  int64_t kv_end = CAUSAL && q_tile0 + NW * 32 < kvlen ? q_tile0 + NW * 32 : kvlen;   // keys this workgroup can see
  if (WINDOW && q_tile0 + NW * 32 + window < kv_end) kv_end = q_tile0 + NW * 32 + window;   // last query NW*32 - 1 sees up to + window
  const int qi = (int)(q_row < (1 << 30) ? q_row : (1 << 30));
  const int t0 = WINDOW && q_tile0 > window ? (int)((q_tile0 - window) / KT) : 0;          // first key tile inside the band
  const int ntiles = (int)((kv_end + KT - 1) / KT);
  TileRegs<T, D, KT, NT> kr, vr;
  kr.init(p.k_stride, tid);
  vr.init(p.v_stride, tid);
  if (ntiles > t0) {
    kr.load(kg, p.k_stride, (int64_t)t0 * KT, lk_, tid);
    vr.load(vg, p.v_stride, (int64_t)t0 * KT, lk_, tid);
    kr.store(ks[0], tid);
    vr.store(vs[0], tid);
  }
  __syncthreads();
  for (int t = t0; t < ntiles; ++t) {
    const int64_t kv0 = (int64_t)t * KT;
    const int cur = DBUF ? ((t - t0) & 1) : 0;
    const bool more = t + 1 < ntiles;
    if (DBUF && more) {
      kr.load(kg, p.k_stride, kv0 + KT, lk_, tid);
      vr.load(vg, p.v_stride, kv0 + KT, lk_, tid);
    }
    if (wave_live) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      if constexpr (CAUSAL) {
        if (kv0 + kb * 32 > q_wave0) continue;                 // key block above this wave's rows (wave-uniform; no barrier inside)
      }
      const bool diag = CAUSAL && kv0 + kb * 32 == q_wave0;    // the only key block that crosses this wave's diagonal
      if constexpr (WINDOW) {
        if (kv0 + kb * 32 > q_wave0 + 31 + window || kv0 + kb * 32 + 31 + window < q_wave0) continue;   // key block outside the band of this wave's rows (wave-uniform)
      }
      // a key block that the band edge crosses for some row of the wave (wave-uniform)
      const bool edge = WINDOW && !(kv0 + kb * 32 + window >= q_wave0 + 31 && kv0 + kb * 32 + 31 <= q_wave0 + window);
      f32x16 s, dp;
#pragma unroll
      for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
      const bool full = kv0 + (kb + 1) * 32 <= kvlen;          // block-uniform
      if constexpr (FOLD) {
        bf16x8 oa = ones_a;
        // only a sequence's last key block is partial.  Without the hint the fix-up is speculated and the KB key blocks fuse into
        // one region: d = 64, 4 waves 166 -> 200 VGPRs, 3 -> 2 waves per SIMD (guard: test_streaming_dq_mfma_chains_stay_per_key_block)
        if (__builtin_expect(!full, 0)) oa[2] = (h == 0 && (int)kv0 + kb * 32 + r >= kvl) ? (__bf16)1.f : (__bf16)0.f;   // A row r = key r of the block
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(oa, ext_s, s, 0, 0, 0);
        if (!DROP) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones_a, ext_dp, dp, 0, 0, 0);
      }
      mma_rows<D>(ks[cur], PITCH, kb * 32, qf, s, r, h);
      mma_rows<D>(vs[cur], PITCH, kb * 32, dof, dp, r, h);
#pragma unroll
      for (int i = 0; i < 16; i += 2) {
        float p0, p1;
        float b0 = 0.f, b1 = 0.f;                                  // BIAS: bias * log2 e of keys key, key + 1
        if constexpr (BIAS) {
          const float* bh = rel_bias + hd * (2 * rel_m - 1) + (rel_m - 1);
          const int rel = (int)kv0 + kb * 32 + acc_row(i, h) - qi, lo = 1 - rel_m, hi = rel_m - 1;   // each index clamped on its own
          b0 = bh[rel < lo ? lo : (rel > hi ? hi : rel)] * kLog2e;
          b1 = bh[rel + 1 < lo ? lo : (rel + 1 > hi ? hi : rel + 1)] * kLog2e;
        }
        if constexpr (DISENT) {
          const float* crow = dt->c + disent_row(p, *dt, hd, qbase + qr);
          const int key = (int)kv0 + kb * 32 + acc_row(i, h), last = (int)lk_ - 1;   // each key row clamped on its own
          b0 = disent_term(*dt, crow, dt->pt + disent_row(p, *dt, hd, kbase + (key < last ? key : last)), qi - key) * sl2;
          b1 = disent_term(*dt, crow, dt->pt + disent_row(p, *dt, hd, kbase + (key + 1 < last ? key + 1 : last)), qi - key - 1) * sl2;
        }
        if constexpr (FOLD) {
          p0 = fast_exp2(PRE ? s[i] + b0 : s[i]);
          p1 = fast_exp2(PRE ? s[i + 1] + b1 : s[i + 1]);
        } else {
          const int key = (int)kv0 + kb * 32 + acc_row(i, h);      // even; registers i, i+1 = keys key, key+1
          // a masked key gets exponent -inf through a select (no branch around the exp); whole blocks skip the test;
          // a query row past the sequence has lse = +inf, i.e. probability 0 everywhere
          float a0 = fmaf(s[i], sl2, PRE ? b0 - lse2 : -lse2), a1 = fmaf(s[i + 1], sl2, PRE ? b1 - lse2 : -lse2);
          if (!full) { a0 = key < kvl ? a0 : -INFINITY; a1 = key + 1 < kvl ? a1 : -INFINITY; }
          p0 = fast_exp2(a0); p1 = fast_exp2(a1);
        }
        if constexpr (CAUSAL) {
          if (diag) {
            const int kq = (int)kv0 + kb * 32 + acc_row(i, h);
            p0 = kq <= qi ? p0 : 0.f;
            p1 = kq + 1 <= qi ? p1 : 0.f;
          }
        }
        if constexpr (WINDOW) {
          if (edge) {
            const int kq = (int)kv0 + kb * 32 + acc_row(i, h), wi = (int)window;    // window < 2^30 (host check)
            p0 = (kq <= qi + wi && kq + wi >= qi) ? p0 : 0.f;
            p1 = (kq + 1 <= qi + wi && kq + 1 + wi >= qi) ? p1 : 0.f;
          }
        }
        if (FOLD && !DROP) {
          s[i] = p0 * dp[i];
          s[i + 1] = p1 * dp[i + 1];
        } else {
          float m0 = 1.f, m1 = 1.f;
          if (DROP) drop_pair_q(dq_u + ((uint32_t)(t * (KT / 2)) + (uint32_t)((kb * 32 + acc_row(i, 0)) >> 1)) * kDropC2, q_odd, p.drop_thresh, p.keep_scale, m0, m1);
          s[i] = p0 * (dp[i] * m0 - dl);
          s[i + 1] = p1 * (dp[i + 1] * m1 - dl);
        }
      }
      mma_acc<D>(ks[cur], PITCH, kb * 32, s, dq, lane);
    }
    }
    if (DBUF) {
      if (more) {
        kr.store(ks[cur ^ 1], tid);
        vr.store(vs[cur ^ 1], tid);
      }
      __syncthreads();
    } else if (more) {
      __syncthreads();
      kr.load(kg, p.k_stride, kv0 + KT, lk_, tid);
      vr.load(vg, p.v_stride, kv0 + KT, lk_, tid);
      kr.store(ks[0], tid);
      vr.store(vs[0], tid);
      __syncthreads();
    }
  }
  if (q_ok) {
    T* og = static_cast<T*>(p.dq) + (qbase + q_row) * p.dq_stride + hd * D;
#pragma unroll
    for (int d = 0; d < DB; ++d) store_t<T>(og + d * 32, dq[d], p.scale, h);
  }
}

// ------------------------------------------------------------------------------------------------
// backward: dK, dV.  workgroup = 128 keys (32 per wave), loop over query tiles of 32.
//   S = Q K^T, P = exp(scale*S - lse[q]), dV^T += dO^T P, dP = dO V^T, dS = P*(dP - delta[q]),
//   dK^T += Q^T dS   (all with the key on the lane, the query in the accumulator registers)
// ------------------------------------------------------------------------------------------------
// QT = query rows staged per barrier: 32 or 64 with two LDS buffers (long sequences: loads of tile t+1 under the MFMAs
// of tile t), or 128 in one buffer for sequences of <= 128 tokens (the whole sequence behind ONE barrier: at
// 16-128 tokens the per-tile barrier / LDS round trip, not the MFMA work, sets the block's lifetime).
// WINDOW (lq == lk, no dropout): the query loop covers [k_tile0 - window, k_tile_end + window] within [0, lq) (block-uniform);
// a 32-query block outside the band of the wave's keys is skipped, one that the band edge crosses selects P = 0 before dS; a
// query with lse = -inf (no visible key) is staged with lse = +inf, i.e. probability 0, and adds nothing to dK or dV.
// BIAS as in attn_dq_body, with the key on the lane: register i holds query q0 + qb * 32 + acc_row(i, h), so the table index
// falls as i rises.
// DISENT as in attn_dq_body, with the key on the lane: the Pt row is the lane's own, the C row changes with the register.
template <typename T, int D, int NW, bool DROP, int QT, bool DBUF, bool WINDOW = false, bool BIAS = false, bool DISENT = false>
__device__ __forceinline__ void attn_dkv_body(const AttnParams& p, int64_t tile, int64_t b, int64_t hd, int64_t o_stride,
                                              int64_t window = 0, const float* rel_bias = nullptr, int rel_m = 0,
                                              const DisentTabs* dt = nullptr) {
  static_assert(!(WINDOW && DROP), "the band mask has no dropout form");
  static_assert(!(BIAS && WINDOW), "the relative-position bias has no band form");
  static_assert(!(DISENT && (WINDOW || BIAS)), "the disentangled terms have no band or bias form");
  constexpr bool PRE = BIAS || DISENT;       // an additive exponent term per score
  constexpr int NT = NW * 64, PITCH = D + Pad<T>::v, DB = D / 32, NBUF = DBUF ? 2 : 1;
  __shared__ __attribute__((aligned(16))) T qs[NBUF][QT * PITCH];
  __shared__ __attribute__((aligned(16))) T dos[NBUF][QT * PITCH];
  __shared__ __attribute__((aligned(16))) float lse_s[NBUF][QT];
  __shared__ __attribute__((aligned(16))) float dl_s[NBUF][QT];
  // bf16: per query row, the A fragments of the extra contraction steps (see attn_dq_body): 16 elements each,
  // [-lse_hi -lse_lo -2^100 0 x 13] and [-delta_hi -delta_lo 0 x 14]; the key side holds [1 1 masked 0 ..] in registers
  constexpr bool FOLD = sizeof(T) == 2;
  __shared__ __attribute__((aligned(16))) bf16_t ext_s[FOLD ? NBUF : 1][FOLD ? QT * 16 : 8];
  __shared__ __attribute__((aligned(16))) bf16_t ext_d[FOLD ? NBUF : 1][FOLD ? QT * 16 : 8];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  int64_t lq_, lk_, qbase, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, qbase, kbase, lse_base);
  if (tile * (NW * 32) >= (true ? lk_ : lq_)) return;   // varlen: tile past this sequence (block-uniform)
  const int64_t kvlen = clamp_kvlen(p, b, lk_);
  const int64_t key = tile * (NW * 32) + w * 32 + r;
  const int64_t k_tile0 = tile * (NW * 32), k_wave0 = k_tile0 + w * 32;
  const int ki = (int)(key < (1 << 30) ? key : (1 << 30));
  const bool key_in = key < lk_;           // row exists in memory
  const bool key_ok = key < kvlen;          // takes part in the softmax
  const bool wave_live = tile * (NW * 32) + w * 32 < kvlen;   // else: staging helper only (dK = dV = 0)
  const int64_t kr_ = key_in ? key : 0;
  RowFrag<T, D> kf, vf;
  kf.load(static_cast<const T*>(p.k) + (kbase + kr_) * p.k_stride + hd * D, key_in, h);
  vf.load(static_cast<const T*>(p.v) + (kbase + kr_) * p.v_stride + hd * D, key_in, h);
  const T* qg = static_cast<const T*>(p.q) + qbase * p.q_stride + hd * D;
  const T* dog = static_cast<const T*>(p.dout) + qbase * o_stride + hd * D;
  const float* lse_g = p.lse + lse_base;
  const float* dl_g = p.delta + lse_base;
  const float sl2 = p.scale * kLog2e;
  const uint32_t dk_u = drop_base(attn_seed(p), lse_base) + (uint32_t)(key >> 1) * kDropC2 + (uint32_t)(2 * h) * kDropC1;   // + 2h: the lane half's queries sit 4 further on
  const int k_odd = (int)(key & 1);
  bf16x8 ones_k, ones_2;
  if constexpr (FOLD) {
    // K' = bf16(K * scale * log2 e) (one more bf16 rounding, the size of the one the forward applies to Q)
#pragma unroll
    for (int s_ = 0; s_ < D / 16; ++s_)
#pragma unroll
      for (int j = 0; j < 8; ++j) kf.v[s_][j] = (__bf16)((float)kf.v[s_][j] * sl2);
#pragma unroll
    for (int j = 0; j < 8; ++j) { ones_k[j] = (__bf16)0.f; ones_2[j] = (__bf16)0.f; }
    if (h == 0) {
      ones_k[0] = ones_2[0] = (__bf16)1.f; ones_k[1] = ones_2[1] = (__bf16)1.f;
      ones_k[2] = key_ok ? (__bf16)0.f : (__bf16)1.f;        // this lane's key is masked: its scores get -2^100
    }
  }
  f32x16 dk[DB], dv[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk[d][i] = 0.f; dv[d][i] = 0.f; }
  // a whole workgroup past kv_len has nothing to accumulate (block-uniform condition)
  const bool block_live = tile * (NW * 32) < kvlen;
  if (block_live) {
    const int64_t q_end = WINDOW && k_tile0 + NW * 32 + window < lq_ ? k_tile0 + NW * 32 + window : lq_;   // queries that see this workgroup's keys
    const int t0 = WINDOW && k_tile0 > window ? (int)((k_tile0 - window) / QT) : 0;
    const int ntiles = (int)((q_end + QT - 1) / QT);
    TileRegs<T, D, QT, NT> qr, dor;
    qr.init(p.q_stride, tid);
    dor.init(o_stride, tid);
    float lr = 0.f, dr = 0.f;
    auto load_small = [&](int64_t q0) {
      if (tid < QT) {
        const bool ok = q0 + tid < lq_;
        lr = ok ? lse_g[q0 + tid] * kLog2e : INFINITY;     // +inf: probability 0 for a row past the sequence
        if (WINDOW && lr == -INFINITY) lr = INFINITY;      // a query with no visible key: probability 0 as well
        dr = ok ? dl_g[q0 + tid] : 0.f;
      }
    };
    auto store_small = [&](int buf) {
      if (tid < QT) {
        lse_s[buf][tid] = lr; dl_s[buf][tid] = dr;
        if constexpr (FOLD) {
          const float l2 = lr < 0x1p100f ? lr : 0x1p100f;            // +inf (row past the sequence): probability 0
          const float lh = (float)(__bf16)l2, ll = (float)(__bf16)(l2 - lh);
          const float dh = (float)(__bf16)dr, dlo = (float)(__bf16)(dr - dh);
          bf16x8 es, ed, z;
#pragma unroll
          for (int j = 0; j < 8; ++j) { es[j] = (__bf16)0.f; ed[j] = (__bf16)0.f; z[j] = (__bf16)0.f; }
          es[0] = (__bf16)(-lh); es[1] = (__bf16)(-ll); es[2] = (__bf16)(-0x1p100f);
          ed[0] = (__bf16)(-dh); ed[1] = (__bf16)(-dlo);
          *reinterpret_cast<bf16x8*>(&ext_s[buf][tid * 16]) = es;
          *reinterpret_cast<bf16x8*>(&ext_s[buf][tid * 16 + 8]) = z;
          *reinterpret_cast<bf16x8*>(&ext_d[buf][tid * 16]) = ed;
          *reinterpret_cast<bf16x8*>(&ext_d[buf][tid * 16 + 8]) = z;
        }
      }
    };
    if (ntiles > t0) {
      qr.load(qg, p.q_stride, (int64_t)t0 * QT, lq_, tid);
      dor.load(dog, o_stride, (int64_t)t0 * QT, lq_, tid);
      load_small((int64_t)t0 * QT);
      qr.store(qs[0], tid);
      dor.store(dos[0], tid);
      store_small(0);
    }
    __syncthreads();
    for (int t = t0; t < ntiles; ++t) {
      const int64_t q0 = (int64_t)t * QT;
      const int cur = DBUF ? ((t - t0) & 1) : 0;
      const bool more = t + 1 < ntiles;
      if (DBUF && more) {
        qr.load(qg, p.q_stride, q0 + QT, lq_, tid);
        dor.load(dog, o_stride, q0 + QT, lq_, tid);
        load_small(q0 + QT);
      }
      if (wave_live) {
#pragma unroll
      for (int qb = 0; qb < QT / 32; ++qb) {
        if (QT > 32 && q0 + qb * 32 >= lq_) break;            // block-uniform
        if constexpr (WINDOW) {
          if (q0 + qb * 32 > k_wave0 + 31 + window || q0 + qb * 32 + 31 + window < k_wave0) continue;   // query block outside the band of this wave's keys (wave-uniform)
        }
        // a query block that the band edge crosses for some key of the wave (wave-uniform)
        const bool edge = WINDOW && !(q0 + qb * 32 + window >= k_wave0 + 31 && q0 + qb * 32 + 31 <= k_wave0 + window);
        f32x16 s, dp;
#pragma unroll
        for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
        if constexpr (FOLD) {
          const bf16x8 ea = *reinterpret_cast<const bf16x8*>(&ext_s[cur][(qb * 32 + r) * 16 + 8 * h]);   // A row r = query r of the block
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ea, ones_k, s, 0, 0, 0);
          if (!DROP) {
            const bf16x8 da = *reinterpret_cast<const bf16x8*>(&ext_d[cur][(qb * 32 + r) * 16 + 8 * h]);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, ones_2, dp, 0, 0, 0);
          }
        }
        mma_rows<D>(qs[cur], PITCH, qb * 32, kf, s, r, h);
        mma_rows<D>(dos[cur], PITCH, qb * 32, vf, dp, r, h);
        if constexpr (FOLD && !DROP) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            float bi = 0.f;
            if constexpr (BIAS) {
              const float* bh = rel_bias + hd * (2 * rel_m - 1) + (rel_m - 1);
              int rel = ki - ((int)q0 + qb * 32 + acc_row(i, h));
              rel = rel < 1 - rel_m ? 1 - rel_m : (rel > rel_m - 1 ? rel_m - 1 : rel);
              bi = bh[rel] * kLog2e;
            }
            if constexpr (DISENT) {
              const int qq = (int)q0 + qb * 32 + acc_row(i, h), last = (int)lq_ - 1;
              bi = disent_term(*dt, dt->c + disent_row(p, *dt, hd, qbase + (qq < last ? qq : last)),
                               dt->pt + disent_row(p, *dt, hd, kbase + kr_), qq - ki) * sl2;
            }
            float pr = fast_exp2(PRE ? s[i] + bi : s[i]);
            if constexpr (WINDOW) {
              if (edge) {                                      // a select, not a product: see attn_dq_body
                const int qq = (int)q0 + qb * 32 + acc_row(i, h), wi = (int)window;
                pr = (qq <= ki + wi && qq + wi >= ki) ? pr : 0.f;
              }
            }
            s[i] = pr;
            dp[i] = pr * dp[i];
          }
        } else {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int q4 = qb * 32 + 8 * g4 + 4 * h;       // accumulator registers 4*g4 .. 4*g4+3 = queries q4 .. q4+3
          const float4 l4 = *reinterpret_cast<const float4*>(&lse_s[cur][q4]);
          const float4 d4 = *reinterpret_cast<const float4*>(&dl_s[cur][q4]);
          const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv4[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
          for (int j = 0; j < 4; j += 2) {
            const int i = 4 * g4 + j;                        // registers i, i+1 = queries q0 + q4 + j, + 1 (even, odd)
            // query rows past the sequence carry lse = +inf in LDS, masked keys select the exponent -inf: both give
            // probability exactly 0 without a branch around the exp
            float b0 = 0.f, b1 = 0.f;                      // BIAS: bias * log2 e of queries q, q + 1 (table index rel, rel - 1)
            if constexpr (BIAS) {
              const float* bh = rel_bias + hd * (2 * rel_m - 1) + (rel_m - 1);
              const int rel = ki - ((int)q0 + q4 + j), lo = 1 - rel_m, hi = rel_m - 1;   // each index clamped on its own
              b0 = bh[rel < lo ? lo : (rel > hi ? hi : rel)] * kLog2e;
              b1 = bh[rel - 1 < lo ? lo : (rel - 1 > hi ? hi : rel - 1)] * kLog2e;
            }
            if constexpr (DISENT) {
              const int qq = (int)q0 + q4 + j, last = (int)lq_ - 1;       // each query row clamped on its own
              const float* prow = dt->pt + disent_row(p, *dt, hd, kbase + kr_);
              b0 = disent_term(*dt, dt->c + disent_row(p, *dt, hd, qbase + (qq < last ? qq : last)), prow, qq - ki) * sl2;
              b1 = disent_term(*dt, dt->c + disent_row(p, *dt, hd, qbase + (qq + 1 < last ? qq + 1 : last)), prow, qq + 1 - ki) * sl2;
            }
            float p0 = FOLD ? fast_exp2(PRE ? s[i] + b0 : s[i]) : fast_exp2(key_ok ? fmaf(s[i], sl2, PRE ? b0 - lv[j] : -lv[j]) : -INFINITY);
            float p1 = FOLD ? fast_exp2(PRE ? s[i + 1] + b1 : s[i + 1]) : fast_exp2(key_ok ? fmaf(s[i + 1], sl2, PRE ? b1 - lv[j + 1] : -lv[j + 1]) : -INFINITY);
            if constexpr (WINDOW) {
              if (edge) {
                const int qq = (int)q0 + q4 + j, wi = (int)window;
                p0 = (qq <= ki + wi && qq + wi >= ki) ? p0 : 0.f;
                p1 = (qq + 1 <= ki + wi && qq + 1 + wi >= ki) ? p1 : 0.f;
              }
            }
            float m0 = 1.f, m1 = 1.f;
            if (DROP) drop_pair_k(dk_u + ((uint32_t)(q0 >> 1) + (uint32_t)((qb * 32 + 8 * g4 + j) >> 1)) * kDropC1, k_odd, p.drop_thresh, p.keep_scale, m0, m1);
            s[i] = p0 * m0;
            s[i + 1] = p1 * m1;
            dp[i] = p0 * (dp[i] * m0 - dv4[j]);
            dp[i + 1] = p1 * (dp[i + 1] * m1 - dv4[j + 1]);
          }
        }
        }
        mma_acc<D>(dos[cur], PITCH, qb * 32, s, dv, lane);
        mma_acc<D>(qs[cur], PITCH, qb * 32, dp, dk, lane);
      }
      }
      if (DBUF) {
        if (more) {
          qr.store(qs[cur ^ 1], tid);
          dor.store(dos[cur ^ 1], tid);
          store_small(cur ^ 1);
        }
        __syncthreads();
      } else if (more) {
        __syncthreads();
        qr.load(qg, p.q_stride, q0 + QT, lq_, tid);
        dor.load(dog, o_stride, q0 + QT, lq_, tid);
        load_small(q0 + QT);
        qr.store(qs[0], tid);
        dor.store(dos[0], tid);
        store_small(0);
        __syncthreads();
      }
    }
  }
  if (key_in) {
    T* dkg = static_cast<T*>(p.dk) + (kbase + key) * p.dk_stride + hd * D;
    T* dvg = static_cast<T*>(p.dv) + (kbase + key) * p.dv_stride + hd * D;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      store_t<T>(dkg + d * 32, dk[d], p.scale, h);
      store_t<T>(dvg + d * 32, dv[d], 1.f, h);
    }
  }
}

}  // namespace gmlm
