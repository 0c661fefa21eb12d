// Attention at head dims 256 / 384 / 512 on gfx950 MFMA: the kernel plan and the loop bodies of the two wide-head families
//   gmlm_attention_wide_*      attn_wide.hip      wide::*   d = 256 / 384 / 512, padded, lq != lk, probability dropout
//   gmlm_attention_gqa_d256_*  attn_gqa_wide.hip  gqaw::*   d = 256, grouped KV heads, causal flag, padded or packed
// A family's file holds its __global__ wrappers (decode + one call of a body here), its dynamic-LDS attributes, its launch macro
// and its exports (the convention of attn_grouped.hpp, whose Params both families launch with).
// One wave cannot hold such a head (at D = 128 the dQ kernel already takes ~256 VGPRs), so the HEAD DIM is split over the
// four waves of a workgroup: all four waves work on the SAME 32 query (forward, dQ) or key (dK/dV) rows, and wave w owns
// columns [w*D/4, (w+1)*D/4) of Q, K, V, dO, O, dQ, dK and dV, i.e. 64 / 96 / 128 columns: the register picture of the
// d = 64 / 96 / 128 bodies of attn_stream.hpp, whose operand helpers (attn_common.hpp) are used unchanged on a column slice.
// Per 32-row tile of the other operand every wave forms the partial 32 x 32 score tile of its slice, the four partials go
// through LDS and every wave adds them in the same order ((w0 + w1) + w2) + w3 (exchange()), so all waves hold bit-identical
// scores: running max, sum, probabilities and the dropout mask agree with no further exchange, and each wave accumulates its
// own slice of the second product.  dP = dO V^T is exchanged the same way.
//  * 1-D grids of (tile, (sequence, head)) work items; workgroup = 32 rows, tiles of 32 rows, one LDS buffer (throughput is not
//    the aim here: beside an encoder pass of seconds this attention is milliseconds);
//  * the tiles hold the full head width: 2 x 32 x (D + pad) elements + the 16 KiB exchange area = 49.3 / 81.3 KiB (bf16) and
//    81.3 / 145.3 KiB (fp32) at D = 256 / 512, dynamic LDS above the 64 KiB default;
//  * scores take the fp32 path of the streaming bodies for both dtypes (scale, lse and the masks applied to the summed score on
//    the VALU, no folded contraction step: a partial sum has no place for it); P and dS are rounded to bf16 before the second
//    product exactly as there; delta is exact in fp32 through out_lo;
//  * no atomics: dK/dV walks the query tiles in order; a repeated call gives identical bytes.
// The template flags, each compiled out with `if constexpr` when false:
//  * DROP: the dropout hash hands out masks in pairs of accumulator registers, so the forward and dQ form P and dS in pairs (the
//    forward's row sum is rsum += e0 + e1 in every instantiation); dK/dV draws the masks of four queries first and forms P and dS
//    one element at a time, which costs its kernels 100 VGPRs less (DESIGN.md section 4 "Encoders wider than 1,024");
//  * GROUPED: query head h reads KV head h / group, group = hq / hkv a runtime value; the dK/dV workgroup owns 32 keys of one
//    (sequence, KV head), walks the query heads of its group in order and, per head, the query tiles, accumulating into the same
//    registers: no expanded K / V or dK / dV in HBM.  Also the packed layout (AttnParams::cu): a tile past its sequence returns
//    block-uniformly before the first barrier;
//  * CAUSAL: query tiles and key tiles are both 32 rows, so tile t of the keys is the diagonal tile of query tile t.  The key
//    loop of the forward and of dQ ends at the diagonal, the query loop of dK/dV starts there; tiles off the diagonal take the
//    compare-free path, the diagonal one compares key <= query per element.  Key kv0 of a tile that is computed is valid for
//    each of the 32 queries (kv0 <= 32 t <= query, kv0 < kv_len), so the running max stays finite;
//  * BAND (attn_gqa_band.hip, gqab::*; only with GROUPED): query i sees key j iff j < kv_len and 0 <= i - j < w (CAUSAL) or
//    |i - j| < w, w = `window` >= 1, an argument of the bodies that the other kernels leave at 0.  The key loop of the forward
//    and of dQ and the query loop of dK/dV cover the tiles the band of the 32 rows touches (key_range / query_range, block-
//    uniform); a tile that lies whole inside the band of every row and below kv_len keeps the compare-free path, every other
//    one applies the rule per element.  The sentence above no longer holds: with w < 32 a row can see no key in the first tile of
//    its loop, and a padded query at or past kv_len + w - 1 sees none at all.  The forward keeps such a row's running max at
//    -inf without forming -inf - -inf (the guards of attn_stream.hpp's WINDOW flag) and a row that never sees a key gets
//    output 0 and lse = -inf; both backward kernels read lse = -inf as "probability 0 everywhere", so its dQ is 0 and it adds
//    nothing to dK / dV.  A finite value is never changed by a guard: with w >= l the bytes are those of the kernels without
//    the flag.
//  * SOFTCAP (attn_gqa_softcap.hip, gqac::*; only with GROUPED, with or without BAND): the scores enter the softmax as
//    z = c tanh(score * scale / c), c = `softcap` > 0, the last argument of the bodies.  The forward replaces every score by z right
//    after exchange() and BEFORE any mask select (tanh(-inf) = -1 is finite: a mask applied first would give a masked key the
//    probability of a score of -c) and runs the rest of its loop on z with log2 e in place of scale * log2 e; lse is that of the
//    capped scores.  dQ and dK/dV recompute z the same way and multiply dS by 1 - tanh^2 before it is rounded for the second
//    product; the p.scale at their stores is the scale of dz/ds = scale (1 - tanh^2).  softcap_z() below says how tanh is formed.
#pragma once
#include <type_traits>
#include "attn_grouped.hpp"

namespace gmlm {
namespace widehead {

using grouped::Params;   // the plain family leaves `group` unread

constexpr int NW = 4, NT = NW * 64, R = 32, KT = 32;   // 4 waves on the same 32 rows; 32-row tiles of the other operand

template <typename T, int D> struct Lds {
  static constexpr int PITCH = D + Pad<T>::v;
  static constexpr int TILE = KT * PITCH * (int)sizeof(T);        // one 32-row tile, full head width
  static constexpr int XCH = NW * 16 * 64 * (int)sizeof(float);   // four partial 32 x 32 accumulator tiles
  static constexpr int SMALL = 2 * KT * (int)sizeof(float);       // dK/dV: lse and delta of the staged query rows
  static constexpr int BYTES = 2 * TILE + XCH + SMALL;
  static_assert(TILE % 16 == 0 && BYTES <= 160 * 1024, "LDS carve");
};

// the instantiations that exist: the grouped family has no dropout and one head dim, the plain one no causal mask
// (and the band only in the grouped one)
template <int D, bool DROP, bool CAUSAL, bool GROUPED, bool BAND = false, bool SOFTCAP = false> constexpr bool kSupported =
    (D == 256 || D == 384 || D == 512) && (GROUPED ? !DROP && D == 256 : !CAUSAL) && (!BAND || (GROUPED && D == 256)) &&
    (!SOFTCAP || (GROUPED && D == 256));

// SOFTCAP: z = c tanh(x), x = score * scale / c (`k` = scale / c), and fac = 1 - tanh(x)^2 = dz / d(score * scale), both from ONE
// exponential of -2|x| taken as em = expm1(-2|x|): tanh|x| = -em / (2 + em) and fac = 4 (1 + em) / (2 + em)^2.  The error is
// relative to |z| (1 - exp(-2|x|) would leave an absolute c 2^-24 on every small score); a saturated score gives em = -1:
// z = +-c and fac = 0 exactly; no finite score gives a NaN (2 + em >= 1).
__device__ __forceinline__ float softcap_z(float s, float k, float c, float& fac) {
  const float x = s * k;
  const float em = expm1f(-2.f * fabsf(x));
  const float r = __builtin_amdgcn_rcpf(2.f + em);
  fac = 4.f * (1.f + em) * r * r;
  return c * copysignf(-em * r, x);
}

// s <- ((s_w0 + s_w1) + s_w2) + s_w3, the same expression in every wave.  Two barriers: partials visible / area free again.
__device__ __forceinline__ void exchange(float* xs, f32x16& s, int w, int lane) {
#pragma unroll
  for (int i = 0; i < 16; ++i) xs[(w * 16 + i) * 64 + lane] = s[i];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i)
    s[i] = ((xs[i * 64 + lane] + xs[(16 + i) * 64 + lane]) + xs[(32 + i) * 64 + lane]) + xs[(48 + i) * 64 + lane];
  __syncthreads();
}

// key tiles [0, n) of query tile `tile`: below kv_len and, CAUSAL, up to the diagonal tile
template <bool CAUSAL>
__device__ __forceinline__ int key_tiles(int64_t kvlen, int64_t tile) {
  const int64_t n = (kvlen + KT - 1) / KT;
  return (int)(CAUSAL && tile + 1 < n ? tile + 1 : n);
}

// BAND: the band rule between a query and a key of one sequence (the caller adds key < kv_len)
template <bool CAUSAL, typename I>
__device__ __forceinline__ bool band_sees(I q, I key, I window) {
  return CAUSAL ? key <= q && q - key < window : q - key < window && key - q < window;
}

// BAND: rows [a0, a0 + 32) and [b0, b0 + 32) of the two operands see each other pair by pair (a = query tile, b = key tile)
template <bool CAUSAL>
__device__ __forceinline__ bool band_whole(int64_t q0, int64_t kv0, int64_t window) {
  return kv0 + (window - 1) >= q0 + R - 1 && (CAUSAL ? kv0 < q0 : kv0 + KT - 1 <= q0 + (window - 1));
}

// key tiles [t0, t1) of query tile `tile`; BAND: from the tile of key 32 tile - (w - 1) to the diagonal tile (CAUSAL) or the
// tile of key 32 tile + 31 + (w - 1), cut to kv_len; t0 >= t1: the rows see no key
template <bool CAUSAL, bool BAND>
__device__ __forceinline__ void key_range(int64_t kvlen, int64_t tile, int64_t window, int& t0, int& t1) {
  t0 = 0;
  t1 = key_tiles<CAUSAL>(kvlen, tile);
  if constexpr (BAND) {
    const int64_t n = (kvlen + KT - 1) / KT, lo = tile * R - (window - 1);
    const int64_t hi = CAUSAL ? tile + 1 : (tile * R + R - 1 + (window - 1)) / KT + 1;
    t0 = (int)((lo > 0 ? lo : 0) / KT);
    t1 = (int)(hi < n ? hi : n);
  }
}

// forward: workgroup = 32 query rows of one (sequence, query head), loop over the key tiles of its KV head
template <typename T, int D, bool DROP, bool CAUSAL, bool GROUPED, bool BAND = false, bool SOFTCAP = false>
__device__ __forceinline__ void fwd_body(const Params& x, const Item& it, int64_t window = 0, float softcap = 0.f) {
  static_assert(kSupported<D, DROP, CAUSAL, GROUPED, BAND, SOFTCAP>, "no kernel of either family has this combination");
  const AttnParams& p = x.a;
  constexpr int DS = D / NW, PITCH = Lds<T, D>::PITCH, DB = DS / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_wide[];
  T* ks = reinterpret_cast<T*>(smem_wide);
  T* vs = ks + KT * PITCH;
  float* xs = reinterpret_cast<float*>(smem_wide + 2 * Lds<T, D>::TILE);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t b = it.b, hd = it.hd;
  int64_t kvh = hd;
  if constexpr (GROUPED) kvh = hd / x.group;
  int64_t lq_, lk_, qbase, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, qbase, kbase, lse_base);
  if constexpr (GROUPED) {
    if (it.tile * R >= lq_) return;                                 // packed: a tile past its sequence (block-uniform)
  }
  const int64_t q_row = it.tile * R + r;
  const bool q_ok = q_row < lq_;
  const int64_t kvlen = clamp_kvlen(p, b, lk_);
  const T* kg = static_cast<const T*>(p.k) + kbase * p.k_stride + kvh * D;
  const T* vg = static_cast<const T*>(p.v) + kbase * p.v_stride + kvh * D;
  RowFrag<T, DS> qf;
  qf.load(static_cast<const T*>(p.q) + (qbase + (q_ok ? q_row : 0)) * p.q_stride + hd * D + w * DS, q_ok, h);
  f32x16 o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[d][i] = 0.f;
  float m = -INFINITY, l = 0.f;              // running max / sum in the log2 domain (scores * scale * log2 e)
  const float sl2 = SOFTCAP ? kLog2e : p.scale * kLog2e;          // SOFTCAP: the capped scores carry the scale already
  [[maybe_unused]] const float kcap = SOFTCAP ? p.scale / softcap : 0.f;
  const uint32_t dq_u = drop_base(attn_seed(p), lse_base) + (uint32_t)(q_row >> 1) * kDropC1 + (uint32_t)(2 * h) * kDropC2;
  const int q_odd = (int)(q_row & 1);
  int t0, ntiles;
  key_range<CAUSAL, BAND>(kvlen, it.tile, window, t0, ntiles);
  for (int t = t0; t < ntiles; ++t) {
    const int64_t kv0 = (int64_t)t * KT;
    stage_rows<T, D, KT, NT>(ks, kg, p.k_stride, kv0, lk_, tid);
    stage_rows<T, D, KT, NT>(vs, vg, p.v_stride, kv0, lk_, tid);
    __syncthreads();
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
    mma_rows<DS>(ks + w * DS, PITCH, 0, qf, s, r, h);
    exchange(xs, s, w, lane);
    if constexpr (SOFTCAP) {                                        // before any mask: tanh(-inf) = -1 would un-mask a key
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        float fac;
        s[i] = softcap_z(s[i], kcap, softcap, fac);
      }
    }
    float rmax = -INFINITY;
    // whole tile valid (block-uniform): no per-key compare.  (BAND is a constant: the conditional is folded where it stands, and
    // the branches of the kernels without the flag stay as they were; a bool formed first changes the causal forward's code)
    if (kv0 + KT <= kvlen && (BAND ? band_whole<CAUSAL>(it.tile * R, kv0, window) : !(CAUSAL && t == it.tile))) {
#pragma unroll
      for (int i = 0; i < 16; ++i) rmax = fmaxf(rmax, s[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int64_t key = kv0 + acc_row(i, h);
        const float v = key < kvlen && (BAND ? band_sees<CAUSAL>(q_row, key, window) : !CAUSAL || key <= q_row) ? s[i] : -INFINITY;
        s[i] = v;
        rmax = fmaxf(rmax, v);
      }
    }
    rmax = xhalf_max(rmax);
    float m_new = fmaxf(m, rmax * sl2);             // finite: key kv0 is valid for every row of the tile (BAND: -inf while the row has seen no key)
    bool keep;                                      // identical in the four waves (identical scores); m = -inf -> false
    float alpha = 1.f, m_ref;                       // m_ref: the exponent reference
    if constexpr (BAND) {
      // a row still at -inf that stays there changes nothing: -inf - -inf would be NaN and end the deferral for the wave
      keep = __all(m_new == -INFINITY || m_new - m <= kDefer);
      if (keep) m_new = m;
      else alpha = m == -INFINITY ? 0.f : fast_exp2(m - m_new);   // also when m_new = -inf
      m_ref = m_new == -INFINITY ? 0.f : m_new;                   // exp2(-inf - 0) = 0 for a row with no key yet
    } else {
      keep = __all(m_new - m <= kDefer);
      if (keep) m_new = m;
      else alpha = fast_exp2(m - m_new);
      m_ref = m_new;
    }
    float rsum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      const float e0 = fast_exp2(fmaf(s[i], sl2, -m_ref));        // masked: exp2(-inf) = 0
      const float e1 = fast_exp2(fmaf(s[i + 1], sl2, -m_ref));
      rsum += e0 + e1;                                            // the normaliser uses the un-dropped probabilities
      if constexpr (DROP) {
        float m0, m1;
        drop_pair_q(dq_u + ((uint32_t)(t * (KT / 2)) + (uint32_t)(acc_row(i, 0) >> 1)) * kDropC2, q_odd, p.drop_thresh, p.keep_scale, m0, m1);
        s[i] = e0 * m0;
        s[i + 1] = e1 * m1;
      } else {
        s[i] = e0;
        s[i + 1] = e1;
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
    mma_acc<DS>(vs + w * DS, PITCH, 0, s, o, lane);
    __syncthreads();                                              // tile consumed: the next staging may overwrite it
  }
  if (q_ok) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    T* og = static_cast<T*>(p.o_w) + (qbase + q_row) * x.dout_stride + hd * D + w * DS;
#pragma unroll
    for (int d = 0; d < DB; ++d) store_t<T>(og + d * 32, o[d], inv, h);
    if constexpr (sizeof(T) == 2) {
      if (p.o_lo_w) {
        T* olg = static_cast<T*>(p.o_lo_w) + (qbase + q_row) * x.dout_stride + hd * D + w * DS;
#pragma unroll
        for (int d = 0; d < DB; ++d) store_t_lo(olg + d * 32, o[d], inv, h);
      }
    }
    if (h == 0 && w == 0 && p.lse_w) p.lse_w[lse_base + q_row] = l > 0.f ? (m + __log2f(l)) * kLn2 : -INFINITY;
  }
}

// backward: delta[s, h, q] = sum_d dO * O (O = out + out_lo when the forward stored the residual); one wave per row of
// [seqs * lq, hn, d]; packed: seqs = 1 and lq = the packed rows, so delta is [hn, rows]
// (attn_delta_body gives a row at most 32 lanes of one 16-byte chunk each: 256 bf16 / 128 fp32 columns)
template <typename T>
__device__ __forceinline__ void delta_body(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                           int64_t rows /* seqs * lq * hn */, int d, int64_t lq, int64_t hn, float* __restrict__ delta) {
  constexpr int V = Store<T>::kVec;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  float acc = 0.f;
  if (row < rows) {
    for (int c = lane; c < d / V; c += 64) {
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
  }
  acc = wave_sum(acc);
  if (row < rows && lane == 0) {
    const int64_t hd = row % hn, bq = row / hn, q = bq % lq, b = bq / lq;
    delta[(b * hn + hd) * lq + q] = acc;
  }
}

// backward: dQ.  workgroup = 32 queries of one (sequence, query head), loop over the key tiles of its KV head.
//   S^T = K Q^T and dP^T = V dO^T as sums of four partials, P^T = exp(scale * S^T - lse[q]), dS^T = P^T * (dP^T - delta[q]),
//   dQ_w^T += K_w^T dS^T  (query on the lane)
template <typename T, int D, bool DROP, bool CAUSAL, bool GROUPED, bool BAND = false, bool SOFTCAP = false>
__device__ __forceinline__ void dq_body(const Params& x, const Item& it, int64_t window = 0, float softcap = 0.f) {
  static_assert(kSupported<D, DROP, CAUSAL, GROUPED, BAND, SOFTCAP>, "no kernel of either family has this combination");
  const AttnParams& p = x.a;
  constexpr int DS = D / NW, PITCH = Lds<T, D>::PITCH, DB = DS / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_wide[];
  T* ks = reinterpret_cast<T*>(smem_wide);
  T* vs = ks + KT * PITCH;
  float* xs = reinterpret_cast<float*>(smem_wide + 2 * Lds<T, D>::TILE);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t b = it.b, hd = it.hd;
  int64_t kvh = hd;
  if constexpr (GROUPED) kvh = hd / x.group;
  int64_t lq_, lk_, qbase, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, qbase, kbase, lse_base);
  if constexpr (GROUPED) {
    if (it.tile * R >= lq_) return;                                 // packed: a tile past its sequence (block-uniform)
  }
  const int64_t q_row = it.tile * R + r;
  const bool q_ok = q_row < lq_;
  const int64_t kvlen = clamp_kvlen(p, b, lk_);
  const int64_t qr = q_ok ? q_row : 0;
  const T* kg = static_cast<const T*>(p.k) + kbase * p.k_stride + kvh * D;
  const T* vg = static_cast<const T*>(p.v) + kbase * p.v_stride + kvh * D;
  RowFrag<T, DS> qf, dof;
  qf.load(static_cast<const T*>(p.q) + (qbase + qr) * p.q_stride + hd * D + w * DS, q_ok, h);
  dof.load(static_cast<const T*>(p.dout) + (qbase + qr) * x.dout_stride + hd * D + w * DS, q_ok, h);
  const float sl2 = SOFTCAP ? kLog2e : p.scale * kLog2e;          // SOFTCAP: the capped scores carry the scale already
  [[maybe_unused]] const float kcap = SOFTCAP ? p.scale / softcap : 0.f;
  float lse2 = q_ok ? p.lse[lse_base + q_row] * kLog2e : INFINITY;   // a row past the sequence: probability 0 everywhere
  if constexpr (BAND) {
    if (lse2 == -INFINITY) lse2 = INFINITY;                           // and a row that saw no key: never exp2(+inf)
  }
  const float dl = q_ok ? p.delta[lse_base + q_row] : 0.f;
  const int kvl = (int)(kvlen < (1 << 30) ? kvlen : (1 << 30));
  const int qi = (int)(q_row < (1 << 30) ? q_row : (1 << 30));
  const uint32_t dq_u = drop_base(attn_seed(p), lse_base) + (uint32_t)(q_row >> 1) * kDropC1 + (uint32_t)(2 * h) * kDropC2;
  const int q_odd = (int)(q_row & 1);
  f32x16 dq[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[d][i] = 0.f;
  const int wi = (int)window;
  int t0, ntiles;
  key_range<CAUSAL, BAND>(kvlen, it.tile, window, t0, ntiles);
  for (int t = t0; t < ntiles; ++t) {
    const int64_t kv0 = (int64_t)t * KT;
    stage_rows<T, D, KT, NT>(ks, kg, p.k_stride, kv0, lk_, tid);
    stage_rows<T, D, KT, NT>(vs, vg, p.v_stride, kv0, lk_, tid);
    __syncthreads();
    f32x16 s, dp;
#pragma unroll
    for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
    mma_rows<DS>(ks + w * DS, PITCH, 0, qf, s, r, h);
    exchange(xs, s, w, lane);
    mma_rows<DS>(vs + w * DS, PITCH, 0, dof, dp, r, h);
    exchange(xs, dp, w, lane);
    bool full = kv0 + KT <= kvlen && !(CAUSAL && t == it.tile);          // block-uniform
    if constexpr (BAND) full = kv0 + KT <= kvlen && band_whole<CAUSAL>(it.tile * R, kv0, window);
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      const int key = (int)kv0 + acc_row(i, h);                   // even; registers i, i+1 = keys key, key+1
      [[maybe_unused]] float f0, f1;                              // SOFTCAP: 1 - tanh^2 of the pair
      if constexpr (SOFTCAP) {
        s[i] = softcap_z(s[i], kcap, softcap, f0);
        s[i + 1] = softcap_z(s[i + 1], kcap, softcap, f1);
      }
      float a0 = fmaf(s[i], sl2, -lse2), a1 = fmaf(s[i + 1], sl2, -lse2);
      if (!full) {                                                // a masked pair has P = exp2(-inf) = 0 whatever its score
        if constexpr (BAND) {
          a0 = key < kvl && band_sees<CAUSAL>(qi, key, wi) ? a0 : -INFINITY;
          a1 = key + 1 < kvl && band_sees<CAUSAL>(qi, key + 1, wi) ? a1 : -INFINITY;
        } else {
          a0 = key < kvl && (!CAUSAL || key <= qi) ? a0 : -INFINITY;
          a1 = key + 1 < kvl && (!CAUSAL || key + 1 <= qi) ? a1 : -INFINITY;
        }
      }
      const float p0 = fast_exp2(a0), p1 = fast_exp2(a1);
      float m0 = 1.f, m1 = 1.f;
      if constexpr (DROP) drop_pair_q(dq_u + ((uint32_t)(t * (KT / 2)) + (uint32_t)(acc_row(i, 0) >> 1)) * kDropC2, q_odd, p.drop_thresh, p.keep_scale, m0, m1);
      s[i] = p0 * (dp[i] * m0 - dl);
      s[i + 1] = p1 * (dp[i + 1] * m1 - dl);
      if constexpr (SOFTCAP) {
        s[i] *= f0;
        s[i + 1] *= f1;
      }
    }
    mma_acc<DS>(ks + w * DS, PITCH, 0, s, dq, lane);
    __syncthreads();
  }
  if (q_ok) {
    T* og = static_cast<T*>(p.dq) + (qbase + q_row) * p.dq_stride + hd * D + w * DS;
#pragma unroll
    for (int d = 0; d < DB; ++d) store_t<T>(og + d * 32, dq[d], p.scale, h);
  }
}

// BAND: query tiles [t0, t1) of key tile `kt` in a sequence of l rows: from the diagonal tile (CAUSAL) or the tile of query
// 32 kt - (w - 1) to the tile of query 32 kt + 31 + (w - 1)
template <bool CAUSAL>
__device__ __forceinline__ void query_range(int64_t l, int64_t kt, int64_t window, int& t0, int& t1) {
  const int64_t n = (l + KT - 1) / KT, lo = kt * R - (window - 1), hi = (kt * R + R - 1 + (window - 1)) / KT + 1;
  t0 = (int)(CAUSAL ? kt : (lo > 0 ? lo : 0) / KT);
  t1 = (int)(hi < n ? hi : n);
}

// backward: dK, dV.  workgroup = 32 keys of one (sequence, KV head): key rows lk_ from kbase, query rows lq_ from qbase (the
// plain family has lq != lk).  GROUPED: for each query head of the group, in order; per head the query tiles of 32 in order
// (CAUSAL: from the diagonal tile on), all into the same registers (deterministic).
//   S = Q K^T and dP = dO V^T as sums of four partials, P = exp(scale * S - lse[q]), dV_w^T += dO_w^T P,
//   dS = P * (dP - delta[q]), dK_w^T += Q_w^T dS  (key on the lane, the query in the accumulator registers)
// The work item is decode()'s for the plain family and causal_key_tile()'s for the grouped one.
template <typename T, int D, bool DROP, bool CAUSAL, bool GROUPED, bool BAND = false, bool SOFTCAP = false>
__device__ __forceinline__ void dkv_body(const Params& x, const std::conditional_t<GROUPED, CausalKeyTile, Item>& it, int64_t window = 0,
                                         float softcap = 0.f) {
  static_assert(kSupported<D, DROP, CAUSAL, GROUPED, BAND, SOFTCAP>, "no kernel of either family has this combination");
  const AttnParams& p = x.a;
  constexpr int DS = D / NW, PITCH = Lds<T, D>::PITCH, DB = DS / 32, QT = KT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_wide[];
  T* qs = reinterpret_cast<T*>(smem_wide);
  T* dos = qs + QT * PITCH;
  float* xs = reinterpret_cast<float*>(smem_wide + 2 * Lds<T, D>::TILE);
  float* lse_s = xs + NW * 16 * 64;
  float* dl_s = lse_s + QT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t b = it.b;
  int64_t tile, kvh, lq_, lk_, qbase, kbase, lse_base;
  if constexpr (GROUPED) {
    tile = it.kt; kvh = it.kvh; lq_ = lk_ = it.l; qbase = kbase = it.base; lse_base = 0;
    if (tile * R >= lk_) return;                                    // packed: a tile past its sequence (block-uniform)
  } else {
    tile = it.tile; kvh = it.hd;
    seq_view(p, b, kvh, lq_, lk_, qbase, kbase, lse_base);
  }
  const int64_t kvlen = clamp_kvlen(p, b, lk_);
  const int64_t key = tile * R + r;
  const bool key_in = key < lk_;           // row exists in memory
  const bool key_ok = key < kvlen;          // takes part in the softmax
  const int64_t kr_ = key_in ? key : 0;
  const int ki = (int)(key < (1 << 30) ? key : (1 << 30));
  RowFrag<T, DS> kf, vf;
  kf.load(static_cast<const T*>(p.k) + (kbase + kr_) * p.k_stride + kvh * D + w * DS, key_in, h);
  vf.load(static_cast<const T*>(p.v) + (kbase + kr_) * p.v_stride + kvh * D + w * DS, key_in, h);
  const T* qg = static_cast<const T*>(p.q) + qbase * p.q_stride + kvh * D;   // Q, dO, lse, delta of the one head; grouped: per head below
  const T* dog = static_cast<const T*>(p.dout) + qbase * x.dout_stride + kvh * D;
  const float* lse_g = p.lse + lse_base;
  const float* dl_g = p.delta + lse_base;
  const float sl2 = SOFTCAP ? kLog2e : p.scale * kLog2e;          // SOFTCAP: the capped scores carry the scale already
  [[maybe_unused]] const float kcap = SOFTCAP ? p.scale / softcap : 0.f;
  const uint32_t dk_u = drop_base(attn_seed(p), lse_base) + (uint32_t)(key >> 1) * kDropC2 + (uint32_t)(2 * h) * kDropC1;
  const int k_odd = (int)(key & 1);
  f32x16 dk[DB], dv[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk[d][i] = 0.f; dv[d][i] = 0.f; }
  if (tile * R < kvlen) {                  // a whole workgroup past kv_len has nothing to accumulate (block-uniform)
    int t0 = CAUSAL ? (int)tile : 0, ntiles = (int)((lq_ + QT - 1) / QT);
    if constexpr (BAND) query_range<CAUSAL>(lq_, tile, window, t0, ntiles);
    const int wi = (int)window;
    int heads = 1;
    if constexpr (GROUPED) heads = x.group;
    for (int g = 0; g < heads; ++g) {
      if constexpr (GROUPED) {
        const int64_t hd = kvh * x.group + g;
        lse_base = p.cu ? hd * p.lq + qbase : (b * p.h + hd) * p.lq;   // [hq, T] or [b, hq, l], as seq_view()
        qg = static_cast<const T*>(p.q) + qbase * p.q_stride + hd * D;
        dog = static_cast<const T*>(p.dout) + qbase * x.dout_stride + hd * D;
        lse_g = p.lse + lse_base;
        dl_g = p.delta + lse_base;
      }
      for (int t = t0; t < ntiles; ++t) {
        const int64_t q0 = (int64_t)t * QT;
        stage_rows<T, D, QT, NT>(qs, qg, p.q_stride, q0, lq_, tid);
        stage_rows<T, D, QT, NT>(dos, dog, x.dout_stride, q0, lq_, tid);
        if (tid < QT) {
          const bool ok = q0 + tid < lq_;
          float lv = ok ? lse_g[q0 + tid] * kLog2e : INFINITY;     // +inf: probability 0 for a row past the sequence
          if constexpr (BAND) {
            if (lv == -INFINITY) lv = INFINITY;                     // and for a row that saw no key: never exp2(+inf)
          }
          lse_s[tid] = lv;
          dl_s[tid] = ok ? dl_g[q0 + tid] : 0.f;
        }
        __syncthreads();
        f32x16 s, dp;
#pragma unroll
        for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
        mma_rows<DS>(qs + w * DS, PITCH, 0, kf, s, r, h);
        exchange(xs, s, w, lane);
        mma_rows<DS>(dos + w * DS, PITCH, 0, vf, dp, r, h);
        exchange(xs, dp, w, lane);
        const bool diag = CAUSAL && t == t0;                        // block-uniform
        bool inside = false;                                        // BAND: every pair of the tile is in the band (block-uniform)
        if constexpr (BAND) inside = band_whole<CAUSAL>(q0, tile * R, window);
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int q4 = 8 * g4 + 4 * h;                 // accumulator registers 4*g4 .. 4*g4+3 = queries q4 .. q4+3
          const float4 l4 = *reinterpret_cast<const float4*>(&lse_s[q4]);
          const float4 d4 = *reinterpret_cast<const float4*>(&dl_s[q4]);
          const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv4[4] = {d4.x, d4.y, d4.z, d4.w};
          float mk[4] = {1.f, 1.f, 1.f, 1.f};           // the dropout hash hands out the masks in pairs: queries q0 + q4 + j, + 1
          if constexpr (DROP) {
#pragma unroll
            for (int j = 0; j < 4; j += 2)
              drop_pair_k(dk_u + ((uint32_t)(q0 >> 1) + (uint32_t)((8 * g4 + j) >> 1)) * kDropC1, k_odd, p.drop_thresh, p.keep_scale, mk[j], mk[j + 1]);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {                  // one element at a time: formed in pairs, P and dS cost ~100 VGPRs
            const int i = 4 * g4 + j;
            bool on = key_ok && (!diag || (int)q0 + q4 + j >= ki);               // P = exp2(-inf) = 0 above the diagonal
            if constexpr (BAND) on = key_ok && (inside || band_sees<CAUSAL>((int)q0 + q4 + j, ki, wi));
            [[maybe_unused]] float fac;                  // SOFTCAP: 1 - tanh^2
            if constexpr (SOFTCAP) s[i] = softcap_z(s[i], kcap, softcap, fac);
            const float pr = fast_exp2(on ? fmaf(s[i], sl2, -lv[j]) : -INFINITY);
            s[i] = pr * mk[j];
            dp[i] = pr * (dp[i] * mk[j] - dv4[j]);
            if constexpr (SOFTCAP) dp[i] *= fac;
          }
        }
        mma_acc<DS>(dos + w * DS, PITCH, 0, s, dv, lane);
        mma_acc<DS>(qs + w * DS, PITCH, 0, dp, dk, lane);
        __syncthreads();                                            // tile consumed, also across the heads of the group
      }
    }
  }
  if (key_in) {
    T* dkg = static_cast<T*>(p.dk) + (kbase + key) * p.dk_stride + kvh * D + w * DS;
    T* dvg = static_cast<T*>(p.dv) + (kbase + key) * p.dv_stride + kvh * D + w * DS;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      store_t<T>(dkg + d * 32, dk[d], p.scale, h);
      store_t<T>(dvg + d * 32, dv[d], 1.f, h);
    }
  }
}

}  // namespace widehead
}  // namespace gmlm
