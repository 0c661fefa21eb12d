// Attention at head dims 256 / 384 / 512, forward + backward, gfx950 MFMA (gmlm_attention_wide_*).
// Shape: padded [b, l, h*D] with an optional per-sequence key length and in-kernel probability dropout: the CrossAttention
// (8 heads) of a text encoder 2,048 to 4,096 wide (Qwen3-Embedding-4B: 8 x 320 zero-padded to 384; -8B: 8 x 512).
// One wave cannot hold such a head (at D = 128 the dQ kernel already takes ~256 VGPRs), so the HEAD DIM is split over the
// four waves of a workgroup: all four waves work on the SAME 32 query (forward, dQ) or key (dK/dV) rows, and wave w owns
// columns [w*D/4, (w+1)*D/4) of Q, K, V, dO, O, dQ, dK and dV, i.e. 64 / 96 / 128 columns: the register picture of the
// d = 64 / 96 / 128 bodies of attn_stream.hpp, whose operand helpers (attn_common.hpp) are used unchanged on a column slice.
// Per 32-row tile of the other operand every wave forms the partial 32 x 32 score tile of its slice, the four partials go
// through LDS and every wave adds them in the same order ((w0 + w1) + w2) + w3 (exchange()), so all waves hold bit-identical
// scores: running max, sum, probabilities and the dropout mask agree with no further exchange, and each wave accumulates its
// own slice of the second product.  dP = dO V^T is exchanged the same way.
//  * 1-D grids of (tile, (batch, head)) work items; workgroup = 32 rows, tiles of 32 rows, one LDS buffer (throughput is not
//    the aim here: beside an encoder pass of seconds this attention is milliseconds);
//  * the tiles hold the full head width: 2 x 32 x (D + pad) elements + the 16 KiB exchange area = 81.3 KiB (bf16) and
//    145.3 KiB (fp32) at D = 512, dynamic LDS above the 64 KiB default;
//  * scores take the fp32 path of the streaming bodies for both dtypes (scale, lse and the key mask applied to the summed
//    score on the VALU, no folded contraction step: a partial sum has no place for it); P and dS are rounded to bf16 before
//    the second product exactly as there; delta is exact in fp32 through out_lo;
//  * no atomics: dK/dV walks the query tiles in order; a repeated call gives identical bytes.
// The argument checks and the AttnParams filling shared with the other attention entry points are in attn_host.hpp.
#include "attn_host.hpp"
#include "../../include/gmlm_hip_wide.h"

namespace gmlm {
namespace wide {

constexpr int NW = 4, NT = NW * 64, R = 32, KT = 32;   // 4 waves on the same 32 rows; 32-row tiles of the other operand

struct Params {
  AttnParams a;            // lse / delta are [b, h, lq]
  int64_t dout_stride;     // row stride of dO / O (= h * D)
};

template <typename T, int D> struct Lds {
  static constexpr int PITCH = D + Pad<T>::v;
  static constexpr int TILE = KT * PITCH * (int)sizeof(T);        // one 32-row tile, full head width
  static constexpr int XCH = NW * 16 * 64 * (int)sizeof(float);   // four partial 32 x 32 accumulator tiles
  static constexpr int SMALL = 2 * KT * (int)sizeof(float);       // dK/dV: lse and delta of the staged query rows
  static constexpr int BYTES = 2 * TILE + XCH + SMALL;
  static_assert(BYTES <= 160 * 1024, "LDS of one workgroup exceeds a CU");
};

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

// forward: workgroup = 32 query rows of one (batch, head), loop over key tiles
template <typename T, int D, bool DROP>
__global__ __launch_bounds__(NT) void fwd_kernel(Params x) {
  const AttnParams& p = x.a;
  constexpr int DS = D / NW, PITCH = Lds<T, D>::PITCH, DB = DS / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_wide[];
  T* ks = reinterpret_cast<T*>(smem_wide);
  T* vs = ks + KT * PITCH;
  float* xs = reinterpret_cast<float*>(smem_wide + 2 * Lds<T, D>::TILE);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const Item it = decode(p);
  const int64_t b = it.b, hd = it.hd;
  int64_t lq_, lk_, qbase, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, qbase, kbase, lse_base);
  const int64_t q_row = it.tile * R + r;
  const bool q_ok = q_row < lq_;
  const int64_t kvlen = clamp_kvlen(p, b, lk_);
  const T* kg = static_cast<const T*>(p.k) + kbase * p.k_stride + hd * D;
  const T* vg = static_cast<const T*>(p.v) + kbase * p.v_stride + hd * D;
  RowFrag<T, DS> qf;
  qf.load(static_cast<const T*>(p.q) + (qbase + (q_ok ? q_row : 0)) * p.q_stride + hd * D + w * DS, q_ok, h);
  f32x16 o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[d][i] = 0.f;
  float m = -INFINITY, l = 0.f;              // running max / sum in the log2 domain (scores * scale * log2 e)
  const float sl2 = p.scale * kLog2e;
  const uint32_t dq_u = drop_base(attn_seed(p), lse_base) + (uint32_t)(q_row >> 1) * kDropC1 + (uint32_t)(2 * h) * kDropC2;
  const int q_odd = (int)(q_row & 1);
  const int ntiles = (int)((kvlen + KT - 1) / KT);
  for (int t = 0; t < ntiles; ++t) {
    const int64_t kv0 = (int64_t)t * KT;
    stage_rows<T, D, KT, NT>(ks, kg, p.k_stride, kv0, lk_, tid);
    stage_rows<T, D, KT, NT>(vs, vg, p.v_stride, kv0, lk_, tid);
    __syncthreads();
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
    mma_rows<DS>(ks + w * DS, PITCH, 0, qf, s, r, h);
    exchange(xs, s, w, lane);
    float rmax = -INFINITY;
    if (kv0 + KT <= kvlen) {                                      // whole tile valid (block-uniform): no per-key compare
#pragma unroll
      for (int i = 0; i < 16; ++i) rmax = fmaxf(rmax, s[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int64_t key = kv0 + acc_row(i, h);
        const float v = key < kvlen ? s[i] : -INFINITY;
        s[i] = v;
        rmax = fmaxf(rmax, v);
      }
    }
    rmax = xhalf_max(rmax);
    float m_new = fmaxf(m, rmax * sl2);             // finite: key kv0 is always valid
    const bool keep = __all(m_new - m <= kDefer);   // identical in the four waves (identical scores); m = -inf -> false
    float alpha = 1.f;
    if (keep) m_new = m;
    else alpha = fast_exp2(m - m_new);
    float rsum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      const float e0 = fast_exp2(fmaf(s[i], sl2, -m_new));        // masked: exp2(-inf) = 0
      const float e1 = fast_exp2(fmaf(s[i + 1], sl2, -m_new));
      rsum += e0 + e1;                                            // the normaliser uses the un-dropped probabilities
      if (DROP) {
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

// backward: delta[b, h, q] = sum_d dO * O (O = out + out_lo when the forward stored the residual); one wave per (b, q, h) row
// (attn_delta_body gives a row at most 32 lanes of one 16-byte chunk each: 256 bf16 / 128 fp32 columns)
template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                    int64_t rows /* b * lq * h */, int d, int64_t lq, int64_t hn, float* __restrict__ delta) {
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

// backward: dQ.  workgroup = 32 queries of one (batch, head), loop over key tiles.
//   S^T = K Q^T and dP^T = V dO^T as sums of four partials, P^T = exp(scale * S^T - lse[q]), dS^T = P^T * (dP^T - delta[q]),
//   dQ_w^T += K_w^T dS^T  (query on the lane)
template <typename T, int D, bool DROP>
__global__ __launch_bounds__(NT) void dq_kernel(Params x) {
  const AttnParams& p = x.a;
  constexpr int DS = D / NW, PITCH = Lds<T, D>::PITCH, DB = DS / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_wide[];
  T* ks = reinterpret_cast<T*>(smem_wide);
  T* vs = ks + KT * PITCH;
  float* xs = reinterpret_cast<float*>(smem_wide + 2 * Lds<T, D>::TILE);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const Item it = decode(p);
  const int64_t b = it.b, hd = it.hd;
  int64_t lq_, lk_, qbase, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, qbase, kbase, lse_base);
  const int64_t q_row = it.tile * R + r;
  const bool q_ok = q_row < lq_;
  const int64_t kvlen = clamp_kvlen(p, b, lk_);
  const int64_t qr = q_ok ? q_row : 0;
  const T* kg = static_cast<const T*>(p.k) + kbase * p.k_stride + hd * D;
  const T* vg = static_cast<const T*>(p.v) + kbase * p.v_stride + hd * D;
  RowFrag<T, DS> qf, dof;
  qf.load(static_cast<const T*>(p.q) + (qbase + qr) * p.q_stride + hd * D + w * DS, q_ok, h);
  dof.load(static_cast<const T*>(p.dout) + (qbase + qr) * x.dout_stride + hd * D + w * DS, q_ok, h);
  const float sl2 = p.scale * kLog2e;
  const float lse2 = q_ok ? p.lse[lse_base + q_row] * kLog2e : INFINITY;   // a row past the sequence: probability 0 everywhere
  const float dl = q_ok ? p.delta[lse_base + q_row] : 0.f;
  const int kvl = (int)(kvlen < (1 << 30) ? kvlen : (1 << 30));
  const uint32_t dq_u = drop_base(attn_seed(p), lse_base) + (uint32_t)(q_row >> 1) * kDropC1 + (uint32_t)(2 * h) * kDropC2;
  const int q_odd = (int)(q_row & 1);
  f32x16 dq[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[d][i] = 0.f;
  const int ntiles = (int)((kvlen + KT - 1) / KT);
  for (int t = 0; t < ntiles; ++t) {
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
    const bool full = kv0 + KT <= kvlen;                          // block-uniform
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      const int key = (int)kv0 + acc_row(i, h);                   // even; registers i, i+1 = keys key, key+1
      float a0 = fmaf(s[i], sl2, -lse2), a1 = fmaf(s[i + 1], sl2, -lse2);
      if (!full) { a0 = key < kvl ? a0 : -INFINITY; a1 = key + 1 < kvl ? a1 : -INFINITY; }
      const float p0 = fast_exp2(a0), p1 = fast_exp2(a1);
      float m0 = 1.f, m1 = 1.f;
      if (DROP) drop_pair_q(dq_u + ((uint32_t)(t * (KT / 2)) + (uint32_t)(acc_row(i, 0) >> 1)) * kDropC2, q_odd, p.drop_thresh, p.keep_scale, m0, m1);
      s[i] = p0 * (dp[i] * m0 - dl);
      s[i + 1] = p1 * (dp[i + 1] * m1 - dl);
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

// backward: dK, dV.  workgroup = 32 keys of one (batch, head), loop over query tiles of 32 in order (deterministic).
//   S = Q K^T and dP = dO V^T as sums of four partials, P = exp(scale * S - lse[q]), dV_w^T += dO_w^T P,
//   dS = P * (dP - delta[q]), dK_w^T += Q_w^T dS  (key on the lane, the query in the accumulator registers)
template <typename T, int D, bool DROP>
__global__ __launch_bounds__(NT) void dkv_kernel(Params x) {
  const AttnParams& p = x.a;
  constexpr int DS = D / NW, PITCH = Lds<T, D>::PITCH, DB = DS / 32, QT = KT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_wide[];
  T* qs = reinterpret_cast<T*>(smem_wide);
  T* dos = qs + QT * PITCH;
  float* xs = reinterpret_cast<float*>(smem_wide + 2 * Lds<T, D>::TILE);
  float* lse_s = xs + NW * 16 * 64;
  float* dl_s = lse_s + QT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const Item it = decode(p);
  const int64_t b = it.b, hd = it.hd;
  int64_t lq_, lk_, qbase, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, qbase, kbase, lse_base);
  const int64_t kvlen = clamp_kvlen(p, b, lk_);
  const int64_t key = it.tile * R + r;
  const bool key_in = key < lk_;           // row exists in memory
  const bool key_ok = key < kvlen;          // takes part in the softmax
  const int64_t kr_ = key_in ? key : 0;
  RowFrag<T, DS> kf, vf;
  kf.load(static_cast<const T*>(p.k) + (kbase + kr_) * p.k_stride + hd * D + w * DS, key_in, h);
  vf.load(static_cast<const T*>(p.v) + (kbase + kr_) * p.v_stride + hd * D + w * DS, key_in, h);
  const T* qg = static_cast<const T*>(p.q) + qbase * p.q_stride + hd * D;
  const T* dog = static_cast<const T*>(p.dout) + qbase * x.dout_stride + hd * D;
  const float* lse_g = p.lse + lse_base;
  const float* dl_g = p.delta + lse_base;
  const float sl2 = p.scale * kLog2e;
  const uint32_t dk_u = drop_base(attn_seed(p), lse_base) + (uint32_t)(key >> 1) * kDropC2 + (uint32_t)(2 * h) * kDropC1;
  const int k_odd = (int)(key & 1);
  f32x16 dk[DB], dv[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk[d][i] = 0.f; dv[d][i] = 0.f; }
  if (it.tile * R < kvlen) {               // a whole workgroup past kv_len has nothing to accumulate (block-uniform)
    const int ntiles = (int)((lq_ + QT - 1) / QT);
    for (int t = 0; t < ntiles; ++t) {
      const int64_t q0 = (int64_t)t * QT;
      stage_rows<T, D, QT, NT>(qs, qg, p.q_stride, q0, lq_, tid);
      stage_rows<T, D, QT, NT>(dos, dog, x.dout_stride, q0, lq_, tid);
      if (tid < QT) {
        const bool ok = q0 + tid < lq_;
        lse_s[tid] = ok ? lse_g[q0 + tid] * kLog2e : INFINITY;   // +inf: probability 0 for a row past the sequence
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
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int q4 = 8 * g4 + 4 * h;                 // accumulator registers 4*g4 .. 4*g4+3 = queries q4 .. q4+3
        const float4 l4 = *reinterpret_cast<const float4*>(&lse_s[q4]);
        const float4 d4 = *reinterpret_cast<const float4*>(&dl_s[q4]);
        const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv4[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
          const int i = 4 * g4 + j;                    // registers i, i+1 = queries q0 + q4 + j, + 1 (even, odd)
          const float p0 = fast_exp2(key_ok ? fmaf(s[i], sl2, -lv[j]) : -INFINITY);
          const float p1 = fast_exp2(key_ok ? fmaf(s[i + 1], sl2, -lv[j + 1]) : -INFINITY);
          float m0 = 1.f, m1 = 1.f;
          if (DROP) drop_pair_k(dk_u + ((uint32_t)(q0 >> 1) + (uint32_t)((8 * g4 + j) >> 1)) * kDropC1, k_odd, p.drop_thresh, p.keep_scale, m0, m1);
          s[i] = p0 * m0;
          s[i + 1] = p1 * m1;
          dp[i] = p0 * (dp[i] * m0 - dv4[j]);
          dp[i + 1] = p1 * (dp[i + 1] * m1 - dv4[j + 1]);
        }
      }
      mma_acc<DS>(dos + w * DS, PITCH, 0, s, dv, lane);
      mma_acc<DS>(qs + w * DS, PITCH, 0, dp, dk, lane);
      __syncthreads();
    }
  }
  if (key_in) {
    T* dkg = static_cast<T*>(p.dk) + (kbase + key) * p.dk_stride + hd * D + w * DS;
    T* dvg = static_cast<T*>(p.dv) + (kbase + key) * p.dv_stride + hd * D + w * DS;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      store_t<T>(dkg + d * 32, dk[d], p.scale, h);
      store_t<T>(dvg + d * 32, dv[d], 1.f, h);
    }
  }
}

// the checks of attn_host.hpp up to the empty-problem return, with this family's head dims and work-item bound; fills the
// launch parameters
static int setup(const char* who, Params& x, const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                 int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                 uint64_t seed, const uint64_t* seed_dev, const void* out_lo, int dtype) {
  int rc = attn_check_shape(who, b >= 0 && h > 0 && lq >= 0 && lk >= 0, d == 256 || d == 384 || d == 512, d,
                            "this entry point takes 256, 384 and 512", dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  if ((rc = attn_check_rates(who, dropout_p, nullptr, scale)) != GMLM_OK) return rc;
  const int64_t rows = lq > lk ? lq : lk;
  GMLM_REQUIRE(b < ((int64_t)1 << 31) && h < ((int64_t)1 << 31) && rows < ((int64_t)1 << 31) &&
                   (double)cdiv(rows, R) * (double)b * (double)h < 2147483648.0 &&
                   (double)lq * (double)b * (double)h < 4.0 * 2147483648.0,      // the delta launch: one wave per (b, q, h) row
               "%s: too many work items", who);
  x = Params{};
  attn_fill(x.a, q, k, v, kv_len, b, h, lq, lk, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev);
  x.dout_stride = h * d;
  return GMLM_OK;
}

// > 64 KiB of dynamic LDS needs the attribute once per instantiation and device
template <typename T, int D> static int set_attrs() {
  constexpr int kLds = Lds<T, D>::BYTES;
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fwd_kernel<T, D, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fwd_kernel<T, D, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dq_kernel<T, D, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dq_kernel<T, D, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dkv_kernel<T, D, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dkv_kernel<T, D, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  return GMLM_OK;
}
static int prepare() {
  static PerDeviceOnce once;
  return once([]() -> int {
    int rc;
    if ((rc = set_attrs<bf16_t, 256>()) != GMLM_OK) return rc;
    if ((rc = set_attrs<bf16_t, 384>()) != GMLM_OK) return rc;
    if ((rc = set_attrs<bf16_t, 512>()) != GMLM_OK) return rc;
    if ((rc = set_attrs<float, 256>()) != GMLM_OK) return rc;
    if ((rc = set_attrs<float, 384>()) != GMLM_OK) return rc;
    return set_attrs<float, 512>();
  });
}

}  // namespace wide
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::wide;

#define GMLM_WIDE_K(KERNEL, T, DD, DR) KERNEL<T, DD, DR><<<grid, NT, Lds<T, DD>::BYTES, st>>>(x)
#define GMLM_WIDE_D(KERNEL, T, DR)                         \
  do {                                                     \
    if (d == 256) GMLM_WIDE_K(KERNEL, T, 256, DR);         \
    else if (d == 384) GMLM_WIDE_K(KERNEL, T, 384, DR);    \
    else GMLM_WIDE_K(KERNEL, T, 512, DR);                  \
  } while (0)
#define GMLM_WIDE_LAUNCH(KERNEL)                           \
  do {                                                     \
    const bool dr_ = x.a.drop_thresh != 0;                 \
    if (dtype == GMLM_BF16) {                              \
      if (dr_) GMLM_WIDE_D(KERNEL, bf16_t, true);          \
      else GMLM_WIDE_D(KERNEL, bf16_t, false);             \
    } else {                                               \
      if (dr_) GMLM_WIDE_D(KERNEL, float, true);           \
      else GMLM_WIDE_D(KERNEL, float, false);              \
    }                                                      \
  } while (0)

extern "C" int gmlm_attention_wide_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                                       int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                       float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* out,
                                       void* out_lo, float* lse, int dtype, gmlm_stream_t stream) {
  static const char* who = "attention_wide_fwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, h * d, h * d, dtype)) != GMLM_OK) return rc;
  if ((rc = prepare()) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(cdiv(lq, R) * b * h));
  GMLM_WIDE_LAUNCH(fwd_kernel);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_wide_bwd_workspace_bytes(int64_t b, int64_t h, int64_t lq) {
  return attn_delta_bytes(b, h, lq);
}

extern "C" int gmlm_attention_wide_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                       const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t h,
                                       int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                       float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* dq, void* dk,
                                       void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                       void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "attention_wide_bwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || (lq == 0 && lk == 0)) return GMLM_OK;
  GMLM_REQUIRE(lq > 0 && lk > 0, "%s: empty query or key set with a non-empty counterpart is not supported", who);
  AttnParams& p = x.a;
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, p, h * d, h * d, dtype, workspace_bytes, attn_delta_bytes(b, h, lq))) != GMLM_OK) return rc;
  if ((rc = prepare()) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t rows = b * lq * h;
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, rows, 64, st, (int)d, lq, h);     // one wave per row
  GMLM_LAUNCH_CHECK();
  {
    const dim3 grid((unsigned)(cdiv(lq, R) * b * h));
    GMLM_WIDE_LAUNCH(dq_kernel);
    GMLM_LAUNCH_CHECK();
  }
  {
    const dim3 grid((unsigned)(cdiv(lk, R) * b * h));
    GMLM_WIDE_LAUNCH(dkv_kernel);
    GMLM_LAUNCH_CHECK();
  }
  return GMLM_OK;
}
