// Self-attention with grouped KV heads at head dim 256, causal or bidirectional, padded or packed, forward + backward, gfx950
// MFMA (gmlm_attention_gqa_d256_*; C ABI in include/gmlm_hip_gqa_wide.h), all in namespace gmlm::gqaw: the attention of a Gemma3
// text encoder (3 / 1, 4 / 1, 8 / 4 or 16 / 8 query / KV heads of 256).
// One wave cannot hold such a head, so the kernels take the split of attn_wide.hip: the four waves of a workgroup work on the SAME
// 32 query (forward, dQ) or key (dK/dV) rows and wave w owns columns [64 w, 64 w + 64) of Q, K, V, dO, O, dQ, dK and dV, the
// d = 64 register picture of attn_stream.hpp with the operand helpers of attn_common.hpp on a column slice.  Per 32-row tile of
// the other operand every wave forms the partial 32 x 32 score tile of its slice, the four partials go through LDS and every
// wave adds them in the same order ((w0 + w1) + w2) + w3 (exchange()), so all waves hold bit-identical scores; dP = dO V^T is
// exchanged the same way.  What this family adds to that one:
//  * grouped KV heads: query head h reads KV head h / group, group = hq / hkv a runtime value; the dK/dV workgroup owns 32 keys
//    of one (sequence, KV head), walks the query heads of its group in order and, per head, the query tiles, accumulating into
//    the same registers: no atomics, no expanded K / V or dK / dV in HBM;
//  * CAUSAL: query tiles and key tiles are both 32 rows, so tile t of the keys is the diagonal tile of query tile t.  The key
//    loop of the forward and of dQ ends at the diagonal, the query loop of dK/dV starts there; tiles off the diagonal take the
//    compare-free path, the diagonal one compares key <= query per element and selects P = 0 before dS.  Key kv0 of a tile that
//    is computed is valid for each of the 32 queries (kv0 <= 32 t <= query, kv0 < kv_len), so the running max stays finite;
//  * the packed layout (AttnParams::cu): sequence i = rows [cu[i], cu[i + 1]); a tile past its sequence returns block-uniformly
//    before the first barrier.
// 1-D grids of (tile, (sequence, head)) work items.  LDS: two 32-row tiles of the full head width + the 16 KiB exchange area =
// 49.3 KiB (bf16) and 81.3 KiB (fp32, dynamic LDS above the 64 KiB default: set_attrs()).  Scores take the fp32 path for both
// dtypes; P and dS are rounded to bf16 before the second product as in every streaming kernel; delta is exact in fp32 through
// out_lo.  A repeated call gives identical bytes.
#include "attn_grouped.hpp"
#include "../../include/gmlm_hip_gqa_wide.h"

namespace gmlm {
namespace gqaw {

using grouped::Params, grouped::Seqs;

constexpr int NW = 4, NT = NW * 64, R = 32, KT = 32, D = 256, DS = D / NW, DB = DS / 32;

template <typename T> struct Lds {
  static constexpr int PITCH = D + Pad<T>::v;
  static constexpr int TILE = KT * PITCH * (int)sizeof(T);        // one 32-row tile, full head width
  static constexpr int XCH = NW * 16 * 64 * (int)sizeof(float);   // four partial 32 x 32 accumulator tiles
  static constexpr int SMALL = 2 * KT * (int)sizeof(float);       // dK/dV: lse and delta of the staged query rows
  static constexpr int BYTES = 2 * TILE + XCH + SMALL;
  static_assert(TILE % 16 == 0 && BYTES <= 160 * 1024, "LDS carve");
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

// key tiles [0, n) of query tile `tile`: below kv_len and, CAUSAL, up to the diagonal tile
template <bool CAUSAL>
__device__ __forceinline__ int key_tiles(int64_t kvlen, int64_t tile) {
  const int64_t n = (kvlen + KT - 1) / KT;
  return (int)(CAUSAL && tile + 1 < n ? tile + 1 : n);
}

// forward: workgroup = 32 query rows of one (sequence, query head), loop over key tiles of its KV head
template <typename T, bool CAUSAL>
__global__ __launch_bounds__(NT) void fwd_kernel(Params x) {
  const AttnParams& p = x.a;
  constexpr int PITCH = Lds<T>::PITCH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_gqaw[];
  T* ks = reinterpret_cast<T*>(smem_gqaw);
  T* vs = ks + KT * PITCH;
  float* xs = reinterpret_cast<float*>(smem_gqaw + 2 * Lds<T>::TILE);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const Item it = decode(p);
  const int64_t b = it.b, hd = it.hd, kvh = hd / x.group;
  int64_t lq_, lk_, qbase, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, qbase, kbase, lse_base);
  if (it.tile * R >= lq_) return;                                   // packed: a tile past its sequence (block-uniform)
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
  const float sl2 = p.scale * kLog2e;
  const int ntiles = key_tiles<CAUSAL>(kvlen, it.tile);
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
    if (kv0 + KT <= kvlen && !(CAUSAL && t == it.tile)) {           // whole tile valid (block-uniform): no per-key compare
#pragma unroll
      for (int i = 0; i < 16; ++i) rmax = fmaxf(rmax, s[i]);
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int64_t key = kv0 + acc_row(i, h);
        const float v = key < kvlen && (!CAUSAL || key <= q_row) ? s[i] : -INFINITY;
        s[i] = v;
        rmax = fmaxf(rmax, v);
      }
    }
    rmax = xhalf_max(rmax);
    float m_new = fmaxf(m, rmax * sl2);             // finite: key kv0 is valid for every row of the tile
    const bool keep = __all(m_new - m <= kDefer);   // identical in the four waves (identical scores); m = -inf -> false
    float alpha = 1.f;
    if (keep) m_new = m;
    else alpha = fast_exp2(m - m_new);
    float rsum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float e = fast_exp2(fmaf(s[i], sl2, -m_new));           // masked: exp2(-inf) = 0
      rsum += e;
      s[i] = e;
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
// [seqs * lq, hn, 256]; packed: seqs = 1 and lq = the packed rows, so delta is [hn, rows]
template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                    int64_t rows /* seqs * lq * hn */, int64_t lq, int64_t hn, float* __restrict__ delta) {
  constexpr int V = Store<T>::kVec;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  float acc = 0.f;
  if (row < rows) {
    for (int c = lane; c < D / V; c += 64) {
      float a[V], g[V];
      Store<T>::ldv(o + row * D + c * V, a);
      Store<T>::ldv(dout + row * D + c * V, g);
      if (o_lo) {
        float al[V];
        Store<T>::ldv(o_lo + row * D + c * V, al);
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

// backward: dQ.  workgroup = 32 queries of one (sequence, query head), loop over key tiles of its KV head.
//   S^T = K Q^T and dP^T = V dO^T as sums of four partials, P^T = exp(scale * S^T - lse[q]), dS^T = P^T * (dP^T - delta[q]),
//   dQ_w^T += K_w^T dS^T  (query on the lane)
template <typename T, bool CAUSAL>
__global__ __launch_bounds__(NT) void dq_kernel(Params x) {
  const AttnParams& p = x.a;
  constexpr int PITCH = Lds<T>::PITCH;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_gqaw[];
  T* ks = reinterpret_cast<T*>(smem_gqaw);
  T* vs = ks + KT * PITCH;
  float* xs = reinterpret_cast<float*>(smem_gqaw + 2 * Lds<T>::TILE);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const Item it = decode(p);
  const int64_t b = it.b, hd = it.hd, kvh = hd / x.group;
  int64_t lq_, lk_, qbase, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, qbase, kbase, lse_base);
  if (it.tile * R >= lq_) return;                                   // packed: a tile past its sequence (block-uniform)
  const int64_t q_row = it.tile * R + r;
  const bool q_ok = q_row < lq_;
  const int64_t kvlen = clamp_kvlen(p, b, lk_);
  const int64_t qr = q_ok ? q_row : 0;
  const T* kg = static_cast<const T*>(p.k) + kbase * p.k_stride + kvh * D;
  const T* vg = static_cast<const T*>(p.v) + kbase * p.v_stride + kvh * D;
  RowFrag<T, DS> qf, dof;
  qf.load(static_cast<const T*>(p.q) + (qbase + qr) * p.q_stride + hd * D + w * DS, q_ok, h);
  dof.load(static_cast<const T*>(p.dout) + (qbase + qr) * x.dout_stride + hd * D + w * DS, q_ok, h);
  const float sl2 = p.scale * kLog2e;
  const float lse2 = q_ok ? p.lse[lse_base + q_row] * kLog2e : INFINITY;   // a row past the sequence: probability 0 everywhere
  const float dl = q_ok ? p.delta[lse_base + q_row] : 0.f;
  const int kvl = (int)(kvlen < (1 << 30) ? kvlen : (1 << 30));
  const int qi = (int)(q_row < (1 << 30) ? q_row : (1 << 30));
  f32x16 dq[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[d][i] = 0.f;
  const int ntiles = key_tiles<CAUSAL>(kvlen, it.tile);
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
    const bool full = kv0 + KT <= kvlen && !(CAUSAL && t == it.tile);    // block-uniform
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float pr = fast_exp2(fmaf(s[i], sl2, -lse2));
      if (!full) {                                                  // the select: a masked pair has P = 0 whatever its score
        const int key = (int)kv0 + acc_row(i, h);
        pr = key < kvl && (!CAUSAL || key <= qi) ? pr : 0.f;
      }
      s[i] = pr * (dp[i] - dl);
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

// backward: dK, dV.  workgroup = 32 keys of one (sequence, KV head); for each query head of the group, in order, the query
// tiles of 32 in order (CAUSAL: from the diagonal tile on), all into the same registers (deterministic).
//   S = Q K^T and dP = dO V^T as sums of four partials, P = exp(scale * S - lse[q]), dV_w^T += dO_w^T P,
//   dS = P * (dP - delta[q]), dK_w^T += Q_w^T dS  (key on the lane, the query in the accumulator registers)
template <typename T, bool CAUSAL>
__global__ __launch_bounds__(NT) void dkv_kernel(Params x) {
  const AttnParams& p = x.a;
  constexpr int PITCH = Lds<T>::PITCH, QT = KT;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_gqaw[];
  T* qs = reinterpret_cast<T*>(smem_gqaw);
  T* dos = qs + QT * PITCH;
  float* xs = reinterpret_cast<float*>(smem_gqaw + 2 * Lds<T>::TILE);
  float* lse_s = xs + NW * 16 * 64;
  float* dl_s = lse_s + QT;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const CausalKeyTile it = causal_key_tile(p, x.group);             // key tile, sequence, KV head, first row, rows
  const int64_t b = it.b, kvh = it.kvh, base = it.base, l_ = it.l;
  if (it.kt * R >= l_) return;                                      // packed: a tile past its sequence (block-uniform)
  const int64_t kvlen = clamp_kvlen(p, b, l_);
  const int64_t key = it.kt * R + r;
  const bool key_in = key < l_;            // row exists in memory
  const bool key_ok = key < kvlen;         // takes part in the softmax
  const int64_t kr_ = key_in ? key : 0;
  const int ki = (int)(key < (1 << 30) ? key : (1 << 30));
  RowFrag<T, DS> kf, vf;
  kf.load(static_cast<const T*>(p.k) + (base + kr_) * p.k_stride + kvh * D + w * DS, key_in, h);
  vf.load(static_cast<const T*>(p.v) + (base + kr_) * p.v_stride + kvh * D + w * DS, key_in, h);
  const float sl2 = p.scale * kLog2e;
  f32x16 dk[DB], dv[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk[d][i] = 0.f; dv[d][i] = 0.f; }
  if (it.kt * R < kvlen) {                 // a whole workgroup past kv_len has nothing to accumulate (block-uniform)
    const int t0 = CAUSAL ? (int)it.kt : 0, ntiles = (int)((l_ + QT - 1) / QT);
    for (int g = 0; g < x.group; ++g) {
      const int64_t hd = kvh * x.group + g;
      const int64_t lse_base = p.cu ? hd * p.lq + base : (b * p.h + hd) * p.lq;   // [hq, T] or [b, hq, l], as seq_view()
      const T* qg = static_cast<const T*>(p.q) + base * p.q_stride + hd * D;
      const T* dog = static_cast<const T*>(p.dout) + base * x.dout_stride + hd * D;
      const float* lse_g = p.lse + lse_base;
      const float* dl_g = p.delta + lse_base;
      for (int t = t0; t < ntiles; ++t) {
        const int64_t q0 = (int64_t)t * QT;
        stage_rows<T, D, QT, NT>(qs, qg, p.q_stride, q0, l_, tid);
        stage_rows<T, D, QT, NT>(dos, dog, x.dout_stride, q0, l_, tid);
        if (tid < QT) {
          const bool ok = q0 + tid < l_;
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
        const bool diag = CAUSAL && t == t0;                        // block-uniform
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int q4 = 8 * g4 + 4 * h;                 // accumulator registers 4*g4 .. 4*g4+3 = queries q4 .. q4+3
          const float4 l4 = *reinterpret_cast<const float4*>(&lse_s[q4]);
          const float4 d4 = *reinterpret_cast<const float4*>(&dl_s[q4]);
          const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv4[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int i = 4 * g4 + j;
            const bool on = key_ok && (!diag || (int)q0 + q4 + j >= ki);
            const float pr = on ? fast_exp2(fmaf(s[i], sl2, -lv[j])) : 0.f;   // the select: P = 0 above the diagonal
            s[i] = pr;
            dp[i] = pr * (dp[i] - dv4[j]);
          }
        }
        mma_acc<DS>(dos + w * DS, PITCH, 0, s, dv, lane);
        mma_acc<DS>(qs + w * DS, PITCH, 0, dp, dk, lane);
        __syncthreads();                                            // tile consumed, also across the heads of the group
      }
    }
  }
  if (key_in) {
    T* dkg = static_cast<T*>(p.dk) + (base + key) * p.dk_stride + kvh * D + w * DS;
    T* dvg = static_cast<T*>(p.dv) + (base + key) * p.dv_stride + kvh * D + w * DS;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      store_t<T>(dkg + d * 32, dk[d], p.scale, h);
      store_t<T>(dvg + d * 32, dv[d], 1.f, h);
    }
  }
}

// the checks of attn_host.hpp up to the empty-problem return, in the order of grouped::setup, with this family's head dim and
// work-item bound; fills the launch parameters
static int setup(const char* who, Params& x, const Seqs& s, const void* q, const void* k, const void* v, int64_t hq, int64_t hkv,
                 int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p, const void* out_lo,
                 int dtype) {
  constexpr int64_t k2_30 = (int64_t)1 << 30;
  if (s.packed) {
    GMLM_REQUIRE(s.cu, "%s: null cu_seqlens", who);
    GMLM_REQUIRE(s.len > 0, "%s: max_len %ld must be positive", who, (long)s.len);
    GMLM_REQUIRE(s.n >= 0 && s.rows >= 0 && s.rows < k2_30, "%s: %ld packed rows (must be >= 0 and < 2^30)", who, (long)s.rows);
  }
  int rc = attn_check_shape(who, (s.packed ? s.len < k2_30 && s.n < k2_30 : s.n >= 0 && s.len >= 0 && s.lk >= 0) && hq > 0 && hkv > 0,
                            d == D, d, "this entry point takes 256", dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(s.len == s.lk, "%s: self-attention needs lq == lk (got %ld and %ld)", who, (long)s.len, (long)s.lk);
  GMLM_REQUIRE(hq % hkv == 0, "%s: %ld query heads are not a multiple of %ld KV heads", who, (long)hq, (long)hkv);
  if ((rc = attn_check_rates(who, dropout_p, "grouped", scale)) != GMLM_OK) return rc;
  GMLM_REQUIRE(s.len < k2_30 && hq < k2_30 && s.n < ((int64_t)1 << 31) &&
                   (double)cdiv(s.len, R) * (double)s.n * (double)hq < 2147483648.0 &&
                   (double)s.rows * (double)s.lse_seqs() * (double)hq < 4.0 * 2147483648.0,   // the delta launch: one wave per row
               "%s: too many work items", who);
  x = Params{};
  attn_fill(x.a, q, k, v, s.kv_len, s.n, hq, s.rows, s.rows, q_stride, k_stride, v_stride, scale, 0.f, 0, nullptr);
  x.a.cu = s.cu;
  x.dout_stride = hq * d;
  x.group = (int32_t)(hq / hkv);
  return GMLM_OK;
}

// > 64 KiB of dynamic LDS (fp32) needs the attribute once per instantiation and device; set for every instantiation, so that
// none depends on the default
template <typename T, bool CAUSAL> static int set_attrs() {
  constexpr int kLds = Lds<T>::BYTES;
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fwd_kernel<T, CAUSAL>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dq_kernel<T, CAUSAL>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dkv_kernel<T, CAUSAL>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  return GMLM_OK;
}
static int prepare() {
  static PerDeviceOnce once;
  return once([]() -> int {
    int rc;
    if ((rc = set_attrs<bf16_t, false>()) != GMLM_OK) return rc;
    if ((rc = set_attrs<bf16_t, true>()) != GMLM_OK) return rc;
    if ((rc = set_attrs<float, false>()) != GMLM_OK) return rc;
    return set_attrs<float, true>();
  });
}

#define GMLM_GQAW_LAUNCH(KERNEL, GRID)                                                              \
  do {                                                                                              \
    const dim3 grid_((unsigned)(GRID));                                                             \
    if (dtype == GMLM_BF16) {                                                                       \
      if (causal) KERNEL<bf16_t, true><<<grid_, NT, Lds<bf16_t>::BYTES, st>>>(x);                   \
      else KERNEL<bf16_t, false><<<grid_, NT, Lds<bf16_t>::BYTES, st>>>(x);                         \
    } else {                                                                                        \
      if (causal) KERNEL<float, true><<<grid_, NT, Lds<float>::BYTES, st>>>(x);                     \
      else KERNEL<float, false><<<grid_, NT, Lds<float>::BYTES, st>>>(x);                           \
    }                                                                                               \
    GMLM_LAUNCH_CHECK();                                                                            \
  } while (0)

// ---- the entry points: a padded export passes grouped::padded(...), its varlen twin grouped::packed(...) -----------------------
static int fwd(const char* who, const Seqs& s, const void* q, const void* k, const void* v, int64_t hq, int64_t hkv, int64_t d,
               int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p, int causal, void* out, void* out_lo,
               float* lse, int dtype, gmlm_stream_t stream) {
  Params x;
  int rc = setup(who, x, s, q, k, v, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (s.empty()) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, hq * d, hkv * d, dtype)) != GMLM_OK) return rc;
  if ((rc = prepare()) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  GMLM_GQAW_LAUNCH(fwd_kernel, cdiv(s.len, R) * s.n * hq);
  return GMLM_OK;
}

static int bwd(const char* who, const Seqs& s, const void* q, const void* k, const void* v, const void* out, const void* out_lo,
               const void* dout, const float* lse, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride, int64_t k_stride,
               int64_t v_stride, float scale, float dropout_p, int causal, void* dq, void* dk, void* dv, int64_t dq_stride,
               int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  Params x;
  int rc = setup(who, x, s, q, k, v, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (s.empty()) return GMLM_OK;
  AttnParams& p = x.a;
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, p, hq * d, hkv * d, dtype, workspace_bytes, attn_delta_bytes(s.lse_seqs(), hq, s.rows))) != GMLM_OK)
    return rc;
  if ((rc = prepare()) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t drows = s.lse_seqs() * s.rows * hq;
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, drows, 64, st, s.rows, hq);       // one wave per row
  GMLM_LAUNCH_CHECK();
  GMLM_GQAW_LAUNCH(dq_kernel, cdiv(s.len, R) * s.n * hq);
  GMLM_GQAW_LAUNCH(dkv_kernel, cdiv(s.len, R) * s.n * hkv);
  return GMLM_OK;
}

}  // namespace gqaw
}  // namespace gmlm

using namespace gmlm;

extern "C" int gmlm_attention_gqa_d256_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                           int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                           int64_t v_stride, float scale, float dropout_p, int causal, void* out, void* out_lo,
                                           float* lse, int dtype, gmlm_stream_t stream) {
  return gqaw::fwd("attention_gqa_d256_fwd", grouped::padded(kv_len, b, lq, lk), q, k, v, hq, hkv, d, q_stride, k_stride, v_stride, scale,
                   dropout_p, causal, out, out_lo, lse, dtype, stream);
}

extern "C" size_t gmlm_attention_gqa_d256_bwd_workspace_bytes(int64_t b, int64_t hq, int64_t lq) { return attn_delta_bytes(b, hq, lq); }

extern "C" int gmlm_attention_gqa_d256_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                           const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq,
                                           int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                           int64_t v_stride, float scale, float dropout_p, int causal, void* dq, void* dk, void* dv,
                                           int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                           size_t workspace_bytes, gmlm_stream_t stream) {
  return gqaw::bwd("attention_gqa_d256_bwd", grouped::padded(kv_len, b, lq, lk), q, k, v, out, out_lo, dout, lse, hq, hkv, d, q_stride,
                   k_stride, v_stride, scale, dropout_p, causal, dq, dk, dv, dq_stride, dk_stride, dv_stride, dtype, workspace,
                   workspace_bytes, stream);
}

extern "C" int gmlm_attention_gqa_d256_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                                  int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv,
                                                  int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                                  float dropout_p, int causal, void* out, void* out_lo, float* lse, int dtype,
                                                  gmlm_stream_t stream) {
  return gqaw::fwd("attention_gqa_d256_varlen_fwd", grouped::packed(cu_seqlens, num_seqs, max_len, total_rows), q, k, v, hq, hkv, d,
                   q_stride, k_stride, v_stride, scale, dropout_p, causal, out, out_lo, lse, dtype, stream);
}

extern "C" size_t gmlm_attention_gqa_d256_varlen_bwd_workspace_bytes(int64_t total_rows, int64_t hq) {
  return attn_delta_bytes(1, hq, total_rows);   // delta [hq, total_rows]
}

extern "C" int gmlm_attention_gqa_d256_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                                  const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                                  int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d,
                                                  int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                                                  int causal, void* dq, void* dk, void* dv, int64_t dq_stride, int64_t dk_stride,
                                                  int64_t dv_stride, int dtype, void* workspace, size_t workspace_bytes,
                                                  gmlm_stream_t stream) {
  return gqaw::bwd("attention_gqa_d256_varlen_bwd", grouped::packed(cu_seqlens, num_seqs, max_len, total_rows), q, k, v, out, out_lo,
                   dout, lse, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, causal, dq, dk, dv, dq_stride, dk_stride,
                   dv_stride, dtype, workspace, workspace_bytes, stream);
}
