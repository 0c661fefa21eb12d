// Row kernels of the Gemma3 text encoder (hf:modeling_gemma3.py; C ABI in include/gmlm_hip_gqa_wide.h): the sandwich RMSNorm
// pair, the per-head RMSNorm of Q / K followed by the rotate-half rotation at head dim 256, and the tanh-GELU gated unit.
// bf16 or fp32 storage, fp32 arithmetic, ONE rounding on store.  HBM-bound streaming kernels; every reduction across rows runs
// in a fixed order (col_reduce, or block partials + rows_sum_kernel): no atomics, identical calls give identical bits.  The
// pieces shared with decoder_kernels.hip and modernbert_kernels.hip (lane sums, the rotary helpers, the GLU bodies) are in
// row_kernels.hpp.
#include "row_kernels.hpp"
#include "../../include/gmlm_hip_gqa_wide.h"

namespace gmlm {
namespace gemma_kernels {

// ------------------------------------------------------------------------------------------------
// Sandwich RMSNorm.  A Gemma3 block output is normed BEFORE it joins the residual stream and the sum is normed again for the
// next block:  s' = s + b * rstd_b * (off + w_post)  (stored once as T),  y = s' * rstd_s * (off + w_pre), rstd_s taken from the
// STORED s' as add_rmsnorm takes it.  One wave per row, CH 16-byte chunks per lane (f <= 64 * CH * V), the row stays in
// registers: b is read once, s once, s' and y are written once: one launch and one [rows, f] round trip less than the two
// add_rmsnorm launches this replaces.
// ------------------------------------------------------------------------------------------------
template <typename T, int CH>
__global__ __launch_bounds__(256) void sandwich_fwd_kernel(const T* __restrict__ s, const T* __restrict__ b,
                                                            const float* __restrict__ w_post, const float* __restrict__ w_pre,
                                                            int64_t rows, int f, float off, float eps, T* __restrict__ s_out,
                                                            T* __restrict__ y, float* __restrict__ rstd_b,
                                                            float* __restrict__ rstd_s) {
  constexpr int V = Store<T>::kVec;
  const int lane = threadIdx.x & 63, nch = f / V;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                                   // wave-uniform; no barrier in this kernel
  float z[CH][V];
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      Store<T>::ldv(b + r * f + (int64_t)ch * V, z[c]);
#pragma unroll
      for (int v = 0; v < V; ++v) acc = fmaf(z[c][v], z[c][v], acc);
    }
  }
  const float rb = 1.f / sqrtf(lanes_sum<64>(acc) / (float)f + eps);
  acc = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      const int64_t o = r * f + (int64_t)ch * V;
      float wv[V], t[V];
      load_f32<V>(w_post + ch * V, wv);
      if (s) Store<T>::ldv(s + o, t);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float n = z[c][v] * rb * (off + wv[v]);
        z[c][v] = rounded<T>(s ? t[v] + n : n);
        acc = fmaf(z[c][v], z[c][v], acc);
      }
      Store<T>::stv(s_out + o, z[c]);
    }
  }
  const float rs = 1.f / sqrtf(lanes_sum<64>(acc) / (float)f + eps);
  if (lane == 0) { rstd_b[r] = rb; rstd_s[r] = rs; }
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      float wv[V], o[V];
      load_f32<V>(w_pre + ch * V, wv);
#pragma unroll
      for (int v = 0; v < V; ++v) o[v] = z[c][v] * rs * (off + wv[v]);
      Store<T>::stv(y + r * f + (int64_t)ch * V, o);
    }
  }
}

// ds' = ds_in + rstd_s (g - xhat mean(g xhat)),  g = dy (off + w_pre),  xhat = s' rstd_s:  the whole gradient of s', = ds;
// db  = rstd_b (h - bhat mean(h bhat)),          h = ds' (off + w_post), bhat = b rstd_b.
// mean(g xhat) of every row is kept in fp32 (m2) for the column sums below.
template <typename T, int CH>
__global__ __launch_bounds__(256) void sandwich_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ ds_in,
                                                            const T* __restrict__ b, const T* __restrict__ sp,
                                                            const float* __restrict__ w_post, const float* __restrict__ w_pre,
                                                            const float* __restrict__ rstd_b, const float* __restrict__ rstd_s,
                                                            int64_t rows, int f, float off, T* __restrict__ ds,
                                                            T* __restrict__ db, float* __restrict__ m2_out) {
  constexpr int V = Store<T>::kVec;
  const int lane = threadIdx.x & 63, nch = f / V;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float rs = rstd_s[r], rb = rstd_b[r];
  float g[CH][V], xh[CH][V];
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      const int64_t o = r * f + (int64_t)ch * V;
      float wv[V];
      Store<T>::ldv(dy + o, g[c]);
      Store<T>::ldv(sp + o, xh[c]);
      load_f32<V>(w_pre + ch * V, wv);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        g[c][v] *= off + wv[v];
        xh[c][v] *= rs;
        dot += g[c][v] * xh[c][v];
      }
    }
  }
  const float m2 = lanes_sum<64>(dot) / (float)f;
  if (lane == 0) m2_out[r] = m2;
  dot = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      const int64_t o = r * f + (int64_t)ch * V;
      float wv[V], t[V];
#pragma unroll
      for (int v = 0; v < V; ++v) g[c][v] = rs * (g[c][v] - xh[c][v] * m2);
      if (ds_in) {
        Store<T>::ldv(ds_in + o, t);
#pragma unroll
        for (int v = 0; v < V; ++v) g[c][v] += t[v];
      }
      if (ds) Store<T>::stv(ds + o, g[c]);
      Store<T>::ldv(b + o, xh[c]);
      load_f32<V>(w_post + ch * V, wv);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        g[c][v] *= off + wv[v];
        xh[c][v] *= rb;
        dot += g[c][v] * xh[c][v];
      }
    }
  }
  const float m1 = lanes_sum<64>(dot) / (float)f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      float o[V];
#pragma unroll
      for (int v = 0; v < V; ++v) o[v] = rb * (g[c][v] - xh[c][v] * m1);
      Store<T>::stv(db + r * f + (int64_t)ch * V, o);
    }
  }
}

// column sums of the weight gradients (col_reduce: fixed order): v[0] = ds' * bhat (dw_post), v[1] = dy * xhat (dw_pre); ds' is
// formed again in fp32 from the row's saved mean, not read back from its rounded store
template <typename T>
struct SandwichDwFn {
  const T *dy, *ds_in, *b, *sp;
  const float *w_pre, *rstd_b, *rstd_s, *m2;
  int64_t f;
  float off;
  __device__ __forceinline__ void operator()(int64_t r, int64_t c, float (&v)[2]) const {
    const float g = Store<T>::ld(dy + r * f + c), rs = rstd_s[r], x = Store<T>::ld(sp + r * f + c) * rs;
    float dsp = rs * (g * (off + w_pre[c]) - x * m2[r]);
    if (ds_in) dsp += Store<T>::ld(ds_in + r * f + c);
    v[0] = dsp * (Store<T>::ld(b + r * f + c) * rstd_b[r]);
    v[1] = g * x;
  }
};

// ------------------------------------------------------------------------------------------------
// Q / K head norm + rotary embedding at head dim 256.  A head row of 256 elements = 32 lanes (bf16) or 64 lanes (fp32) x 16
// bytes.   n = x * rsqrt(mean(x^2) + eps) * (off + w);   out[i] = n[i] cos[i] - n[i + 128] sin[i],
// out[i + 128] = n[i + 128] cos[i] + n[i] sin[i].  Every lane reads its own chunk and takes its partner's by a cross-lane
// exchange before it stores, so out == qkv (in place) is fine.
// ------------------------------------------------------------------------------------------------
constexpr int kHeadDim = 256;

template <typename T>
__global__ __launch_bounds__(256) void qknorm_rope_fwd_kernel(const T* qkv, int64_t in_stride, const float* __restrict__ qw,
                                                               const float* __restrict__ kw, const float* __restrict__ cs,
                                                               int64_t tokens, int64_t seq_len, int hq, int hkv, float off,
                                                               float eps, T* out, int64_t out_stride, float* __restrict__ rstd_o,
                                                               const int32_t* __restrict__ pos_ids, int64_t max_len) {
  constexpr int V = Store<T>::kVec, LPR = kHeadDim / V;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lr = (int)(gid % LPR), nh = hq + hkv;
  const int64_t item = gid / LPR;
  int64_t t;
  int hd;
  const bool live = head_row(item, tokens * nh, nh, t, hd);
  float x[V], wv[V], c[V], sn[V];
  Store<T>::ldv(qkv + t * in_stride + (int64_t)hd * kHeadDim + lr * V, x);
  load_f32<V>((hd < hq ? qw : kw) + lr * V, wv);
  const int col = (lr * V) & (kHeadDim / 2 - 1);
  const float* csr = rope_row<kHeadDim>(cs, t, seq_len, pos_ids, max_len);
  load_f32<V>(csr + col, c);
  load_f32<V>(csr + kHeadDim / 2 + col, sn);
  float sq = 0.f;
#pragma unroll
  for (int v = 0; v < V; ++v) sq += x[v] * x[v];
  const float rs = 1.f / sqrtf(lanes_sum<LPR>(sq) / (float)kHeadDim + eps);
  const bool upper = lr >= LPR / 2;
  float o[V];
#pragma unroll
  for (int v = 0; v < V; ++v) o[v] = rotate_half<LPR, false>(x[v] * rs * (off + wv[v]), c[v], sn[v], upper);
  if (live) {
    Store<T>::stv(out + t * out_stride + (int64_t)hd * kHeadDim + lr * V, o);
    if (lr == 0) rstd_o[item] = rs;
  }
}

// Backward, in place on the leading (hq + hkv) * 256 columns of the fused dqkv rows: inverse rotation, then the RMSNorm
// backward.  Weight gradients: every thread keeps the sums of its fixed columns over its grid-stride rows (Q and K heads
// apart), the block adds its row groups through LDS in a fixed order and writes ONE partial row [2][256]; rows_sum_kernel
// adds the blocks.
template <typename T>
__global__ __launch_bounds__(256) void qknorm_rope_bwd_kernel(T* __restrict__ dqkv, int64_t d_stride, const T* __restrict__ qkv,
                                                               int64_t in_stride, const float* __restrict__ qw,
                                                               const float* __restrict__ kw, const float* __restrict__ cs,
                                                               const float* __restrict__ rstd, int64_t tokens, int64_t seq_len,
                                                               int hq, int hkv, float off, float* __restrict__ partial,
                                                               const int32_t* __restrict__ pos_ids, int64_t max_len) {
  constexpr int V = Store<T>::kVec, LPR = kHeadDim / V, RPB = 256 / LPR;
  __shared__ float red[RPB][2][kHeadDim];
  const int lr = threadIdx.x % LPR, grp = threadIdx.x / LPR, nh = hq + hkv;
  const int64_t items = tokens * nh;
  const int col = (lr * V) & (kHeadDim / 2 - 1);
  const bool upper = lr >= LPR / 2;
  float wq[V], wk[V], accq[V], acck[V];
  load_f32<V>(qw + lr * V, wq);
  load_f32<V>(kw + lr * V, wk);
#pragma unroll
  for (int v = 0; v < V; ++v) { wq[v] += off; wk[v] += off; accq[v] = 0.f; acck[v] = 0.f; }
  // every lane group runs the same number of iterations (the shuffles need all lanes of a wave)
  const int64_t per_pass = (int64_t)gridDim.x * RPB;
  const int64_t iters = (items + per_pass - 1) / per_pass;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t item = (it * gridDim.x + blockIdx.x) * RPB + grp;
    const bool live = item < items;
    const int64_t t = live ? item / nh : 0;
    const int hd = live ? (int)(item % nh) : 0;
    const bool is_k = hd >= hq;
    float g[V], x[V], c[V], sn[V];
    T* dptr = dqkv + t * d_stride + (int64_t)hd * kHeadDim + lr * V;
    Store<T>::ldv(dptr, g);
    Store<T>::ldv(qkv + t * in_stride + (int64_t)hd * kHeadDim + lr * V, x);
    const float* csr = rope_row<kHeadDim>(cs, t, seq_len, pos_ids, max_len);
    load_f32<V>(csr + col, c);
    load_f32<V>(csr + kHeadDim / 2 + col, sn);
    const float rs = rstd[live ? item : 0];
    float dot = 0.f, dn[V], xh[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      dn[v] = rotate_half<LPR, true>(g[v], c[v], sn[v], upper);   // R^T dout
      xh[v] = x[v] * rs;
      if (live) {
        if (is_k) acck[v] += dn[v] * xh[v];
        else accq[v] += dn[v] * xh[v];
      }
      dn[v] *= is_k ? wk[v] : wq[v];
      dot += dn[v] * xh[v];
    }
    const float m = lanes_sum<LPR>(dot) / (float)kHeadDim;
    if (live) {
      float o[V];
#pragma unroll
      for (int v = 0; v < V; ++v) o[v] = rs * (dn[v] - xh[v] * m);
      Store<T>::stv(dptr, o);
    }
  }
#pragma unroll
  for (int v = 0; v < V; ++v) {
    red[grp][0][lr * V + v] = accq[v];
    red[grp][1][lr * V + v] = acck[v];
  }
  __syncthreads();
#pragma unroll
  for (int o = 0; o < 2; ++o) {                            // 512 sums over 256 threads: thread t adds column t of the Q, then of the K row
    float sum = 0.f;
#pragma unroll
    for (int g = 0; g < RPB; ++g) sum += red[g][o][threadIdx.x];
    partial[(int64_t)blockIdx.x * 2 * kHeadDim + o * kHeadDim + threadIdx.x] = sum;
  }
}

// ------------------------------------------------------------------------------------------------
// tanh-GELU gated unit: y = gelu_tanh(gate) * up.  With u = sqrt(2 / pi) (g + 0.044715 g^3), 0.5 (1 + tanh u) = sigmoid(2 u).
// sigmoid(2 u) and its complement are formed from e = exp(-2 |u|) in (0, 1]: 1 / (1 + e) and e / (1 + e), swapped by the sign
// of u.  No difference of nearly equal numbers, no overflow: a saturated gate has e = 0, so the pair is exactly (1, 0) or
// (0, 1), the value exactly g or 0 and the derivative exactly 1 or 0; no NaN for any finite gate.
// ------------------------------------------------------------------------------------------------
struct TanhGeluAct {
  static constexpr float kA = 0.7978845608028654f, kB = 0.044715f;
  // sig = sigmoid(2 u(g)), co = 1 - sig, du2 = d(2 u) / dg
  static __device__ __forceinline__ void parts(float g, float& sig, float& co, float& du2) {
    const float g2 = g * g;
    const float u = kA * g * fmaf(kB, g2, 1.f);
    const float e = expf(-2.f * fabsf(u));
    const float big = 1.f / (1.f + e), small = e * big;
    sig = u >= 0.f ? big : small;
    co = u >= 0.f ? small : big;
    du2 = 2.f * kA * fmaf(3.f * kB, g2, 1.f);
  }
  template <typename T> static __device__ __forceinline__ float fwd(float g) {
    float sig, co, du2;
    parts(g, sig, co, du2);
    return g * sig;
  }
  // d (act(g) * u) -> dg, du;  act' = sig (1 + g (1 - sig) (2 u)')
  template <typename T> static __device__ __forceinline__ void bwd(float d, float g, float u, float& dg, float& du) {
    float sig, co, du2;
    parts(g, sig, co, du2);
    du = d * g * sig;
    dg = d * u * sig * fmaf(g * co, du2, 1.f);
  }
};

template <typename T>
__global__ __launch_bounds__(256) void geglu_tanh_fwd_kernel(const T* __restrict__ gu, int64_t rows, int64_t inter, T* __restrict__ y) {
  glu_fwd_body<T, TanhGeluAct>(gu, rows, inter, y);
}

template <typename T>
__global__ __launch_bounds__(256) void geglu_tanh_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ gu, int64_t rows,
                                                              int64_t inter, T* __restrict__ dgu) {
  glu_bwd_body<T, TanhGeluAct>(dy, gu, rows, inter, dgu);
}

// ---- host ----------------------------------------------------------------------------------------
static int rms_check(const char* who, int64_t rows, int64_t f, int dtype) {
  GMLM_REQUIRE(dtype == GMLM_F32 || dtype == GMLM_BF16, "%s: unsupported dtype", who);
  const int v = dtype == GMLM_F32 ? 4 : 8;
  GMLM_REQUIRE(rows >= 0 && f > 0 && f <= 4096 && f % v == 0, "%s: row width %ld must be a multiple of %d, at most 4096", who, (long)f, v);
  GMLM_REQUIRE(cdiv(rows, 4) < ((int64_t)1 << 31), "%s: too many rows", who);
  return GMLM_OK;
}

// smallest instantiated chunk count covering f / V chunks over 64 lanes; WIDEST = the count f = 4096 needs (8 chunks of
// 8 bf16, 16 chunks of 4 fp32), so that no instantiation exists that cannot be launched
#define GMLM_SANDWICH_DISPATCH(T, WIDEST, KERNEL, ...)                                        \
  do {                                                                                        \
    const int need_ = (int)cdiv(f / Store<T>::kVec, 64);                                      \
    const unsigned grid_ = (unsigned)cdiv(rows, 4);                                           \
    if (need_ <= 2) KERNEL<T, 2><<<grid_, 256, 0, st>>>(__VA_ARGS__);                         \
    else if (need_ <= 4) KERNEL<T, 4><<<grid_, 256, 0, st>>>(__VA_ARGS__);                    \
    else if (need_ <= 8) KERNEL<T, 8><<<grid_, 256, 0, st>>>(__VA_ARGS__);                    \
    else KERNEL<T, WIDEST><<<grid_, 256, 0, st>>>(__VA_ARGS__);                               \
  } while (0)

// the fp32 row means in front of the column-sum partials; a multiple of 16 bytes
static size_t sandwich_m2_bytes(int64_t rows) { return (size_t)((rows > 0 ? rows : 0) + 3) / 4 * 16; }

constexpr int kRopeBwdMaxBlocks = 1024;
static int64_t rope_bwd_blocks(int64_t items, int dtype) {
  const int64_t rpb = dtype == GMLM_F32 ? 4 : 8;
  const int64_t nb = cdiv(items, rpb);
  return nb < 1 ? 1 : (nb > kRopeBwdMaxBlocks ? kRopeBwdMaxBlocks : nb);
}

// rope_sizes (row_kernels.hpp) first, pointers second: a call with no token returns GMLM_OK in between
static int rope_ptrs(const char* who, const void* qkv, const void* other, const float* qw, const float* kw, const float* cs,
                     const float* rstd, bool by_pos, const int32_t* pos_ids) {
  GMLM_REQUIRE(qkv && other && aligned16(qkv) && aligned16(other), "%s: null or not 16-byte aligned pointer", who);
  GMLM_REQUIRE(qw && kw && cs && aligned16(qw) && aligned16(kw) && aligned16(cs), "%s: null or misaligned weight / table", who);
  GMLM_REQUIRE(rstd, "%s: null rstd", who);
  GMLM_REQUIRE(!by_pos || pos_ids, "%s: null pos_ids", who);
  return GMLM_OK;
}

// by_pos: position = pos_ids[row] (seq_len unused, passed as 1); else pos_ids is NULL and position = row % seq_len
static int rope_fwd(const char* who, const void* qkv, int64_t qkv_stride, const float* q_weight, const float* k_weight,
                    const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len, bool by_pos, const int32_t* pos_ids,
                    int64_t hq, int64_t hkv, int64_t d, float w_offset, float eps, void* out, int64_t out_stride, float* rstd,
                    int dtype, gmlm_stream_t stream) {
  int rc = rope_sizes(who, kHeadDim, qkv_stride, out_stride, (hq + hkv) * kHeadDim, tokens, seq_len, by_pos, max_len, hq, hkv, d, dtype);
  if (rc != GMLM_OK) return rc;
  if (tokens == 0) return GMLM_OK;
  if ((rc = rope_ptrs(who, qkv, out, q_weight, k_weight, cos_sin, rstd, by_pos, pos_ids)) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t items = tokens * (hq + hkv);
  if (dtype == GMLM_BF16)
    qknorm_rope_fwd_kernel<bf16_t><<<(unsigned)cdiv(items * 32, 256), 256, 0, st>>>((const bf16_t*)qkv, qkv_stride, q_weight, k_weight,
        cos_sin, tokens, seq_len, (int)hq, (int)hkv, w_offset, eps, (bf16_t*)out, out_stride, rstd, pos_ids, max_len);
  else
    qknorm_rope_fwd_kernel<float><<<(unsigned)cdiv(items * 64, 256), 256, 0, st>>>((const float*)qkv, qkv_stride, q_weight, k_weight,
        cos_sin, tokens, seq_len, (int)hq, (int)hkv, w_offset, eps, (float*)out, out_stride, rstd, pos_ids, max_len);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

static size_t rope_bwd_ws(int64_t tokens, int64_t hq, int64_t hkv, int dtype) {
  return (size_t)rope_bwd_blocks(tokens * (hq + hkv), dtype) * 2 * kHeadDim * sizeof(float);
}

static int rope_bwd(const char* who, void* dqkv, int64_t dqkv_stride, const void* qkv, int64_t qkv_stride, const float* q_weight,
                    const float* k_weight, const float* cos_sin, int64_t max_len, const float* rstd, int64_t tokens,
                    int64_t seq_len, bool by_pos, const int32_t* pos_ids, int64_t hq, int64_t hkv, int64_t d, float w_offset,
                    float* dq_weight, float* dk_weight, int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  int rc = rope_sizes(who, kHeadDim, qkv_stride, dqkv_stride, (hq + hkv) * kHeadDim, tokens, seq_len, by_pos, max_len, hq, hkv, d, dtype);
  if (rc != GMLM_OK) return rc;
  // the one output a call with no token still has: zero weight gradients
  GMLM_REQUIRE(dq_weight && dk_weight && dk_weight == dq_weight + kHeadDim, "%s: dq_weight | dk_weight are one fp32 [2, 256] buffer", who);
  hipStream_t st = as_stream(stream);
  if (tokens == 0) {
    hipError_t e = zero_async(dq_weight, 2 * kHeadDim * sizeof(float), st);
    if (e != hipSuccess) { set_error("%s: zero fill failed: %s", who, hipGetErrorString(e)); return GMLM_ELAUNCH; }
    return GMLM_OK;
  }
  if ((rc = rope_ptrs(who, qkv, dqkv, q_weight, k_weight, cos_sin, rstd, by_pos, pos_ids)) != GMLM_OK) return rc;
  GMLM_REQUIRE_WS(workspace && workspace_bytes >= rope_bwd_ws(tokens, hq, hkv, dtype), "%s: workspace too small", who);
  const int nb = (int)rope_bwd_blocks(tokens * (hq + hkv), dtype);
  float* partial = static_cast<float*>(workspace);
  if (dtype == GMLM_BF16)
    qknorm_rope_bwd_kernel<bf16_t><<<nb, 256, 0, st>>>((bf16_t*)dqkv, dqkv_stride, (const bf16_t*)qkv, qkv_stride, q_weight, k_weight,
        cos_sin, rstd, tokens, seq_len, (int)hq, (int)hkv, w_offset, partial, pos_ids, max_len);
  else
    qknorm_rope_bwd_kernel<float><<<nb, 256, 0, st>>>((float*)dqkv, dqkv_stride, (const float*)qkv, qkv_stride, q_weight, k_weight,
        cos_sin, rstd, tokens, seq_len, (int)hq, (int)hkv, w_offset, partial, pos_ids, max_len);
  GMLM_LAUNCH_CHECK();
  rows_sum_kernel<<<2 * kHeadDim / 32, 256, 0, st>>>(partial, nb, 2 * kHeadDim, dq_weight);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

}  // namespace gemma_kernels
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::gemma_kernels;

extern "C" int gmlm_sandwich_rmsnorm_fwd(const void* s, const void* b, const float* w_post, const float* w_pre, int64_t rows,
                                         int64_t f, float w_offset, float eps, void* s_out, void* y, float* rstd_b, float* rstd_s,
                                         int dtype, gmlm_stream_t stream) {
  static const char* who = "sandwich_rmsnorm_fwd";
  int rc = rms_check(who, rows, f, dtype);
  if (rc != GMLM_OK) return rc;
  if (rows == 0) return GMLM_OK;
  GMLM_REQUIRE(b && w_post && w_pre && s_out && y && rstd_b && rstd_s && aligned16(s) && aligned16(b) && aligned16(w_post) &&
                   aligned16(w_pre) && aligned16(s_out) && aligned16(y),
               "%s: null or not 16-byte aligned pointer", who);
  hipStream_t st = as_stream(stream);
  if (dtype == GMLM_BF16)
    GMLM_SANDWICH_DISPATCH(bf16_t, 8, sandwich_fwd_kernel, (const bf16_t*)s, (const bf16_t*)b, w_post, w_pre, rows, (int)f, w_offset, eps,
                           (bf16_t*)s_out, (bf16_t*)y, rstd_b, rstd_s);
  else
    GMLM_SANDWICH_DISPATCH(float, 16, sandwich_fwd_kernel, (const float*)s, (const float*)b, w_post, w_pre, rows, (int)f, w_offset, eps,
                           (float*)s_out, (float*)y, rstd_b, rstd_s);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_sandwich_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t f) {
  return sandwich_m2_bytes(rows) + col_reduce_workspace_bytes(rows, f, 2);
}

extern "C" int gmlm_sandwich_rmsnorm_bwd(const void* dy, const void* ds_in, const void* b, const void* s_out, const float* w_post,
                                         const float* w_pre, const float* rstd_b, const float* rstd_s, int64_t rows, int64_t f,
                                         float w_offset, void* ds, void* db, float* dw_post, float* dw_pre, int dtype,
                                         void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "sandwich_rmsnorm_bwd";
  int rc = rms_check(who, rows, f, dtype);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(dw_post && dw_pre && dw_pre == dw_post + f, "%s: dw_post | dw_pre are one fp32 [2, f] buffer", who);
  GMLM_REQUIRE_WS(rows == 0 || (workspace && workspace_bytes >= gmlm_sandwich_rmsnorm_bwd_workspace_bytes(rows, f)),
                  "%s: workspace too small", who);
  hipStream_t st = as_stream(stream);
  float* m2 = static_cast<float*>(workspace);
  void* part = rows > 0 ? static_cast<unsigned char*>(workspace) + sandwich_m2_bytes(rows) : nullptr;
  const size_t part_bytes = rows > 0 ? workspace_bytes - sandwich_m2_bytes(rows) : 0;
  if (rows > 0) {
    GMLM_REQUIRE(dy && b && s_out && w_post && w_pre && rstd_b && rstd_s && db && aligned16(dy) && aligned16(ds_in) && aligned16(b) &&
                     aligned16(s_out) && aligned16(w_post) && aligned16(w_pre) && aligned16(ds) && aligned16(db),
                 "%s: null or not 16-byte aligned pointer", who);
    if (dtype == GMLM_BF16)
      GMLM_SANDWICH_DISPATCH(bf16_t, 8, sandwich_bwd_kernel, (const bf16_t*)dy, (const bf16_t*)ds_in, (const bf16_t*)b,
                             (const bf16_t*)s_out, w_post, w_pre, rstd_b, rstd_s, rows, (int)f, w_offset, (bf16_t*)ds, (bf16_t*)db, m2);
    else
      GMLM_SANDWICH_DISPATCH(float, 16, sandwich_bwd_kernel, (const float*)dy, (const float*)ds_in, (const float*)b, (const float*)s_out,
                             w_post, w_pre, rstd_b, rstd_s, rows, (int)f, w_offset, (float*)ds, (float*)db, m2);
    GMLM_LAUNCH_CHECK();
  }
  if (dtype == GMLM_BF16)
    return col_reduce<2>(rows, f, SandwichDwFn<bf16_t>{(const bf16_t*)dy, (const bf16_t*)ds_in, (const bf16_t*)b, (const bf16_t*)s_out,
                                                       w_pre, rstd_b, rstd_s, m2, f, w_offset}, dw_post, part, part_bytes, st);
  return col_reduce<2>(rows, f, SandwichDwFn<float>{(const float*)dy, (const float*)ds_in, (const float*)b, (const float*)s_out, w_pre,
                                                    rstd_b, rstd_s, m2, f, w_offset}, dw_post, part, part_bytes, st);
}

extern "C" int gmlm_qknorm_rope_d256_fwd(const void* qkv, int64_t qkv_stride, const float* q_weight, const float* k_weight,
                                         const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len, int64_t hq,
                                         int64_t hkv, int64_t d, float w_offset, float eps, void* out, int64_t out_stride,
                                         float* rstd, int dtype, gmlm_stream_t stream) {
  return rope_fwd("qknorm_rope_d256_fwd", qkv, qkv_stride, q_weight, k_weight, cos_sin, max_len, tokens, seq_len, false, nullptr, hq,
                  hkv, d, w_offset, eps, out, out_stride, rstd, dtype, stream);
}

extern "C" int gmlm_qknorm_rope_d256_pos_fwd(const void* qkv, int64_t qkv_stride, const float* q_weight, const float* k_weight,
                                             const float* cos_sin, int64_t max_len, int64_t tokens, const int32_t* pos_ids,
                                             int64_t hq, int64_t hkv, int64_t d, float w_offset, float eps, void* out,
                                             int64_t out_stride, float* rstd, int dtype, gmlm_stream_t stream) {
  return rope_fwd("qknorm_rope_d256_pos_fwd", qkv, qkv_stride, q_weight, k_weight, cos_sin, max_len, tokens, 1, true, pos_ids, hq, hkv,
                  d, w_offset, eps, out, out_stride, rstd, dtype, stream);
}

extern "C" size_t gmlm_qknorm_rope_d256_bwd_workspace_bytes(int64_t tokens, int64_t hq, int64_t hkv, int dtype) {
  return rope_bwd_ws(tokens, hq, hkv, dtype);
}

extern "C" int gmlm_qknorm_rope_d256_bwd(void* dqkv, int64_t dqkv_stride, const void* qkv, int64_t qkv_stride, const float* q_weight,
                                         const float* k_weight, const float* cos_sin, int64_t max_len, const float* rstd,
                                         int64_t tokens, int64_t seq_len, int64_t hq, int64_t hkv, int64_t d, float w_offset,
                                         float* dq_weight, float* dk_weight, int dtype, void* workspace, size_t workspace_bytes,
                                         gmlm_stream_t stream) {
  return rope_bwd("qknorm_rope_d256_bwd", dqkv, dqkv_stride, qkv, qkv_stride, q_weight, k_weight, cos_sin, max_len, rstd, tokens,
                  seq_len, false, nullptr, hq, hkv, d, w_offset, dq_weight, dk_weight, dtype, workspace, workspace_bytes, stream);
}

extern "C" int gmlm_qknorm_rope_d256_pos_bwd(void* dqkv, int64_t dqkv_stride, const void* qkv, int64_t qkv_stride,
                                             const float* q_weight, const float* k_weight, const float* cos_sin, int64_t max_len,
                                             const float* rstd, int64_t tokens, const int32_t* pos_ids, int64_t hq, int64_t hkv,
                                             int64_t d, float w_offset, float* dq_weight, float* dk_weight, int dtype,
                                             void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  return rope_bwd("qknorm_rope_d256_pos_bwd", dqkv, dqkv_stride, qkv, qkv_stride, q_weight, k_weight, cos_sin, max_len, rstd, tokens, 1,
                  true, pos_ids, hq, hkv, d, w_offset, dq_weight, dk_weight, dtype, workspace, workspace_bytes, stream);
}

extern "C" int gmlm_geglu_tanh_fwd(const void* gate_up, int64_t rows, int64_t inter, void* y, int dtype, gmlm_stream_t stream) {
  static const char* who = "geglu_tanh_fwd";
  int rc = glu_check(who, rows, inter, dtype);
  if (rc != GMLM_OK) return rc;
  if (rows == 0) return GMLM_OK;
  GMLM_REQUIRE(gate_up && y && aligned16(gate_up) && aligned16(y), "%s: null or not 16-byte aligned pointer", who);
  hipStream_t st = as_stream(stream);
  const int v = dtype == GMLM_F32 ? 4 : 8;
  const int grid = grid_cap(cdiv(rows * (inter / v), 256), 8192);
  if (dtype == GMLM_BF16) geglu_tanh_fwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)gate_up, rows, inter, (bf16_t*)y);
  else geglu_tanh_fwd_kernel<float><<<grid, 256, 0, st>>>((const float*)gate_up, rows, inter, (float*)y);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" int gmlm_geglu_tanh_bwd(const void* dy, const void* gate_up, int64_t rows, int64_t inter, void* dgate_up, int dtype,
                                   gmlm_stream_t stream) {
  static const char* who = "geglu_tanh_bwd";
  int rc = glu_check(who, rows, inter, dtype);
  if (rc != GMLM_OK) return rc;
  if (rows == 0) return GMLM_OK;
  GMLM_REQUIRE(dy && gate_up && dgate_up && aligned16(dy) && aligned16(gate_up) && aligned16(dgate_up),
               "%s: null or not 16-byte aligned pointer", who);
  hipStream_t st = as_stream(stream);
  const int v = dtype == GMLM_F32 ? 4 : 8;
  const int grid = grid_cap(cdiv(rows * (inter / v), 256), 8192);
  if (dtype == GMLM_BF16) geglu_tanh_bwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)dy, (const bf16_t*)gate_up, rows, inter, (bf16_t*)dgate_up);
  else geglu_tanh_bwd_kernel<float><<<grid, 256, 0, st>>>((const float*)dy, (const float*)gate_up, rows, inter, (float*)dgate_up);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
