// Row kernels of a ModernBERT text encoder (hf:modeling_modernbert.py; C ABI in include/gmlm_hip_modernbert.h): residual add +
// LayerNorm that also returns the residual stream, the rotate-half rotary embedding at head dim 64 in place on a fused
// [q | k | v] row block, and the GeGLU product.  bf16 or fp32 storage, fp32 arithmetic, ONE rounding on store.  HBM-bound
// streaming kernels; every reduction across rows runs in a fixed order (col_reduce): no atomics, identical calls give
// identical bits.  The kernels live in namespace gmlm::mbert; the shapes follow their RMSNorm / SwiGLU siblings of
// decoder_kernels.hip.
#include "colreduce.hpp"
#include "../../include/gmlm_hip_modernbert.h"

namespace gmlm {
namespace mbert {

template <int LPR>
__device__ __forceinline__ float lanes_sum(float v) {
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int V>
__device__ __forceinline__ void load_f32(const float* __restrict__ p, float (&o)[V]) {
#pragma unroll
  for (int v = 0; v < V; v += 4) {
    const float4 t = *reinterpret_cast<const float4*>(p + v);
    o[v] = t.x; o[v + 1] = t.y; o[v + 2] = t.z; o[v + 3] = t.w;
  }
}

// the value a store of `x` as T leaves in memory: the statistics are taken over the ROUNDED sum, which is what every later
// kernel reads back and what the reference normalises in its bf16 run
template <typename T> __device__ __forceinline__ float rounded(float x);
template <> __device__ __forceinline__ float rounded<float>(float x) { return x; }
template <> __device__ __forceinline__ float rounded<bf16_t>(float x) { return bf16_to_f32(f32_to_bf16(x)); }

// ------------------------------------------------------------------------------------------------
// add + LayerNorm.  One wave per row, CH 16-byte chunks per lane (f <= 64 * CH * V), the row stays in registers.
//   s = a + b (b optional) stored as T;  y = (s - mean) * rstd * gamma (+ beta);  mean[r], rstd[r] saved in fp32
// Two passes over the registers: the mean first, then the sum of squared deviations (no E[x^2] - mean^2 cancellation).
// ------------------------------------------------------------------------------------------------
template <typename T, int CH>
__global__ __launch_bounds__(256) void add_ln_fwd_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         int64_t rows, int f, float eps, T* __restrict__ s_out,
                                                         T* __restrict__ y, float* __restrict__ mean_o, float* __restrict__ rstd_o) {
  constexpr int V = Store<T>::kVec;
  const int lane = threadIdx.x & 63, nch = f / V;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                                   // wave-uniform; no barrier in this kernel
  float z[CH][V];
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      const int64_t off = r * f + (int64_t)ch * V;
      Store<T>::ldv(a + off, z[c]);
      if (b) {
        float t[V];
        Store<T>::ldv(b + off, t);
#pragma unroll
        for (int v = 0; v < V; ++v) z[c][v] = rounded<T>(z[c][v] + t[v]);
        Store<T>::stv(s_out + off, z[c]);
      }
#pragma unroll
      for (int v = 0; v < V; ++v) sum += z[c][v];
    }
  }
  const float mu = lanes_sum<64>(sum) / (float)f;
  float sq = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (c * 64 + lane < nch) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const float dlt = z[c][v] - mu;
        sq = fmaf(dlt, dlt, sq);
      }
    }
  }
  const float rs = 1.f / sqrtf(lanes_sum<64>(sq) / (float)f + eps);
  if (lane == 0) { mean_o[r] = mu; rstd_o[r] = rs; }
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      float gv[V], o[V];
      load_f32<V>(gamma + ch * V, gv);
#pragma unroll
      for (int v = 0; v < V; ++v) o[v] = (z[c][v] - mu) * rs * gv[v];
      if (beta) {
        float bv[V];
        load_f32<V>(beta + ch * V, bv);
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] += bv[v];
      }
      Store<T>::stv(y + r * f + (int64_t)ch * V, o);
    }
  }
}

// ds = dres (optional: the gradient arriving on the residual stream) + rstd * (g - mean(g) - xhat * mean(g * xhat)),
// g = dy * gamma, xhat = (s - mean) * rstd.  The gradient of a AND of b is ds.
template <typename T, int CH>
__global__ __launch_bounds__(256) void add_ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ dres,
                                                         const T* __restrict__ s, const float* __restrict__ gamma,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         int64_t rows, int f, T* __restrict__ ds) {
  constexpr int V = Store<T>::kVec;
  const int lane = threadIdx.x & 63, nch = f / V;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float mu = mean[r], rs = rstd[r];
  float g[CH][V], xh[CH][V];
  float sg = 0.f, dot = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      const int64_t off = r * f + (int64_t)ch * V;
      float gv[V];
      Store<T>::ldv(dy + off, g[c]);
      Store<T>::ldv(s + off, xh[c]);
      load_f32<V>(gamma + ch * V, gv);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        g[c][v] *= gv[v];
        xh[c][v] = (xh[c][v] - mu) * rs;
        sg += g[c][v];
        dot += g[c][v] * xh[c][v];
      }
    }
  }
  const float m1 = lanes_sum<64>(sg) / (float)f, m2 = lanes_sum<64>(dot) / (float)f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      const int64_t off = r * f + (int64_t)ch * V;
      float o[V];
#pragma unroll
      for (int v = 0; v < V; ++v) o[v] = rs * (g[c][v] - m1 - xh[c][v] * m2);
      if (dres) {
        float t[V];
        Store<T>::ldv(dres + off, t);
#pragma unroll
        for (int v = 0; v < V; ++v) o[v] += t[v];
      }
      Store<T>::stv(ds + off, o);
    }
  }
}

// dgamma[c] = sum_r dy[r, c] * xhat[r, c] (k = 0), dbeta[c] = sum_r dy[r, c] (k = 1)  (col_reduce: fixed order)
template <typename T, int K>
struct LnDwFn {
  const T* dy;
  const T* s;
  const float* mean;
  const float* rstd;
  int64_t f;
  __device__ __forceinline__ void operator()(int64_t r, int64_t c, float (&v)[K]) const {
    const float g = Store<T>::ld(dy + r * f + c);
    v[0] = g * ((Store<T>::ld(s + r * f + c) - mean[r]) * rstd[r]);
    if constexpr (K == 2) v[1] = g;
  }
};

// ------------------------------------------------------------------------------------------------
// Rotary embedding at head dim 64, in place.  A head row of 64 elements = LPR lanes x 16 bytes (8 lanes bf16, 16 lanes fp32);
// element i pairs with i + 32, i.e. lane j with lane j ^ (LPR / 2): one cross-lane exchange, no LDS.  Every lane reads its 16
// bytes, exchanges, and writes the same 16 bytes back: in place without a hazard.
//   forward: out[i] = x[i] cos[i] - x[i + 32] sin[i],  out[i + 32] = x[i + 32] cos[i] + x[i] sin[i]
//   INV (backward): the transposed = inverse rotation, the same with sin negated
// cs: fp32 [max_len, 2, 32] (cos row, then sin row) of the token's position: row % seq_len (padded [b, seq_len] layout), or,
// when pos_ids is given (packed rows), pos_ids[row] clamped into [0, max_len) so that no position reads outside the table.
// ------------------------------------------------------------------------------------------------
constexpr int kRopeDim = 64;

template <typename T, bool INV>
__global__ __launch_bounds__(256) void rope64_kernel(T* __restrict__ qkv, int64_t stride, const float* __restrict__ cs,
                                                     int64_t tokens, int64_t seq_len, int nh /* 2 * h head rows per token */,
                                                     const int32_t* __restrict__ pos_ids, int64_t max_len) {
  constexpr int V = Store<T>::kVec, LPR = kRopeDim / V;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lr = (int)(gid % LPR);
  const int64_t item = gid / LPR;
  const bool live = item < tokens * nh;                    // whole LPR-lane groups are live or not
  const int64_t t = live ? item / nh : 0;
  const int hd = live ? (int)(item % nh) : 0;
  int64_t pos;
  if (pos_ids) {                                           // a kernel argument: uniform over the grid
    pos = pos_ids[t];
    pos = pos < 0 ? 0 : (pos >= max_len ? max_len - 1 : pos);
  } else {
    pos = t % seq_len;
  }
  T* ptr = qkv + t * stride + (int64_t)hd * kRopeDim + lr * V;
  float x[V], c[V], sn[V], o[V];
  Store<T>::ldv(ptr, x);
  const int col = (lr * V) & 31;
  load_f32<V>(cs + pos * 64 + col, c);
  load_f32<V>(cs + pos * 64 + 32 + col, sn);
  const bool upper = lr >= LPR / 2;
  const bool plus = upper != INV;                          // forward: the upper half adds x[i] sin, the lower subtracts x[i + 32] sin
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const float other = __shfl_xor(x[v], LPR / 2, 64);     // every lane of the wave takes part
    o[v] = plus ? fmaf(other, sn[v], x[v] * c[v]) : fmaf(-other, sn[v], x[v] * c[v]);
  }
  if (live) Store<T>::stv(ptr, o);
}

// ------------------------------------------------------------------------------------------------
// GeGLU: u = [gate | up] rows of 2 * I  ->  y = gelu(gate) * up  [rows, I]  (erf GELU: common.hpp)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void geglu_fwd_kernel(const T* __restrict__ u, int64_t rows, int64_t inter, T* __restrict__ y) {
  constexpr int V = Store<T>::kVec;
  const int64_t cpr = inter / V, total = rows * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cpr, c = (i % cpr) * V;
    float g[V], up[V], o[V];
    Store<T>::ldv(u + r * 2 * inter + c, g);
    Store<T>::ldv(u + r * 2 * inter + inter + c, up);
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = gelu_fwd_t<T>(g[v]) * up[v];
    Store<T>::stv(y + r * inter + c, o);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ u, int64_t rows,
                                                        int64_t inter, T* __restrict__ du) {
  constexpr int V = Store<T>::kVec;
  const int64_t cpr = inter / V, total = rows * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cpr, c = (i % cpr) * V;
    float g[V], up[V], d[V], dg[V], dup[V];
    Store<T>::ldv(u + r * 2 * inter + c, g);
    Store<T>::ldv(u + r * 2 * inter + inter + c, up);
    Store<T>::ldv(dy + r * inter + c, d);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      dup[v] = d[v] * gelu_fwd_t<T>(g[v]);
      dg[v] = d[v] * up[v] * gelu_grad_t<T>(g[v]);
    }
    Store<T>::stv(du + r * 2 * inter + c, dg);
    Store<T>::stv(du + r * 2 * inter + inter + c, dup);
  }
}

// ---- host ----------------------------------------------------------------------------------------
static int ln_check(const char* who, int64_t rows, int64_t f, int dtype) {
  GMLM_REQUIRE(dtype == GMLM_F32 || dtype == GMLM_BF16, "%s: unsupported dtype", who);
  const int v = dtype == GMLM_F32 ? 4 : 8;
  GMLM_REQUIRE(rows >= 0 && f > 0 && f <= GMLM_ADD_LAYERNORM_MAX_F && f % v == 0, "%s: row width %ld must be a multiple of %d, at most %d",
               who, (long)f, v, GMLM_ADD_LAYERNORM_MAX_F);
  GMLM_REQUIRE(cdiv(rows, 4) < ((int64_t)1 << 31), "%s: too many rows", who);
  return GMLM_OK;
}

// smallest instantiated chunk count covering f / V chunks over 64 lanes; WIDEST = the count f = 4096 needs (8 chunks of
// 8 bf16, 16 chunks of 4 fp32), so that no instantiation exists that cannot be launched
#define GMLM_LN_DISPATCH(T, WIDEST, KERNEL, ...)                                              \
  do {                                                                                        \
    const int need_ = (int)cdiv(f / Store<T>::kVec, 64);                                      \
    const unsigned grid_ = (unsigned)cdiv(rows, 4);                                           \
    if (need_ <= 2) KERNEL<T, 2><<<grid_, 256, 0, st>>>(__VA_ARGS__);                         \
    else if (need_ <= 4) KERNEL<T, 4><<<grid_, 256, 0, st>>>(__VA_ARGS__);                    \
    else if (need_ <= 8) KERNEL<T, 8><<<grid_, 256, 0, st>>>(__VA_ARGS__);                    \
    else KERNEL<T, WIDEST><<<grid_, 256, 0, st>>>(__VA_ARGS__);                               \
  } while (0)

// sizes first, pointers second: a call with no token returns GMLM_OK in between.  seq_len = 0 is the padded layout [b, 0]: it
// has no token, and only then is it accepted; with pos_ids the sequence length is not used
static int rope_sizes(const char* who, int64_t stride, int64_t tokens, int64_t seq_len, bool by_pos, int64_t max_len, int64_t h,
                      int64_t d, int dtype) {
  GMLM_REQUIRE(dtype == GMLM_F32 || dtype == GMLM_BF16, "%s: unsupported dtype", who);
  GMLM_REQUIRE(d == 64, "%s: head dim %ld not supported (this entry point takes 64)", who, (long)d);
  GMLM_REQUIRE(tokens >= 0 && h > 0 && h < 2048, "%s: bad sizes", who);
  GMLM_REQUIRE(max_len > 0, "%s: empty cos / sin table", who);
  if (!by_pos) {
    GMLM_REQUIRE(seq_len >= 0 && seq_len <= max_len, "%s: sequence length %ld exceeds the %ld rows of the cos / sin table", who,
                 (long)seq_len, (long)max_len);
    GMLM_REQUIRE(seq_len > 0 || tokens == 0, "%s: %ld tokens in sequences of length 0", who, (long)tokens);
  }
  const int v = dtype == GMLM_F32 ? 4 : 8;
  GMLM_REQUIRE(stride >= 3 * h * 64 && stride % v == 0, "%s: qkv row stride %ld must be >= %ld and a multiple of %d", who,
               (long)stride, (long)(3 * h * 64), v);
  GMLM_REQUIRE(tokens * 2 * h < ((int64_t)1 << 34), "%s: too many head rows", who);
  return GMLM_OK;
}

template <bool INV>
static int rope64(const char* who, void* qkv, int64_t stride, const float* cos_sin, int64_t max_len, int64_t tokens,
                  int64_t seq_len, const int32_t* pos_ids, int64_t h, int64_t d, int dtype, gmlm_stream_t stream) {
  int rc = rope_sizes(who, stride, tokens, seq_len, pos_ids != nullptr, max_len, h, d, dtype);
  if (rc != GMLM_OK) return rc;
  if (tokens == 0) return GMLM_OK;
  GMLM_REQUIRE(qkv && aligned16(qkv), "%s: null or not 16-byte aligned pointer", who);
  GMLM_REQUIRE(cos_sin && aligned16(cos_sin), "%s: null or misaligned cos / sin table", who);
  hipStream_t st = as_stream(stream);
  const int64_t items = tokens * 2 * h;
  if (dtype == GMLM_BF16)
    rope64_kernel<bf16_t, INV><<<(unsigned)cdiv(items * 8, 256), 256, 0, st>>>((bf16_t*)qkv, stride, cos_sin, tokens, seq_len,
                                                                              (int)(2 * h), pos_ids, max_len);
  else
    rope64_kernel<float, INV><<<(unsigned)cdiv(items * 16, 256), 256, 0, st>>>((float*)qkv, stride, cos_sin, tokens, seq_len,
                                                                              (int)(2 * h), pos_ids, max_len);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

static int geglu_check(const char* who, int64_t rows, int64_t inter, int dtype) {
  GMLM_REQUIRE(dtype == GMLM_F32 || dtype == GMLM_BF16, "%s: unsupported dtype", who);
  const int v = dtype == GMLM_F32 ? 4 : 8;
  GMLM_REQUIRE(rows >= 0 && inter > 0 && inter % v == 0, "%s: width %ld must be a multiple of %d", who, (long)inter, v);
  return GMLM_OK;
}

}  // namespace mbert
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::mbert;

extern "C" int gmlm_add_layernorm_fwd(const void* a, const void* b, const float* gamma, const float* beta, int64_t rows, int64_t f,
                                      float eps, void* s, void* y, float* mean, float* rstd, int dtype, gmlm_stream_t stream) {
  static const char* who = "add_layernorm_fwd";
  int rc = ln_check(who, rows, f, dtype);
  if (rc != GMLM_OK) return rc;
  if (rows == 0) return GMLM_OK;
  GMLM_REQUIRE(a && gamma && y && mean && rstd && aligned16(a) && aligned16(gamma) && aligned16(beta) && aligned16(y) && aligned16(b) &&
                   aligned16(s), "%s: null or not 16-byte aligned pointer", who);
  GMLM_REQUIRE(!b == !s, "%s: s (the stored sum) is given exactly when b is", who);
  hipStream_t st = as_stream(stream);
  if (dtype == GMLM_BF16)
    GMLM_LN_DISPATCH(bf16_t, 8, add_ln_fwd_kernel, (const bf16_t*)a, (const bf16_t*)b, gamma, beta, rows, (int)f, eps, (bf16_t*)s,
                     (bf16_t*)y, mean, rstd);
  else
    GMLM_LN_DISPATCH(float, 16, add_ln_fwd_kernel, (const float*)a, (const float*)b, gamma, beta, rows, (int)f, eps, (float*)s, (float*)y,
                     mean, rstd);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_add_layernorm_bwd_workspace_bytes(int64_t rows, int64_t f) { return col_reduce_workspace_bytes(rows, f, 2); }

extern "C" int gmlm_add_layernorm_bwd(const void* dy, const void* dres, const void* s, const float* gamma, const float* mean,
                                      const float* rstd, int64_t rows, int64_t f, void* ds, float* dgamma, float* dbeta, int dtype,
                                      void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "add_layernorm_bwd";
  int rc = ln_check(who, rows, f, dtype);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(dgamma && (!dbeta || dbeta == dgamma + f), "%s: null dgamma, or dgamma | dbeta are not one fp32 [2, f] buffer", who);
  if (rows > 0 && (!workspace || workspace_bytes < gmlm_add_layernorm_bwd_workspace_bytes(rows, f))) {   // before any launch
    set_error("%s: workspace too small", who);
    return GMLM_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (rows > 0) {
    GMLM_REQUIRE(dy && s && gamma && mean && rstd && ds && aligned16(dy) && aligned16(s) && aligned16(gamma) && aligned16(ds) &&
                     aligned16(dres), "%s: null or not 16-byte aligned pointer", who);
    if (dtype == GMLM_BF16)
      GMLM_LN_DISPATCH(bf16_t, 8, add_ln_bwd_kernel, (const bf16_t*)dy, (const bf16_t*)dres, (const bf16_t*)s, gamma, mean, rstd, rows,
                       (int)f, (bf16_t*)ds);
    else
      GMLM_LN_DISPATCH(float, 16, add_ln_bwd_kernel, (const float*)dy, (const float*)dres, (const float*)s, gamma, mean, rstd, rows, (int)f,
                       (float*)ds);
    GMLM_LAUNCH_CHECK();
  }
  if (dtype == GMLM_BF16) {
    const bf16_t *dyt = (const bf16_t*)dy, *st_ = (const bf16_t*)s;
    if (dbeta) return col_reduce<2>(rows, f, LnDwFn<bf16_t, 2>{dyt, st_, mean, rstd, f}, dgamma, workspace, workspace_bytes, st);
    return col_reduce<1>(rows, f, LnDwFn<bf16_t, 1>{dyt, st_, mean, rstd, f}, dgamma, workspace, workspace_bytes, st);
  }
  const float *dyt = (const float*)dy, *st_ = (const float*)s;
  if (dbeta) return col_reduce<2>(rows, f, LnDwFn<float, 2>{dyt, st_, mean, rstd, f}, dgamma, workspace, workspace_bytes, st);
  return col_reduce<1>(rows, f, LnDwFn<float, 1>{dyt, st_, mean, rstd, f}, dgamma, workspace, workspace_bytes, st);
}

extern "C" int gmlm_rope64_fwd(void* qkv, int64_t qkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len,
                               const int32_t* pos_ids, int64_t h, int64_t d, int dtype, gmlm_stream_t stream) {
  return rope64<false>("rope64_fwd", qkv, qkv_stride, cos_sin, max_len, tokens, seq_len, pos_ids, h, d, dtype, stream);
}

extern "C" int gmlm_rope64_bwd(void* dqkv, int64_t dqkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens,
                               int64_t seq_len, const int32_t* pos_ids, int64_t h, int64_t d, int dtype, gmlm_stream_t stream) {
  return rope64<true>("rope64_bwd", dqkv, dqkv_stride, cos_sin, max_len, tokens, seq_len, pos_ids, h, d, dtype, stream);
}

extern "C" int gmlm_geglu_fwd(const void* u, int64_t rows, int64_t inter, void* y, int dtype, gmlm_stream_t stream) {
  static const char* who = "geglu_fwd";
  int rc = geglu_check(who, rows, inter, dtype);
  if (rc != GMLM_OK) return rc;
  if (rows == 0) return GMLM_OK;
  GMLM_REQUIRE(u && y && aligned16(u) && aligned16(y), "%s: null or not 16-byte aligned pointer", who);
  hipStream_t st = as_stream(stream);
  const int v = dtype == GMLM_F32 ? 4 : 8;
  const int grid = grid_cap(cdiv(rows * (inter / v), 256), 8192);
  if (dtype == GMLM_BF16) geglu_fwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)u, rows, inter, (bf16_t*)y);
  else geglu_fwd_kernel<float><<<grid, 256, 0, st>>>((const float*)u, rows, inter, (float*)y);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" int gmlm_geglu_bwd(const void* dy, const void* u, int64_t rows, int64_t inter, void* du, int dtype, gmlm_stream_t stream) {
  static const char* who = "geglu_bwd";
  int rc = geglu_check(who, rows, inter, dtype);
  if (rc != GMLM_OK) return rc;
  if (rows == 0) return GMLM_OK;
  GMLM_REQUIRE(dy && u && du && aligned16(dy) && aligned16(u) && aligned16(du), "%s: null or not 16-byte aligned pointer", who);
  hipStream_t st = as_stream(stream);
  const int v = dtype == GMLM_F32 ? 4 : 8;
  const int grid = grid_cap(cdiv(rows * (inter / v), 256), 8192);
  if (dtype == GMLM_BF16) geglu_bwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)dy, (const bf16_t*)u, rows, inter, (bf16_t*)du);
  else geglu_bwd_kernel<float><<<grid, 256, 0, st>>>((const float*)dy, (const float*)u, rows, inter, (float*)du);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
