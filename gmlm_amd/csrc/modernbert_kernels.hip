// Row kernels of a ModernBERT text encoder (hf:modeling_modernbert.py; C ABI in include/gmlm_hip_modernbert.h): residual add +
// LayerNorm that also returns the residual stream, the rotate-half rotary embedding at head dim 64 in place on a fused
// [q | k | v] row block, and the GeGLU product.  bf16 or fp32 storage, fp32 arithmetic, ONE rounding on store.  HBM-bound
// streaming kernels; every reduction across rows runs in a fixed order (col_reduce): no atomics, identical calls give
// identical bits.  The kernels live in namespace gmlm::mbert; their bodies, shared with the RMSNorm / SwiGLU siblings of
// decoder_kernels.hip, are in row_kernels.hpp.
#include "row_kernels.hpp"
#include "../../include/gmlm_hip_modernbert.h"

namespace gmlm {
namespace mbert {

// add + LayerNorm (add_norm_*_body with LnStat):  s = a + b (b optional) stored as T;  y = (s - mean) * rstd * gamma (+ beta);
// mean[r], rstd[r] saved in fp32
template <typename T, int CH>
__global__ __launch_bounds__(256) void add_ln_fwd_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         int64_t rows, int f, float eps, T* __restrict__ s_out,
                                                         T* __restrict__ y, float* __restrict__ mean_o, float* __restrict__ rstd_o) {
  add_norm_fwd_body<T, CH, LnStat>(a, b, gamma, beta, rows, f, eps, s_out, y, mean_o, rstd_o);
}

template <typename T, int CH>
__global__ __launch_bounds__(256) void add_ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ dres,
                                                         const T* __restrict__ s, const float* __restrict__ gamma,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         int64_t rows, int f, T* __restrict__ ds) {
  add_norm_bwd_body<T, CH, LnStat>(dy, dres, s, gamma, mean, rstd, rows, f, ds);
}

// dgamma[c] = sum_r dy[r, c] * xhat[r, c] (k = 0), dbeta[c] = sum_r dy[r, c] (k = 1)
template <typename T, int K>
struct LnDwFn {
  const T* dy;
  const T* s;
  const float* mean;
  const float* rstd;
  int64_t f;
  __device__ __forceinline__ void operator()(int64_t r, int64_t c, float (&v)[K]) const {
    norm_dw_terms<T, K, true>(dy, s, mean, rstd, f, r, c, v);
  }
};

// Rotary embedding at head dim 64, in place (the rotary pieces: row_kernels.hpp).  A head row = 8 lanes (bf16) or 16 lanes
// (fp32) x 16 bytes.  Every lane reads its 16 bytes, exchanges, and writes the same 16 bytes back: in place without a hazard.
// INV: the backward.
constexpr int kRopeDim = 64;

template <typename T, bool INV>
__global__ __launch_bounds__(256) void rope64_kernel(T* __restrict__ qkv, int64_t stride, const float* __restrict__ cs,
                                                     int64_t tokens, int64_t seq_len, int nh /* 2 * h head rows per token */,
                                                     const int32_t* __restrict__ pos_ids, int64_t max_len) {
  constexpr int V = Store<T>::kVec, LPR = kRopeDim / V;
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int lr = (int)(gid % LPR);
  int64_t t;
  int hd;
  const bool live = head_row(gid / LPR, tokens * nh, nh, t, hd);
  const float* csr = rope_row<kRopeDim>(cs, t, seq_len, pos_ids, max_len);
  T* ptr = qkv + t * stride + (int64_t)hd * kRopeDim + lr * V;
  float x[V], c[V], sn[V], o[V];
  Store<T>::ldv(ptr, x);
  const int col = (lr * V) & 31;
  load_f32<V>(csr + col, c);
  load_f32<V>(csr + 32 + col, sn);
  const bool upper = lr >= LPR / 2;
#pragma unroll
  for (int v = 0; v < V; ++v) o[v] = rotate_half<LPR, INV>(x[v], c[v], sn[v], upper);
  if (live) Store<T>::stv(ptr, o);
}

// GeGLU: u = [gate | up] rows of 2 * I  ->  y = gelu(gate) * up  [rows, I]  (erf GELU)
template <typename T>
__global__ __launch_bounds__(256) void geglu_fwd_kernel(const T* __restrict__ u, int64_t rows, int64_t inter, T* __restrict__ y) {
  glu_fwd_body<T, GeluAct>(u, rows, inter, y);
}

template <typename T>
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ u, int64_t rows,
                                                        int64_t inter, T* __restrict__ du) {
  glu_bwd_body<T, GeluAct>(dy, u, rows, inter, du);
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

template <bool INV>
static int rope64(const char* who, void* qkv, int64_t stride, const float* cos_sin, int64_t max_len, int64_t tokens,
                  int64_t seq_len, const int32_t* pos_ids, int64_t h, int64_t d, int dtype, gmlm_stream_t stream) {
  int rc = rope_sizes(who, kRopeDim, stride, stride, 0, tokens, seq_len, pos_ids != nullptr, max_len, h, h, d, dtype);   // in place: one row block
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
  int rc = glu_check(who, rows, inter, dtype);
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
  int rc = glu_check(who, rows, inter, dtype);
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
