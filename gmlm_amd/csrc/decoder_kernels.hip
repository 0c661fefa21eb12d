// Row kernels of the pre-norm decoder-style text encoders (Qwen3 geometry, hf:modeling_qwen3.py): residual add + RMSNorm,
// per-head RMSNorm of Q / K followed by the rotate-half position rotation, and the SwiGLU product.  bf16 or fp32 storage, fp32
// arithmetic, ONE rounding on store.  HBM-bound streaming kernels; every reduction across rows runs in a fixed order
// (block partials + rows_sum_kernel, or col_reduce): no atomics, identical calls give identical bits.  The kernel bodies
// shared with modernbert_kernels.hip are in row_kernels.hpp.
#include "row_kernels.hpp"

namespace gmlm {

// add + RMSNorm (add_norm_*_body with RmsStat):  s = a + b (b optional) stored as T;  y = s * rsqrt(mean(s^2) + eps) * w;
// rstd[r] saved in fp32
template <typename T, int CH>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                           const float* __restrict__ w, int64_t rows, int f, float eps,
                                                           T* __restrict__ s_out, T* __restrict__ y, float* __restrict__ rstd_o) {
  add_norm_fwd_body<T, CH, RmsStat>(a, b, w, nullptr, rows, f, eps, s_out, y, nullptr, rstd_o);
}

template <typename T, int CH>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ dres,
                                                           const T* __restrict__ s, const float* __restrict__ w,
                                                           const float* __restrict__ rstd, int64_t rows, int f,
                                                           T* __restrict__ ds) {
  add_norm_bwd_body<T, CH, RmsStat>(dy, dres, s, w, nullptr, rstd, rows, f, ds);
}

// dw[c] = sum_r dy[r, c] * s[r, c] * rstd[r]
template <typename T>
struct RmsDwFn {
  const T* dy;
  const T* s;
  const float* rstd;
  int64_t f;
  __device__ __forceinline__ void operator()(int64_t r, int64_t c, float (&v)[1]) const {
    norm_dw_terms<T, 1, false>(dy, s, nullptr, rstd, f, r, c, v);
  }
};

// ------------------------------------------------------------------------------------------------
// Q / K head norm + rotary embedding (the rotary pieces: row_kernels.hpp).  A head row of 128 elements = 16 lanes (bf16) or
// 32 lanes (fp32) x 16 bytes.
//   n = x * rsqrt(mean(x^2) + eps) * w;   out[i] = n[i] cos[i] - n[i + 64] sin[i],  out[i + 64] = n[i + 64] cos[i] + n[i] sin[i]
// ------------------------------------------------------------------------------------------------
constexpr int kHeadDim = 128;

template <typename T>
__global__ __launch_bounds__(256) void qknorm_rope_fwd_kernel(const T* __restrict__ qkv, int64_t in_stride,
                                                               const float* __restrict__ qw, const float* __restrict__ kw,
                                                               const float* __restrict__ cs, int64_t tokens, int64_t seq_len,
                                                               int hq, int hkv, float eps, T* __restrict__ out,
                                                               int64_t out_stride, float* __restrict__ rstd_o,
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
  const int col = (lr * V) & 63;
  const float* csr = rope_row<kHeadDim>(cs, t, seq_len, pos_ids, max_len);
  load_f32<V>(csr + col, c);
  load_f32<V>(csr + 64 + col, sn);
  float sq = 0.f;
#pragma unroll
  for (int v = 0; v < V; ++v) sq += x[v] * x[v];
  const float rs = 1.f / sqrtf(lanes_sum<LPR>(sq) / (float)kHeadDim + eps);
  const bool upper = lr >= LPR / 2;
  float o[V];
#pragma unroll
  for (int v = 0; v < V; ++v) o[v] = rotate_half<LPR, false>(x[v] * rs * wv[v], c[v], sn[v], upper);
  if (live) {
    Store<T>::stv(out + t * out_stride + (int64_t)hd * kHeadDim + lr * V, o);
    if (lr == 0) rstd_o[item] = rs;
  }
}

// Backward, in place on the leading (hq + hkv) * 128 columns of the fused dqkv rows: inverse rotation, then the RMSNorm
// backward.  Weight gradients: every thread keeps the sums of its fixed columns over its grid-stride rows (Q and K heads
// apart), the block adds its row groups through LDS in a fixed order and writes ONE partial row [2][128]; rows_sum_kernel
// adds the blocks.
template <typename T>
__global__ __launch_bounds__(256) void qknorm_rope_bwd_kernel(T* __restrict__ dqkv, int64_t d_stride, const T* __restrict__ qkv,
                                                               int64_t in_stride, const float* __restrict__ qw,
                                                               const float* __restrict__ kw, const float* __restrict__ cs,
                                                               const float* __restrict__ rstd, int64_t tokens, int64_t seq_len,
                                                               int hq, int hkv, float* __restrict__ partial,
                                                               const int32_t* __restrict__ pos_ids, int64_t max_len) {
  constexpr int V = Store<T>::kVec, LPR = kHeadDim / V, RPB = 256 / LPR;
  __shared__ float red[RPB][2][kHeadDim];
  const int lr = threadIdx.x % LPR, grp = threadIdx.x / LPR, nh = hq + hkv;
  const int64_t items = tokens * nh;
  const int col = (lr * V) & 63;
  const bool upper = lr >= LPR / 2;
  float wq[V], wk[V], accq[V], acck[V];
  load_f32<V>(qw + lr * V, wq);
  load_f32<V>(kw + lr * V, wk);
#pragma unroll
  for (int v = 0; v < V; ++v) { accq[v] = 0.f; acck[v] = 0.f; }
  // every lane group runs the same number of iterations (the shuffles need all lanes of a wave)
  const int64_t per_pass = (int64_t)gridDim.x * RPB;
  const int64_t iters = (items + per_pass - 1) / per_pass;
  for (int64_t it = 0; it < iters; ++it) {
    const int64_t item = (it * gridDim.x + blockIdx.x) * RPB + grp;
    const bool live = item < items;                        // as head_row has it, for this kernel's own item order
    const int64_t t = live ? item / nh : 0;
    const int hd = live ? (int)(item % nh) : 0;
    const bool is_k = hd >= hq;
    float g[V], x[V], c[V], sn[V];
    T* dptr = dqkv + t * d_stride + (int64_t)hd * kHeadDim + lr * V;
    Store<T>::ldv(dptr, g);
    Store<T>::ldv(qkv + t * in_stride + (int64_t)hd * kHeadDim + lr * V, x);
    const float* csr = rope_row<kHeadDim>(cs, t, seq_len, pos_ids, max_len);
    load_f32<V>(csr + col, c);
    load_f32<V>(csr + 64 + col, sn);
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
  float sum = 0.f;
#pragma unroll
  for (int g = 0; g < RPB; ++g) sum += red[g][threadIdx.x >> 7][threadIdx.x & 127];
  partial[(int64_t)blockIdx.x * 256 + threadIdx.x] = sum;
}

// ------------------------------------------------------------------------------------------------
// SwiGLU: gu = [gate | up] rows of 2 * I  ->  y = silu(gate) * up  [rows, I]
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const T* __restrict__ gu, int64_t rows, int64_t inter, T* __restrict__ y) {
  glu_fwd_body<T, SiluAct>(gu, rows, inter, y);
}

template <typename T>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ gu, int64_t rows,
                                                          int64_t inter, T* __restrict__ dgu) {
  glu_bwd_body<T, SiluAct>(dy, gu, rows, inter, dgu);
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
#define GMLM_RMS_DISPATCH(T, WIDEST, KERNEL, ...)                                             \
  do {                                                                                        \
    const int need_ = (int)cdiv(f / Store<T>::kVec, 64);                                      \
    const unsigned grid_ = (unsigned)cdiv(rows, 4);                                           \
    if (need_ <= 2) KERNEL<T, 2><<<grid_, 256, 0, st>>>(__VA_ARGS__);                         \
    else if (need_ <= 4) KERNEL<T, 4><<<grid_, 256, 0, st>>>(__VA_ARGS__);                    \
    else if (need_ <= 8) KERNEL<T, 8><<<grid_, 256, 0, st>>>(__VA_ARGS__);                    \
    else KERNEL<T, WIDEST><<<grid_, 256, 0, st>>>(__VA_ARGS__);                               \
  } while (0)

constexpr int kRopeBwdMaxBlocks = 1024;
static int64_t rope_bwd_blocks(int64_t items, int dtype) {
  const int64_t rpb = dtype == GMLM_F32 ? 8 : 16;
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

}  // namespace gmlm

using namespace gmlm;

extern "C" int gmlm_add_rmsnorm_fwd(const void* a, const void* b, const float* w, int64_t rows, int64_t f, float eps, void* s,
                                    void* y, float* rstd, int dtype, gmlm_stream_t stream) {
  static const char* who = "add_rmsnorm_fwd";
  int rc = rms_check(who, rows, f, dtype);
  if (rc != GMLM_OK) return rc;
  if (rows == 0) return GMLM_OK;
  GMLM_REQUIRE(a && w && y && rstd && aligned16(a) && aligned16(w) && aligned16(y) && aligned16(b) && aligned16(s),
               "%s: null or not 16-byte aligned pointer", who);
  GMLM_REQUIRE(!b == !s, "%s: s (the stored sum) is given exactly when b is", who);
  hipStream_t st = as_stream(stream);
  if (dtype == GMLM_BF16)
    GMLM_RMS_DISPATCH(bf16_t, 8, rmsnorm_fwd_kernel, (const bf16_t*)a, (const bf16_t*)b, w, rows, (int)f, eps, (bf16_t*)s, (bf16_t*)y, rstd);
  else
    GMLM_RMS_DISPATCH(float, 16, rmsnorm_fwd_kernel, (const float*)a, (const float*)b, w, rows, (int)f, eps, (float*)s, (float*)y, rstd);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_add_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t f) { return col_reduce_workspace_bytes(rows, f, 1); }

extern "C" int gmlm_add_rmsnorm_bwd(const void* dy, const void* dres, const void* s, const float* w, const float* rstd,
                                    int64_t rows, int64_t f, void* ds, float* dw, int dtype, void* workspace,
                                    size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "add_rmsnorm_bwd";
  int rc = rms_check(who, rows, f, dtype);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(dw, "%s: null dw", who);
  if (rows > 0 && (!workspace || workspace_bytes < gmlm_add_rmsnorm_bwd_workspace_bytes(rows, f))) {   // before any launch
    set_error("%s: workspace too small", who);
    return GMLM_EWORKSPACE;
  }
  hipStream_t st = as_stream(stream);
  if (rows > 0) {
    GMLM_REQUIRE(dy && s && w && rstd && ds && aligned16(dy) && aligned16(s) && aligned16(w) && aligned16(ds) && aligned16(dres),
                 "%s: null or not 16-byte aligned pointer", who);
    if (dtype == GMLM_BF16)
      GMLM_RMS_DISPATCH(bf16_t, 8, rmsnorm_bwd_kernel, (const bf16_t*)dy, (const bf16_t*)dres, (const bf16_t*)s, w, rstd, rows, (int)f, (bf16_t*)ds);
    else
      GMLM_RMS_DISPATCH(float, 16, rmsnorm_bwd_kernel, (const float*)dy, (const float*)dres, (const float*)s, w, rstd, rows, (int)f, (float*)ds);
    GMLM_LAUNCH_CHECK();
  }
  if (dtype == GMLM_BF16)
    return col_reduce<1>(rows, f, RmsDwFn<bf16_t>{(const bf16_t*)dy, (const bf16_t*)s, rstd, f}, dw, workspace, workspace_bytes, st);
  return col_reduce<1>(rows, f, RmsDwFn<float>{(const float*)dy, (const float*)s, rstd, f}, dw, workspace, workspace_bytes, st);
}

// by_pos: position = pos_ids[row] (seq_len unused, passed as 1); else pos_ids is NULL and position = row % seq_len
static int rope_fwd(const char* who, const void* qkv, int64_t qkv_stride, const float* q_weight, const float* k_weight,
                    const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len, bool by_pos, const int32_t* pos_ids,
                    int64_t hq, int64_t hkv, int64_t d, float eps, void* out, int64_t out_stride, float* rstd, int dtype,
                    gmlm_stream_t stream) {
  int rc = rope_sizes(who, kHeadDim, qkv_stride, out_stride, (hq + hkv) * 128, tokens, seq_len, by_pos, max_len, hq, hkv, d, dtype);
  if (rc != GMLM_OK) return rc;
  if (tokens == 0) return GMLM_OK;
  if ((rc = rope_ptrs(who, qkv, out, q_weight, k_weight, cos_sin, rstd, by_pos, pos_ids)) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t items = tokens * (hq + hkv);
  if (dtype == GMLM_BF16)
    qknorm_rope_fwd_kernel<bf16_t><<<(unsigned)cdiv(items * 16, 256), 256, 0, st>>>((const bf16_t*)qkv, qkv_stride, q_weight, k_weight,
        cos_sin, tokens, seq_len, (int)hq, (int)hkv, eps, (bf16_t*)out, out_stride, rstd, pos_ids, max_len);
  else
    qknorm_rope_fwd_kernel<float><<<(unsigned)cdiv(items * 32, 256), 256, 0, st>>>((const float*)qkv, qkv_stride, q_weight, k_weight,
        cos_sin, tokens, seq_len, (int)hq, (int)hkv, eps, (float*)out, out_stride, rstd, pos_ids, max_len);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" int gmlm_qknorm_rope_fwd(const void* qkv, int64_t qkv_stride, const float* q_weight, const float* k_weight,
                                    const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len, int64_t hq,
                                    int64_t hkv, int64_t d, float eps, void* out, int64_t out_stride, float* rstd, int dtype,
                                    gmlm_stream_t stream) {
  return rope_fwd("qknorm_rope_fwd", qkv, qkv_stride, q_weight, k_weight, cos_sin, max_len, tokens, seq_len, false, nullptr, hq, hkv, d,
                  eps, out, out_stride, rstd, dtype, stream);
}

extern "C" int gmlm_qknorm_rope_pos_fwd(const void* qkv, int64_t qkv_stride, const float* q_weight, const float* k_weight,
                                        const float* cos_sin, int64_t max_len, int64_t tokens, const int32_t* pos_ids, int64_t hq,
                                        int64_t hkv, int64_t d, float eps, void* out, int64_t out_stride, float* rstd, int dtype,
                                        gmlm_stream_t stream) {
  return rope_fwd("qknorm_rope_pos_fwd", qkv, qkv_stride, q_weight, k_weight, cos_sin, max_len, tokens, 1, true, pos_ids, hq, hkv, d, eps,
                  out, out_stride, rstd, dtype, stream);
}

extern "C" size_t gmlm_qknorm_rope_bwd_workspace_bytes(int64_t tokens, int64_t hq, int64_t hkv, int dtype) {
  return (size_t)rope_bwd_blocks(tokens * (hq + hkv), dtype) * 256 * sizeof(float);
}

static int rope_bwd(const char* who, void* dqkv, int64_t dqkv_stride, const void* qkv, int64_t qkv_stride, const float* q_weight,
                    const float* k_weight, const float* cos_sin, int64_t max_len, const float* rstd, int64_t tokens,
                    int64_t seq_len, bool by_pos, const int32_t* pos_ids, int64_t hq, int64_t hkv, int64_t d, float* dq_weight,
                    float* dk_weight, int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  int rc = rope_sizes(who, kHeadDim, qkv_stride, dqkv_stride, (hq + hkv) * 128, tokens, seq_len, by_pos, max_len, hq, hkv, d, dtype);
  if (rc != GMLM_OK) return rc;
  // the one output a call with no token still has: zero weight gradients
  GMLM_REQUIRE(dq_weight && dk_weight && dk_weight == dq_weight + 128, "%s: dq_weight | dk_weight are one fp32 [2, 128] buffer", who);
  hipStream_t st = as_stream(stream);
  if (tokens == 0) {
    hipError_t e = zero_async(dq_weight, 256 * sizeof(float), st);
    if (e != hipSuccess) { set_error("%s: zero fill failed: %s", who, hipGetErrorString(e)); return GMLM_ELAUNCH; }
    return GMLM_OK;
  }
  if ((rc = rope_ptrs(who, qkv, dqkv, q_weight, k_weight, cos_sin, rstd, by_pos, pos_ids)) != GMLM_OK) return rc;
  if (!workspace || workspace_bytes < gmlm_qknorm_rope_bwd_workspace_bytes(tokens, hq, hkv, dtype)) {
    set_error("%s: workspace too small", who);
    return GMLM_EWORKSPACE;
  }
  const int nb = (int)rope_bwd_blocks(tokens * (hq + hkv), dtype);
  float* partial = static_cast<float*>(workspace);
  if (dtype == GMLM_BF16)
    qknorm_rope_bwd_kernel<bf16_t><<<nb, 256, 0, st>>>((bf16_t*)dqkv, dqkv_stride, (const bf16_t*)qkv, qkv_stride, q_weight, k_weight,
        cos_sin, rstd, tokens, seq_len, (int)hq, (int)hkv, partial, pos_ids, max_len);
  else
    qknorm_rope_bwd_kernel<float><<<nb, 256, 0, st>>>((float*)dqkv, dqkv_stride, (const float*)qkv, qkv_stride, q_weight, k_weight,
        cos_sin, rstd, tokens, seq_len, (int)hq, (int)hkv, partial, pos_ids, max_len);
  GMLM_LAUNCH_CHECK();
  rows_sum_kernel<<<8, 256, 0, st>>>(partial, nb, 256, dq_weight);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" int gmlm_qknorm_rope_bwd(void* dqkv, int64_t dqkv_stride, const void* qkv, int64_t qkv_stride, const float* q_weight,
                                    const float* k_weight, const float* cos_sin, int64_t max_len, const float* rstd,
                                    int64_t tokens, int64_t seq_len, int64_t hq, int64_t hkv, int64_t d, float* dq_weight,
                                    float* dk_weight, int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  return rope_bwd("qknorm_rope_bwd", dqkv, dqkv_stride, qkv, qkv_stride, q_weight, k_weight, cos_sin, max_len, rstd, tokens, seq_len,
                  false, nullptr, hq, hkv, d, dq_weight, dk_weight, dtype, workspace, workspace_bytes, stream);
}

extern "C" int gmlm_qknorm_rope_pos_bwd(void* dqkv, int64_t dqkv_stride, const void* qkv, int64_t qkv_stride,
                                        const float* q_weight, const float* k_weight, const float* cos_sin, int64_t max_len,
                                        const float* rstd, int64_t tokens, const int32_t* pos_ids, int64_t hq, int64_t hkv,
                                        int64_t d, float* dq_weight, float* dk_weight, int dtype, void* workspace,
                                        size_t workspace_bytes, gmlm_stream_t stream) {
  return rope_bwd("qknorm_rope_pos_bwd", dqkv, dqkv_stride, qkv, qkv_stride, q_weight, k_weight, cos_sin, max_len, rstd, tokens, 1, true,
                  pos_ids, hq, hkv, d, dq_weight, dk_weight, dtype, workspace, workspace_bytes, stream);
}

extern "C" int gmlm_swiglu_fwd(const void* gate_up, int64_t rows, int64_t inter, void* y, int dtype, gmlm_stream_t stream) {
  static const char* who = "swiglu_fwd";
  int rc = glu_check(who, rows, inter, dtype);
  if (rc != GMLM_OK) return rc;
  if (rows == 0) return GMLM_OK;
  GMLM_REQUIRE(gate_up && y && aligned16(gate_up) && aligned16(y), "%s: null or not 16-byte aligned pointer", who);
  hipStream_t st = as_stream(stream);
  const int v = dtype == GMLM_F32 ? 4 : 8;
  const int grid = grid_cap(cdiv(rows * (inter / v), 256), 8192);
  if (dtype == GMLM_BF16) swiglu_fwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)gate_up, rows, inter, (bf16_t*)y);
  else swiglu_fwd_kernel<float><<<grid, 256, 0, st>>>((const float*)gate_up, rows, inter, (float*)y);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" int gmlm_swiglu_bwd(const void* dy, const void* gate_up, int64_t rows, int64_t inter, void* dgate_up, int dtype,
                               gmlm_stream_t stream) {
  static const char* who = "swiglu_bwd";
  int rc = glu_check(who, rows, inter, dtype);
  if (rc != GMLM_OK) return rc;
  if (rows == 0) return GMLM_OK;
  GMLM_REQUIRE(dy && gate_up && dgate_up && aligned16(dy) && aligned16(gate_up) && aligned16(dgate_up),
               "%s: null or not 16-byte aligned pointer", who);
  hipStream_t st = as_stream(stream);
  const int v = dtype == GMLM_F32 ? 4 : 8;
  const int grid = grid_cap(cdiv(rows * (inter / v), 256), 8192);
  if (dtype == GMLM_BF16) swiglu_bwd_kernel<bf16_t><<<grid, 256, 0, st>>>((const bf16_t*)dy, (const bf16_t*)gate_up, rows, inter, (bf16_t*)dgate_up);
  else swiglu_bwd_kernel<float><<<grid, 256, 0, st>>>((const float*)dy, (const float*)gate_up, rows, inter, (float*)dgate_up);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
