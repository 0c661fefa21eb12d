// bias + dropout + residual + LayerNorm (+GELU) for rows of 1,028 ... 4,096 elements (gmlm_bias_res_layernorm_wide_*):
// the LayerNorm(P) of MultiScaleFusion and of the fusion MLP on a text encoder wider than 1,024.
// The kernels of norm_kernels.hip (K6) give a row one wave (at most 64 lanes x 4 chunks of 16 B = 1,024 fp32); here ONE
// 256-lane workgroup holds a row in registers (CH <= 4 chunks of 16 B per lane, chunk index c * 256 + lane: coalesced), and
// a workgroup strides through the rows.  Row sums: wave butterfly, then the four wave sums added in order through LDS, the
// same expression in every lane.  Element arithmetic, rounding points and the dropout bit (dropout_keep_bits of the element
// offset row * f + column) are those of K6, so a checkpoint recompute replays the mask.
// Backward: a lane owns fixed columns, so its dgamma / dbeta / dbias partial sums over the rows of its workgroup need no
// in-block reduction; the workgroup writes them to partial[3][blocks][f] and rows_sum_kernel (colreduce.hpp) adds the blocks in
// index order.  No atomics: a repeated call gives identical bytes.
#include "colreduce.hpp"
#include "../../include/gmlm_hip_wide.h"

namespace gmlm {
namespace lnw {

constexpr int NT = 256, kMaxBlocks = 256;   // backward: at most one partial row per CU

template <typename T> struct Ch;             // chunks of 16 B per lane that cover 4,096 columns
template <> struct Ch<float> { static constexpr int v = 4; };
template <> struct Ch<bf16_t> { static constexpr int v = 2; };

template <int V>
__device__ __forceinline__ void load_param(const float* __restrict__ p, int col, float (&o)[V], float fill) {
  if (p) {
#pragma unroll
    for (int v = 0; v < V; v += 4) {
      const float4 t = *reinterpret_cast<const float4*>(p + col + v);
      o[v] = t.x; o[v + 1] = t.y; o[v + 2] = t.z; o[v + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = fill;
  }
}

// sum over the 256 lanes: butterfly inside the wave, then ((w0 + w1) + w2) + w3; every lane returns the same bits
__device__ __forceinline__ float block_sum(float v, float* red, int wv, int lane) {
  v = wave_sum(v);
  if (lane == 0) red[wv] = v;
  __syncthreads();
  const float s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

template <typename T, bool ACT>
__global__ __launch_bounds__(NT) void fwd_kernel(const T* __restrict__ x, const float* __restrict__ bias, const T* __restrict__ res,
                                                 const float* __restrict__ gamma, const float* __restrict__ beta, int64_t rows, int f,
                                                 float eps, uint32_t thresh, float keep_scale, SeedArg seed_a, T* __restrict__ y,
                                                 float* __restrict__ mean_o, float* __restrict__ rstd_o) {
  constexpr int V = Store<T>::kVec, CH = Ch<T>::v;
  __shared__ float red[4];
  const uint64_t seed = seed_a.get();
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nch = f / V;
  float gm[CH][V], bt[CH][V], bi[CH][V];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * NT + tid;
    if (ch < nch) {
      load_param<V>(gamma, ch * V, gm[c], 1.f);
      load_param<V>(beta, ch * V, bt[c], 0.f);
      load_param<V>(bias, ch * V, bi[c], 0.f);
    }
  }
  const float inv_f = 1.f / (float)f;
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {       // block-uniform bound: the barriers of block_sum are safe
    float z[CH][V];
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = c * NT + tid;
      if (ch < nch) {
        const int64_t off = r * f + (int64_t)ch * V;
        Store<T>::ldv(x + off, z[c]);
        float rr[V];
        if (res) Store<T>::ldv(res + off, rr);
#pragma unroll
        for (int v = 0; v < V; ++v) z[c][v] += bi[c][v];
        if (thresh) {
          const uint32_t kb = dropout_keep_bits<V>(seed, (uint64_t)off, thresh);
#pragma unroll
          for (int v = 0; v < V; ++v) z[c][v] = ((kb >> v) & 1u) ? z[c][v] * keep_scale : 0.f;
        }
        if (res) {
#pragma unroll
          for (int v = 0; v < V; ++v) z[c][v] += rr[v];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) sum += z[c][v];
      }
    }
    const float mu = block_sum(sum, red, wv, lane) * inv_f;
    float sq = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (c * NT + tid < nch)
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float d = z[c][v] - mu;
          sq += d * d;
        }
    const float rs = 1.f / sqrtf(block_sum(sq, red, wv, lane) * inv_f + eps);
    if (tid == 0) {
      if (mean_o) mean_o[r] = mu;
      if (rstd_o) rstd_o[r] = rs;
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = c * NT + tid;
      if (ch < nch) {
        float o[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float t = (z[c][v] - mu) * rs * gm[c][v] + bt[c][v];
          o[v] = ACT ? gelu_fwd_t<T>(t) : t;
        }
        Store<T>::stv(y + r * f + (int64_t)ch * V, o);
      }
    }
  }
}

template <typename T, bool ACT, bool DROP, bool RES>
__global__ __launch_bounds__(NT) void bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ bias,
                                                 const T* __restrict__ res, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, const float* __restrict__ mean,
                                                 const float* __restrict__ rstd, int64_t rows, int f, uint32_t thresh,
                                                 float keep_scale, SeedArg seed_a, T* __restrict__ dx, T* __restrict__ dres,
                                                 float* __restrict__ partial /* [3][gridDim.x][f] */) {
  constexpr int V = Store<T>::kVec, CH = Ch<T>::v;
  static_assert(CH * V <= 32, "keep bits of one lane's row slice must fit one word");
  __shared__ float red[4];
  const uint64_t seed = seed_a.get();
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nch = f / V;
  float gm[CH][V], bt[CH][V], bi[CH][V];
  float dg[CH][V], db[CH][V], dbi[CH][V];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * NT + tid;
    if (ch < nch) {
      load_param<V>(gamma, ch * V, gm[c], 1.f);
      if (ACT) load_param<V>(beta, ch * V, bt[c], 0.f);
      load_param<V>(bias, ch * V, bi[c], 0.f);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) dg[c][v] = db[c][v] = dbi[c][v] = 0.f;
  }
  const float inv_f = 1.f / (float)f;
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {       // rows of a workgroup in increasing order
    const float mu = mean[r], rs = rstd[r];
    float zh[CH][V], dzh[CH][V];
    float s1 = 0.f, s2 = 0.f;
    uint32_t keep = 0;                       // dropout decisions of this lane's elements, reused by the dx pass
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = c * NT + tid;
      if (ch < nch) {
        const int64_t off = r * f + (int64_t)ch * V;
        float gv[V], rr[V];
        Store<T>::ldv(x + off, zh[c]);
        Store<T>::ldv(dy + off, gv);
        if (RES) Store<T>::ldv(res + off, rr);
        uint32_t kb = 0;
        if (DROP) {
          kb = dropout_keep_bits<V>(seed, (uint64_t)off, thresh);
          keep |= kb << (c * V);
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
          float z = zh[c][v] + bi[c][v];
          if (DROP) z = ((kb >> v) & 1u) ? z * keep_scale : 0.f;
          if (RES) z += rr[v];
          z = (z - mu) * rs;
          zh[c][v] = z;
          float dyn = gv[v];
          if (ACT) dyn *= gelu_grad_t<T>(z * gm[c][v] + bt[c][v]);
          dg[c][v] += dyn * z;
          db[c][v] += dyn;
          dzh[c][v] = dyn * gm[c][v];
          s1 += dzh[c][v];
          s2 += dzh[c][v] * z;
        }
      }
    }
    s1 = block_sum(s1, red, wv, lane) * inv_f;
    s2 = block_sum(s2, red, wv, lane) * inv_f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int ch = c * NT + tid;
      if (ch < nch) {
        const int64_t off = r * f + (int64_t)ch * V;
        float dz[V], dxv[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
          dz[v] = rs * (dzh[c][v] - s1 - zh[c][v] * s2);
          dxv[v] = DROP ? (((keep >> (c * V + v)) & 1u) ? dz[v] * keep_scale : 0.f) : dz[v];
          dbi[c][v] += dxv[v];
        }
        Store<T>::stv(dx + off, dxv);
        if (dres) Store<T>::stv(dres + off, dz);
      }
    }
  }
  const int64_t slab = (int64_t)gridDim.x * f;
  float* prow = partial + (int64_t)blockIdx.x * f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * NT + tid;
    if (ch < nch) {
#pragma unroll
      for (int v = 0; v < V; v += 4) {
        *reinterpret_cast<float4*>(prow + ch * V + v) = make_float4(dg[c][v], dg[c][v + 1], dg[c][v + 2], dg[c][v + 3]);
        *reinterpret_cast<float4*>(prow + slab + ch * V + v) = make_float4(db[c][v], db[c][v + 1], db[c][v + 2], db[c][v + 3]);
        *reinterpret_cast<float4*>(prow + 2 * slab + ch * V + v) = make_float4(dbi[c][v], dbi[c][v + 1], dbi[c][v + 2], dbi[c][v + 3]);
      }
    }
  }
}

static inline int bwd_blocks(int64_t rows) { return (int)(rows < 1 ? 1 : (rows > kMaxBlocks ? kMaxBlocks : rows)); }

static int check(const char* who, int64_t rows, int64_t f, int dtype, float dropout_p) {
  GMLM_REQUIRE(rows >= 0 && f > 0, "%s: bad sizes", who);
  GMLM_REQUIRE(dtype == GMLM_F32 || dtype == GMLM_BF16, "%s: unsupported dtype", who);
  const int v = dtype == GMLM_F32 ? 4 : 8;
  GMLM_REQUIRE(f % v == 0 && f > 1024 && f <= 4096, "%s: row width %ld must be a multiple of %d, above 1024 and <= 4096", who, (long)f, v);
  GMLM_REQUIRE(rows < ((int64_t)1 << 40), "%s: too many rows", who);
  GMLM_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout_p must be in [0,1)", who);
  return GMLM_OK;
}

}  // namespace lnw
}  // namespace gmlm

using namespace gmlm;

extern "C" int gmlm_bias_res_layernorm_wide_fwd(const void* x, const float* bias, const void* residual, const float* gamma,
                                                const float* beta, int64_t rows, int64_t f, float eps, int act, float dropout_p,
                                                uint64_t seed_host, const uint64_t* seed_dev, void* y, float* mean, float* rstd,
                                                int dtype, gmlm_stream_t stream) {
  const SeedArg seed{seed_host, seed_dev};
  int rc = lnw::check("bias_res_layernorm_wide_fwd", rows, f, dtype, dropout_p);
  if (rc != GMLM_OK) return rc;
  if (rows == 0) return GMLM_OK;
  GMLM_REQUIRE(x && gamma && beta && y, "bias_res_layernorm_wide_fwd: null pointer");
  GMLM_REQUIRE(aligned16(x) && aligned16(y) && aligned16(residual) && aligned16(bias) && aligned16(gamma) && aligned16(beta),
               "bias_res_layernorm_wide_fwd: 16-byte alignment required");
  const uint32_t th = dropout_threshold(dropout_p);
  const float ks = dropout_keep_scale(th);
  hipStream_t st = as_stream(stream);
  const int grid = grid_cap(rows);
#define L(T, A) lnw::fwd_kernel<T, A><<<grid, lnw::NT, 0, st>>>((const T*)x, bias, (const T*)residual, gamma, beta, rows, (int)f, eps, th, ks, seed, (T*)y, mean, rstd)
  if (dtype == GMLM_F32) { if (act) L(float, true); else L(float, false); }
  else { if (act) L(bf16_t, true); else L(bf16_t, false); }
#undef L
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_bias_res_layernorm_wide_bwd_workspace_bytes(int64_t rows, int64_t f) {
  return (size_t)lnw::bwd_blocks(rows) * 3 * (size_t)(f > 0 ? f : 1) * sizeof(float);
}

extern "C" int gmlm_bias_res_layernorm_wide_bwd(const void* dy, const void* x, const float* bias, const void* residual,
                                                const float* gamma, const float* beta, const float* mean, const float* rstd,
                                                int64_t rows, int64_t f, int act, float dropout_p, uint64_t seed_host,
                                                const uint64_t* seed_dev, void* dx, void* dresidual, float* dgamma, float* dbeta,
                                                float* dbias, int dtype, void* workspace, size_t workspace_bytes,
                                                gmlm_stream_t stream) {
  const SeedArg seed{seed_host, seed_dev};
  int rc = lnw::check("bias_res_layernorm_wide_bwd", rows, f, dtype, dropout_p);
  if (rc != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  if (rows == 0) {
    if (dgamma) GMLM_HIP(zero_async(dgamma, sizeof(float) * f, st));
    if (dbeta) GMLM_HIP(zero_async(dbeta, sizeof(float) * f, st));
    if (dbias) GMLM_HIP(zero_async(dbias, sizeof(float) * f, st));
    return GMLM_OK;
  }
  GMLM_REQUIRE(dy && x && gamma && beta && mean && rstd && dx, "bias_res_layernorm_wide_bwd: null pointer");
  GMLM_REQUIRE(aligned16(dy) && aligned16(x) && aligned16(dx) && aligned16(residual) && aligned16(dresidual) && aligned16(bias) &&
                   aligned16(gamma) && aligned16(beta),
               "bias_res_layernorm_wide_bwd: 16-byte alignment required");
  GMLM_REQUIRE_WS(workspace && aligned16(workspace) && workspace_bytes >= gmlm_bias_res_layernorm_wide_bwd_workspace_bytes(rows, f),
                  "bias_res_layernorm_wide_bwd: workspace too small (or not 16-byte aligned)");
  const uint32_t th = dropout_threshold(dropout_p);
  const float ks = dropout_keep_scale(th);
  const int blocks = lnw::bwd_blocks(rows);
  float* partial = static_cast<float*>(workspace);
#define L3(T, A, D, R) lnw::bwd_kernel<T, A, D, R><<<blocks, lnw::NT, 0, st>>>((const T*)dy, (const T*)x, bias, (const T*)residual, gamma, beta, mean, rstd, rows, (int)f, th, ks, seed, (T*)dx, (T*)dresidual, partial)
#define L(T, A) do { if (th) { if (residual) L3(T, A, true, true); else L3(T, A, true, false); } \
                     else { if (residual) L3(T, A, false, true); else L3(T, A, false, false); } } while (0)
  if (dtype == GMLM_F32) { if (act) L(float, true); else L(float, false); }
  else { if (act) L(bf16_t, true); else L(bf16_t, false); }
#undef L
#undef L3
  GMLM_LAUNCH_CHECK();
  // second stage: the partial rows of each of dgamma / dbeta / dbias summed in index order
  float* outs[3] = {dgamma, dbeta, dbias};
  for (int k = 0; k < 3; ++k) {
    if (!outs[k]) continue;
    rows_sum_kernel<<<(unsigned)cdiv(f, 32), 256, 0, st>>>(partial + (int64_t)k * blocks * f, blocks, f, outs[k]);
    GMLM_LAUNCH_CHECK();
  }
  return GMLM_OK;
}
