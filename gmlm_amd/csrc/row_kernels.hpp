// The shared bodies of the pre-norm encoders' row kernels (decoder_kernels.hip: Qwen3 geometry; modernbert_kernels.hip):
// residual add + norm, the weight-gradient column sums, the gated-linear-unit product and the rotate-half rotary pieces.
// bf16 or fp32 storage, fp32 arithmetic, ONE rounding on store.  The __global__ kernels of the two files are thin wrappers
// over these bodies: a policy type picks the row statistics (RmsStat / LnStat) or the activation (SiluAct / GeluAct).
#pragma once
#include "colreduce.hpp"

namespace gmlm {

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

// the value a store of `x` as T leaves in memory (the residual stream is read back in T by every later kernel, so the
// statistics are taken over the ROUNDED sum, as the reference takes them over its bf16 hidden states)
template <typename T> __device__ __forceinline__ float rounded(float x);
template <> __device__ __forceinline__ float rounded<float>(float x) { return x; }
template <> __device__ __forceinline__ float rounded<bf16_t>(float x) { return bf16_to_f32(f32_to_bf16(x)); }

// ------------------------------------------------------------------------------------------------
// add + norm.  One wave per row, CH 16-byte chunks per lane (f <= 64 * CH * V), the row stays in registers.
//   s = a + b (b optional) stored as T;  y = xhat * w (+ beta);  the row statistics saved in fp32
//   RmsStat: xhat = s * rstd,           rstd = rsqrt(mean(s^2) + eps)
//   LnStat:  xhat = (s - mean) * rstd,  rstd = rsqrt(mean((s - mean)^2) + eps): two passes over the registers, the mean first,
//            then the sum of squared deviations (no E[x^2] - mean^2 cancellation)
// ------------------------------------------------------------------------------------------------
struct RmsStat {
  static constexpr bool kMean = false;
  static __device__ __forceinline__ float xhat(float x, float, float rs) { return x * rs; }
};
struct LnStat {
  static constexpr bool kMean = true;
  static __device__ __forceinline__ float xhat(float x, float mu, float rs) { return (x - mu) * rs; }
};

// beta, mean_o: LnStat only.  The host checks that s_out comes with b; the RMS kernel has always tested it as well.
template <typename T, int CH, typename Stat>
__device__ __forceinline__ void add_norm_fwd_body(const T* a, const T* b, const float* w,
                                                  const float* beta, int64_t rows, int f, float eps,
                                                  T* s_out, T* y, float* mean_o,
                                                  float* rstd_o) {
  constexpr int V = Store<T>::kVec;
  const int lane = threadIdx.x & 63, nch = f / V;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;                                   // wave-uniform; no barrier in this kernel
  float z[CH][V];
  float acc = 0.f;                                         // RmsStat: the squares; LnStat: the sum
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
        if (Stat::kMean || s_out) Store<T>::stv(s_out + off, z[c]);
      }
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if constexpr (Stat::kMean) acc += z[c][v];
        else acc = fmaf(z[c][v], z[c][v], acc);            // a chain of v_fma_f32 (separate squares pair up into v_pk_mul_f32)
      }
    }
  }
  float mu = 0.f;
  if constexpr (Stat::kMean) {
    mu = lanes_sum<64>(acc) / (float)f;
    acc = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (c * 64 + lane < nch) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float dlt = z[c][v] - mu;
          acc = fmaf(dlt, dlt, acc);
        }
      }
    }
  }
  const float rs = 1.f / sqrtf(lanes_sum<64>(acc) / (float)f + eps);
  if (lane == 0) {
    if constexpr (Stat::kMean) mean_o[r] = mu;
    rstd_o[r] = rs;
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      float wv[V], o[V];
      load_f32<V>(w + ch * V, wv);
#pragma unroll
      for (int v = 0; v < V; ++v) o[v] = Stat::xhat(z[c][v], mu, rs) * wv[v];
      if constexpr (Stat::kMean) {
        if (beta) {
          float bv[V];
          load_f32<V>(beta + ch * V, bv);
#pragma unroll
          for (int v = 0; v < V; ++v) o[v] += bv[v];
        }
      }
      Store<T>::stv(y + r * f + (int64_t)ch * V, o);
    }
  }
}

// ds = dres (optional: the gradient arriving on the residual stream) + rstd * (g [- mean(g)] - xhat * mean(g * xhat)),
// g = dy * w; the mean(g) term is LnStat's (as is `mean`).  The gradient of a AND of b is ds.
template <typename T, int CH, typename Stat>
__device__ __forceinline__ void add_norm_bwd_body(const T* dy, const T* dres, const T* s,
                                                  const float* w, const float* mean,
                                                  const float* rstd, int64_t rows, int f, T* ds) {
  constexpr int V = Store<T>::kVec;
  const int lane = threadIdx.x & 63, nch = f / V;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  float mu = 0.f;
  if constexpr (Stat::kMean) mu = mean[r];
  const float rs = rstd[r];
  float g[CH][V], xh[CH][V];
  float sg = 0.f, dot = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      const int64_t off = r * f + (int64_t)ch * V;
      float wv[V];
      Store<T>::ldv(dy + off, g[c]);
      Store<T>::ldv(s + off, xh[c]);
      load_f32<V>(w + ch * V, wv);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        g[c][v] *= wv[v];
        xh[c][v] = Stat::xhat(xh[c][v], mu, rs);
        if constexpr (Stat::kMean) sg += g[c][v];
        dot += g[c][v] * xh[c][v];
      }
    }
  }
  float m1 = 0.f;
  if constexpr (Stat::kMean) m1 = lanes_sum<64>(sg) / (float)f;
  const float m2 = lanes_sum<64>(dot) / (float)f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int ch = c * 64 + lane;
    if (ch < nch) {
      const int64_t off = r * f + (int64_t)ch * V;
      float o[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if constexpr (Stat::kMean) o[v] = rs * (g[c][v] - m1 - xh[c][v] * m2);
        else o[v] = rs * (g[c][v] - xh[c][v] * m2);
      }
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

// The column sums of the weight gradients (col_reduce: fixed order): v[0] = dy * xhat (dw or dgamma), v[1] = dy (dbeta,
// K = 2).  `mean` is read only with MEAN.  RmsDwFn and mbert::LnDwFn hold the pointers: they are kernel arguments, so
// each keeps its own layout.
template <typename T, int K, bool MEAN>
__device__ __forceinline__ void norm_dw_terms(const T* dy, const T* s, const float* mean, const float* rstd, int64_t f, int64_t r,
                                              int64_t c, float (&v)[K]) {
  const float g = Store<T>::ld(dy + r * f + c), x = Store<T>::ld(s + r * f + c);
  if constexpr (MEAN) v[0] = g * ((x - mean[r]) * rstd[r]);
  else v[0] = g * (x * rstd[r]);
  if constexpr (K == 2) v[1] = g;
}

// ------------------------------------------------------------------------------------------------
// Gated linear unit: gu = [gate | up] rows of 2 * I  ->  y = act(gate) * up  [rows, I]
// ------------------------------------------------------------------------------------------------
struct SiluAct {
  template <typename T> static __device__ __forceinline__ float fwd(float g) { return g / (1.f + expf(-g)); }
  // d (act(g) * u) -> dg, du
  template <typename T> static __device__ __forceinline__ void bwd(float d, float g, float u, float& dg, float& du) {
    const float sig = 1.f / (1.f + expf(-g));
    du = d * g * sig;
    dg = d * u * sig * (1.f + g * (1.f - sig));
  }
};
struct GeluAct {   // erf GELU: common.hpp
  template <typename T> static __device__ __forceinline__ float fwd(float g) { return gelu_fwd_t<T>(g); }
  template <typename T> static __device__ __forceinline__ void bwd(float d, float g, float u, float& dg, float& du) {
    du = d * gelu_fwd_t<T>(g);
    dg = d * u * gelu_grad_t<T>(g);
  }
};

template <typename T, typename Act>
__device__ __forceinline__ void glu_fwd_body(const T* gu, int64_t rows, int64_t inter, T* y) {
  constexpr int V = Store<T>::kVec;
  const int64_t cpr = inter / V, total = rows * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cpr, c = (i % cpr) * V;
    float g[V], u[V], o[V];
    Store<T>::ldv(gu + r * 2 * inter + c, g);
    Store<T>::ldv(gu + r * 2 * inter + inter + c, u);
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = Act::template fwd<T>(g[v]) * u[v];
    Store<T>::stv(y + r * inter + c, o);
  }
}

template <typename T, typename Act>
__device__ __forceinline__ void glu_bwd_body(const T* dy, const T* gu, int64_t rows, int64_t inter,
                                             T* dgu) {
  constexpr int V = Store<T>::kVec;
  const int64_t cpr = inter / V, total = rows * cpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / cpr, c = (i % cpr) * V;
    float g[V], u[V], d[V], dg[V], du[V];
    Store<T>::ldv(gu + r * 2 * inter + c, g);
    Store<T>::ldv(gu + r * 2 * inter + inter + c, u);
    Store<T>::ldv(dy + r * inter + c, d);
#pragma unroll
    for (int v = 0; v < V; ++v) Act::template bwd<T>(d[v], g[v], u[v], dg[v], du[v]);
    Store<T>::stv(dgu + r * 2 * inter + c, dg);
    Store<T>::stv(dgu + r * 2 * inter + inter + c, du);
  }
}

// ------------------------------------------------------------------------------------------------
// Rotate-half rotary embedding at head dim D.  A head row of D elements = LPR = D / V lanes x 16 bytes; element i pairs with
// i + D / 2, i.e. lane j with lane j ^ (LPR / 2): one cross-lane exchange, no LDS.
// cs: fp32 [max_len, 2, D / 2] (cos row, then sin row) of the token's position: row % seq_len (padded [b, seq_len] layout), or,
// when pos_ids is given (packed rows), pos_ids[row] clamped into [0, max_len) so that no position reads outside the table.
// ------------------------------------------------------------------------------------------------
// pos_ids is a kernel argument: the branch is uniform over the grid
template <int D>
__device__ __forceinline__ const float* rope_row(const float* __restrict__ cs, int64_t t, int64_t seq_len,
                                                 const int32_t* __restrict__ pos_ids, int64_t max_len) {
  if (pos_ids) {
    int64_t pos = pos_ids[t];
    pos = pos < 0 ? 0 : (pos >= max_len ? max_len - 1 : pos);
    return cs + pos * D;
  }
  return cs + (t % seq_len) * D;
}

// Head row `item` of tokens x nh (one group of LPR lanes holds it) -> its token t and head hd; returns `live`.  Whole
// groups are live or not; a dead group computes on token 0, head 0, so that every lane of the wave reaches the shuffles,
// and stores nothing.
__device__ __forceinline__ bool head_row(int64_t item, int64_t items, int nh, int64_t& t, int& hd) {
  const bool live = item < items;
  t = live ? item / nh : 0;
  hd = live ? (int)(item % nh) : 0;
  return live;
}

// forward: out[i] = x[i] cos[i] - x[i + D/2] sin[i],  out[i + D/2] = x[i + D/2] cos[i] + x[i] sin[i]; `upper`: this lane
// holds the second half.  INV (backward): the transposed = inverse rotation, the same with sin negated.  Called outside
// any `live` branch: every lane of the wave takes part in the exchange.
template <int LPR, bool INV>
__device__ __forceinline__ float rotate_half(float x, float c, float sn, bool upper) {
  const float other = __shfl_xor(x, LPR / 2, 64);
  return fmaf(upper != INV ? other : -other, sn, x * c);   // the sign chosen once: one v_cndmask and one fma
}

// ---- host ----------------------------------------------------------------------------------------
static int glu_check(const char* who, int64_t rows, int64_t inter, int dtype) {
  GMLM_REQUIRE(dtype == GMLM_F32 || dtype == GMLM_BF16, "%s: unsupported dtype", who);
  const int v = dtype == GMLM_F32 ? 4 : 8;
  GMLM_REQUIRE(rows >= 0 && inter > 0 && inter % v == 0, "%s: width %ld must be a multiple of %d", who, (long)inter, v);
  return GMLM_OK;
}

// Sizes of a rotary call at head dim D over fused [q | k | v] rows of hq + 2 hkv heads; `other_stride` is the second row
// block's (the output, or the gradient), at least `min_other` wide.  Sizes first, pointers second: a call with no token
// returns GMLM_OK in between, as the other row kernels do for zero rows.  seq_len = 0 is the padded layout [b, 0]: it has
// no token, and only then is it accepted; with pos_ids (by_pos) the sequence length is not used.
static int rope_sizes(const char* who, int64_t D, int64_t stride, int64_t other_stride, int64_t min_other, int64_t tokens,
                      int64_t seq_len, bool by_pos, int64_t max_len, int64_t hq, int64_t hkv, int64_t d, int dtype) {
  GMLM_REQUIRE(dtype == GMLM_F32 || dtype == GMLM_BF16, "%s: unsupported dtype", who);
  GMLM_REQUIRE(d == D, "%s: head dim %ld not supported (this entry point takes %ld)", who, (long)d, (long)D);
  // hq + hkv < 4096 without the overflowing sum; rope64 passes hq = hkv = h, for which this is its h < 2048
  GMLM_REQUIRE(tokens >= 0 && hq > 0 && hkv > 0 && hq < 4096 - hkv, "%s: bad sizes", who);
  GMLM_REQUIRE(max_len > 0, "%s: empty cos / sin table", who);
  if (!by_pos) {
    GMLM_REQUIRE(seq_len >= 0 && seq_len <= max_len, "%s: sequence length %ld exceeds the %ld rows of the cos / sin table", who,
                 (long)seq_len, (long)max_len);
    GMLM_REQUIRE(seq_len > 0 || tokens == 0, "%s: %ld tokens in sequences of length 0", who, (long)tokens);
  }
  const int v = dtype == GMLM_F32 ? 4 : 8;
  GMLM_REQUIRE(stride >= (hq + 2 * hkv) * D && stride % v == 0, "%s: qkv row stride %ld must be >= %ld and a multiple of %d", who,
               (long)stride, (long)((hq + 2 * hkv) * D), v);
  GMLM_REQUIRE(other_stride >= min_other && other_stride % v == 0, "%s: row stride %ld must be >= %ld and a multiple of %d", who,
               (long)other_stride, (long)min_other, v);
  GMLM_REQUIRE(tokens * (hq + hkv) < ((int64_t)1 << 34), "%s: too many head rows", who);
  return GMLM_OK;
}

}  // namespace gmlm
