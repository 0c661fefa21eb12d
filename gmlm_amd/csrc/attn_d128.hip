// Attention at head dim 128, forward + backward, gfx950 MFMA (gmlm_attention_d128_*).
// Shape: padded [b, l, h*128] with an optional per-sequence key length (kv_len) and in-kernel probability dropout: the
// CrossAttention of a 1024-wide text encoder (8 heads x 128, one sequence of N nodes, main.py:159-163) and the self-attention
// of any encoder whose head dim is 97..128 (zero-padded to 128 by nn.attention_any_dim).
// Forward, delta and dK/dV ARE the streaming kernels of attn_kernels.hip: both files instantiate the bodies of attn_stream.hpp
// (S^T = K Q^T with the query on the lane, online softmax in the log2 domain, P fed straight from the accumulators into
// O^T += V^T P^T, bf16 folding of lse / delta / the key mask into one extra contraction step, exact fp32 delta through out_lo,
// the replayable 2 x 2 dropout hash of attn_common.hpp with the same row offsets).  dq_kernel alone keeps its own copy of
// attn_dq_body's text (reason at the kernel).  This file fixes D = 128, 4 waves, and:
//  * 1-D grids of (tile, (batch, head)) work items: no 65,535 bound on batch * heads;
//  * bf16: 64-row K / V (forward, dQ) and 32-row Q / dO (dK/dV) tiles, double-buffered in LDS (68 KiB / 35 KiB per
//    workgroup); fp32 (the 1e-4 parity path, v_mfma_f32_32x32x2_f32): 32-row tiles, one buffer.  No kernel spills.
//  * dK/dV without atomics: a workgroup owns 128 keys and walks all query tiles in order (deterministic).
// The argument checks and the AttnParams filling shared with the other attention entry points are in attn_host.hpp.
#include "attn_stream.hpp"
#include "attn_host.hpp"

namespace gmlm {
namespace d128 {

constexpr int D = 128, NW = 4, NT = NW * 64, BQ = NW * 32;   // 4 waves, 32 rows each: 128 query (or key) rows per workgroup

struct Params {
  AttnParams a;            // lse / delta are [b, h, lq]
  int64_t dout_stride;     // row stride of dO / O (= h * 128)
};

// Cfg<T> (tile sizes) is attn_stream.hpp's, decode() (1-D grid -> tile, batch, head) attn_common.hpp's

// forward: workgroup = 128 query rows of one (batch, head), loop over key tiles
template <typename T, bool DROP>
__global__ __launch_bounds__(NT) void fwd_kernel(Params x) {
  const Item it = decode(x.a);
  attn_fwd_body<T, D, NW, DROP, Cfg<T>::KT, Cfg<T>::DBUF>(x.a, it.tile, it.b, it.hd, x.dout_stride);
}

// backward: delta = rowsum(dO * O) over rows of [b * lq, h, 128] (O = out + out_lo when the forward stored the residual)
template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                    int64_t rows /* b * lq * h */, int64_t lq, int64_t hn, float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);     // 16 (bf16) or 32 (fp32) lanes per row
}

// backward: dQ.  workgroup = 128 queries of one (batch, head), loop over key tiles.
// The text of attn_dq_body (attn_stream.hpp), kept as a kernel of its own: compiled through the shared body the bf16 dropout
// instantiation takes 262 instead of 250 VGPRs, and with 68 KiB of LDS per workgroup that is one workgroup per CU instead
// of two.  A fix to either copy belongs in both.
template <typename T, bool DROP>
__global__ __launch_bounds__(NT) void dq_kernel(Params x) {
  const AttnParams& p = x.a;
  constexpr bool DBUF = Cfg<T>::DBUF;
  constexpr int KT = Cfg<T>::KT, KB = KT / 32, PITCH = D + Pad<T>::v, DB = D / 32, NBUF = DBUF ? 2 : 1;
  __shared__ __attribute__((aligned(16))) T ks[NBUF][KT * PITCH];
  __shared__ __attribute__((aligned(16))) T vs[NBUF][KT * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t pairs = p.b * p.h, item = blockIdx.x;
  const int64_t qt = item / pairs, bh = item % pairs;
  const int64_t b = bh / p.h, hd = bh % p.h;
  int64_t lq_, lk_, qbase, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, qbase, kbase, lse_base);
  const int64_t q_tile0 = qt * BQ;
  if (q_tile0 >= lq_) return;
  const int64_t q_row = q_tile0 + w * 32 + r;
  const bool q_ok = q_row < lq_;
  const bool wave_live = q_tile0 + w * 32 < lq_;
  const int64_t kvlen = clamp_kvlen(p, b, lk_);
  const int64_t qr = q_ok ? q_row : 0;
  const T* kg = static_cast<const T*>(p.k) + kbase * p.k_stride + hd * D;
  const T* vg = static_cast<const T*>(p.v) + kbase * p.v_stride + hd * D;
  RowFrag<T, D> qf, dof;
  qf.load(static_cast<const T*>(p.q) + (qbase + qr) * p.q_stride + hd * D, q_ok, h);
  dof.load(static_cast<const T*>(p.dout) + (qbase + qr) * x.dout_stride + hd * D, q_ok, h);
  const float sl2 = p.scale * kLog2e;
  const float lse2 = q_ok ? p.lse[lse_base + q_row] * kLog2e : INFINITY;
  const float dl = q_ok ? p.delta[lse_base + q_row] : 0.f;
  const int kvl = (int)(kvlen < (1 << 30) ? kvlen : (1 << 30));
  const uint32_t dq_u = drop_base(attn_seed(p), lse_base) + (uint32_t)(q_row >> 1) * kDropC1 + (uint32_t)(2 * h) * kDropC2;
  const int q_odd = (int)(q_row & 1);
  // bf16: scale * log2 e folded into Q, lse / delta / the kv_len mask folded into one extra contraction step (attn_kernels.hip)
  constexpr bool FOLD = sizeof(T) == 2;
  bf16x8 ones_a, ext_s, ext_dp;
  if constexpr (FOLD) {
#pragma unroll
    for (int s_ = 0; s_ < D / 16; ++s_)
#pragma unroll
      for (int j = 0; j < 8; ++j) qf.v[s_][j] = (__bf16)((float)qf.v[s_][j] * sl2);
    const float l2 = q_ok ? lse2 : 0x1p100f;
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
  const int ntiles = (int)((kvlen + KT - 1) / KT);
  TileRegs<T, D, KT, NT> kr, vr;
  kr.init(p.k_stride, tid);
  vr.init(p.v_stride, tid);
  if (ntiles > 0) {
    kr.load(kg, p.k_stride, 0, lk_, tid);
    vr.load(vg, p.v_stride, 0, lk_, tid);
    kr.store(ks[0], tid);
    vr.store(vs[0], tid);
  }
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const int64_t kv0 = (int64_t)t * KT;
    const int cur = DBUF ? (t & 1) : 0;
    const bool more = t + 1 < ntiles;
    if (DBUF && more) {
      kr.load(kg, p.k_stride, kv0 + KT, lk_, tid);
      vr.load(vg, p.v_stride, kv0 + KT, lk_, tid);
    }
    if (wave_live) {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        f32x16 s, dp;
#pragma unroll
        for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
        const int64_t k32 = kv0 + kb * 32;
        const bool full = k32 + 32 <= kvlen;                            // block-uniform
        if constexpr (FOLD) {
          bf16x8 oa = ones_a;
          if (!full) oa[2] = (h == 0 && (int)k32 + r >= kvl) ? (__bf16)1.f : (__bf16)0.f;   // A row r = key r of the block
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(oa, ext_s, s, 0, 0, 0);
          if (!DROP) dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ones_a, ext_dp, dp, 0, 0, 0);
        }
        mma_rows<D>(ks[cur], PITCH, kb * 32, qf, s, r, h);
        mma_rows<D>(vs[cur], PITCH, kb * 32, dof, dp, r, h);
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          float p0, p1;
          if constexpr (FOLD) {
            p0 = fast_exp2(s[i]);
            p1 = fast_exp2(s[i + 1]);
          } else {
            const int64_t key = k32 + acc_row(i, h);                   // even; registers i, i+1 = keys key, key+1
            float a0 = fmaf(s[i], sl2, -lse2), a1 = fmaf(s[i + 1], sl2, -lse2);
            if (!full) { a0 = key < kvl ? a0 : -INFINITY; a1 = key + 1 < kvl ? a1 : -INFINITY; }
            p0 = fast_exp2(a0); p1 = fast_exp2(a1);
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

// backward: dK, dV.  workgroup = 128 keys of one (batch, head), loop over query tiles of 32 in order
template <typename T, bool DROP>
__global__ __launch_bounds__(NT) void dkv_kernel(Params x) {
  const Item it = decode(x.a);
  attn_dkv_body<T, D, NW, DROP, Cfg<T>::QT, Cfg<T>::DBUF>(x.a, it.tile, it.b, it.hd, x.dout_stride);
}

// the checks of attn_host.hpp up to the empty-problem return, with this family's head dim and work-item bound; fills the
// launch parameters
static int setup(const char* who, Params& x, const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                 int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                 uint64_t seed, const uint64_t* seed_dev, const void* out_lo, int dtype) {
  int rc = attn_check_shape(who, b >= 0 && h > 0 && lq >= 0 && lk >= 0, d == 128, d, "this entry point takes 128", dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  if ((rc = attn_check_rates(who, dropout_p, nullptr, scale)) != GMLM_OK) return rc;
  const int64_t rows = lq > lk ? lq : lk;
  GMLM_REQUIRE(cdiv(rows, BQ) * b * h < ((int64_t)1 << 31), "%s: too many work items", who);
  x = Params{};
  attn_fill(x.a, q, k, v, kv_len, b, h, lq, lk, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev);
  x.dout_stride = h * D;
  return GMLM_OK;
}

}  // namespace d128
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::d128;

#define GMLM_D128_LAUNCH(KERNEL, grid, st, prm)                                                             \
  do {                                                                                                      \
    const bool dr_ = (prm).a.drop_thresh != 0;                                                              \
    if (dtype == GMLM_BF16) {                                                                               \
      if (dr_) KERNEL<bf16_t, true><<<grid, NT, 0, st>>>(prm);                                              \
      else KERNEL<bf16_t, false><<<grid, NT, 0, st>>>(prm);                                                 \
    } else {                                                                                                \
      if (dr_) KERNEL<float, true><<<grid, NT, 0, st>>>(prm);                                               \
      else KERNEL<float, false><<<grid, NT, 0, st>>>(prm);                                                  \
    }                                                                                                       \
  } while (0)

extern "C" int gmlm_attention_d128_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                                       int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                       float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* out,
                                       void* out_lo, float* lse, int dtype, gmlm_stream_t stream) {
  static const char* who = "attention_d128_fwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, h * D, h * D, dtype)) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(cdiv(lq, BQ) * b * h));
  GMLM_D128_LAUNCH(fwd_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_d128_workspace_bytes(int64_t b, int64_t h, int64_t lq) {
  return attn_delta_bytes(b, h, lq);
}

extern "C" int gmlm_attention_d128_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                       const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t h,
                                       int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                       float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* dq, void* dk,
                                       void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                       void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "attention_d128_bwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || (lq == 0 && lk == 0)) return GMLM_OK;
  GMLM_REQUIRE(lq > 0 && lk > 0, "%s: empty query or key set with a non-empty counterpart is not supported", who);
  AttnParams& p = x.a;
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, p, h * D, h * D, dtype, workspace_bytes, attn_delta_bytes(b, h, lq))) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t rows = b * lq * h;
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, rows, dtype == GMLM_BF16 ? 16 : 32, st, lq, h);
  GMLM_LAUNCH_CHECK();
  const dim3 gq((unsigned)(cdiv(lq, BQ) * b * h));
  GMLM_D128_LAUNCH(dq_kernel, gq, st, x);
  GMLM_LAUNCH_CHECK();
  const dim3 gk((unsigned)(cdiv(lk, BQ) * b * h));
  GMLM_D128_LAUNCH(dkv_kernel, gk, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
