// Causal attention with grouped KV heads at head dim 128, forward + backward, gfx950 MFMA (gmlm_attention_causal_d128_*):
// the self-attention of a Qwen3-geometry text encoder (hq query heads share hkv KV heads, query i sees keys 0..i of its own
// sequence and, of those, the ones below kv_len).  Padded layout [b, l, heads, 128] with per-operand row strides, so the
// fused [q | k | v] projection output is read (and its gradient written) without copies; or packed layout [T, heads, 128]
// (gmlm_attention_causal_d128_varlen_*): the same kernels with AttnParams::cu set, sequence i = rows [cu[i], cu[i + 1]).
// Forward and dQ ARE the streaming bodies of attn_stream.hpp, instantiated with their CAUSAL and GQA template flags (defaults
// false: the existing kernels' code objects are unchanged, profiles/attn_causal_static.json) at the tiling of attn_d128.hip
// (4 waves, 128 query rows per workgroup, bf16: 64-row K / V tiles double-buffered, fp32: 32-row tiles in one buffer); delta is
// the shared delta body.  dK/dV has a loop nest of its own (an outer loop over the query heads of a KV head, a start tile, a
// barrier between heads) and is written out here on the helpers of attn_common.hpp (DESIGN.md section 4 "Qwen3 encoder").
//  * tiles wholly below the diagonal take the compare-free path of the non-causal kernels (block- or wave-uniform test);
//    only tiles that touch the diagonal compare key <= query per element (and key < kv_len);
//  * every wave reaches every barrier: a wave whose rows lie above a tile still stages K / V;
//  * key 0 is valid for every query and a wave only computes tiles whose first key is <= its first query, so every row of a
//    computing wave has a valid key in every tile it computes: the running max is finite, -inf - (-inf) never occurs;
//  * bf16 backward: lse, delta and the kv_len mask ride in one extra contraction step as in the non-causal kernels; the
//    causal mask is not rank-1, so diagonal tiles select P = 0 explicitly before dS;
//  * dK/dV: a workgroup owns 128 keys of one KV head, walks the query heads of its group in order and, per head, the query
//    tiles from the diagonal on, accumulating into the same registers.  No atomics, no expanded K / V or dK / dV in HBM.
// The argument checks and the AttnParams filling shared with the other attention entry points are in attn_host.hpp.
#include "attn_stream.hpp"
#include "attn_host.hpp"

namespace gmlm {
namespace causal128 {

constexpr int D = 128, NW = 4, NT = NW * 64, BQ = NW * 32;

struct Params {
  AttnParams a;            // a.h = query heads; lse / delta are [b, hq, l]; a.lq == a.lk
  int64_t dout_stride;     // row stride of dO / O (= hq * 128)
  int32_t group;           // query heads per KV head (hq / hkv)
};

template <typename T> struct Cfg;
template <> struct Cfg<bf16_t> { static constexpr int KT = 64, QT = 32; static constexpr bool DBUF = true; };
template <> struct Cfg<float> { static constexpr int KT = 32, QT = 32; static constexpr bool DBUF = false; };

__device__ __forceinline__ int64_t clamp_kvlen(const AttnParams& p, int64_t b, int64_t lk_) {
  int64_t kvlen = lk_;
  if (p.kv_len) { kvlen = p.kv_len[b]; if (kvlen > lk_) kvlen = lk_; if (kvlen < 0) kvlen = 0; }
  return kvlen;
}

// work item of the 1-D grid -> (tile, batch, query head); tiles are outermost
struct Item { int64_t tile, b, hd; };
__device__ __forceinline__ Item decode(const AttnParams& p) {
  const int64_t pairs = p.b * p.h, item = blockIdx.x;
  const int64_t bh = item % pairs;
  return {item / pairs, bh / p.h, bh % p.h};
}

// forward: workgroup = 128 query rows of one (batch, query head); key tiles 0 .. the tile holding its last query
template <typename T>
__global__ __launch_bounds__(NT) void fwd_kernel(Params x) {
  const Item it = decode(x.a);
  attn_fwd_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, true, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

// backward: delta = rowsum(dO * O) over rows of [b * l, hq, 128]
template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                    int64_t rows /* b * l * hq */, int64_t lq, int64_t hn, float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);
}

// backward: dQ.  workgroup = 128 queries of one (batch, query head), key tiles up to the diagonal.  Without dropout the shared
// body keeps its register budget at D = 128 (d128::dq_kernel's own copy exists for the dropout instantiation).
template <typename T>
__global__ __launch_bounds__(NT) void dq_kernel(Params x) {
  const Item it = decode(x.a);
  attn_dq_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, true, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

// backward: dK, dV.  workgroup = 128 keys (32 per wave) of one (batch, KV head); for each query head of the group, in order,
// the query tiles of 32 from the one holding the workgroup's first key to the end of the sequence.
template <typename T>
__global__ __launch_bounds__(NT) void dkv_kernel(Params x) {
  const AttnParams& p = x.a;
  constexpr bool DBUF = Cfg<T>::DBUF;
  constexpr int QT = Cfg<T>::QT, PITCH = D + Pad<T>::v, DB = D / 32, NBUF = DBUF ? 2 : 1;
  static_assert(QT == 32, "the diagonal test below is written for one 32-query block per tile");
  __shared__ __attribute__((aligned(16))) T qs[NBUF][QT * PITCH];
  __shared__ __attribute__((aligned(16))) T dos[NBUF][QT * PITCH];
  __shared__ __attribute__((aligned(16))) float lse_s[NBUF][QT];
  __shared__ __attribute__((aligned(16))) float dl_s[NBUF][QT];
  constexpr bool FOLD = sizeof(T) == 2;
  __shared__ __attribute__((aligned(16))) bf16_t ext_s[FOLD ? NBUF : 1][FOLD ? QT * 16 : 8];
  __shared__ __attribute__((aligned(16))) bf16_t ext_d[FOLD ? NBUF : 1][FOLD ? QT * 16 : 8];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t hkv = p.h / x.group, pairs = p.b * hkv, item = blockIdx.x;
  const int64_t kt = item / pairs, bh = item % pairs;
  const int64_t b = bh / hkv, kvh = bh % hkv;
  // padded: sequence b owns rows [b * lq, (b + 1) * lq); packed: rows [cu[b], cu[b + 1]) of lq = T rows in all (block-uniform)
  int64_t l_ = p.lq, base = b * p.lq;
  if (p.cu) { base = p.cu[b]; l_ = p.cu[b + 1] - base; }
  const int64_t k_tile0 = kt * BQ;
  if (k_tile0 >= l_) return;                // also a packed sequence of length 0: before any operand load
  const int64_t kvlen = clamp_kvlen(p, b, l_);
  const int64_t k_wave0 = k_tile0 + w * 32, key = k_wave0 + r;
  const bool key_in = key < l_;            // row exists in memory
  const bool key_ok = key < kvlen;         // takes part in the softmax
  const bool wave_live = k_wave0 < kvlen;  // else: staging helper only (dK = dV = 0)
  const int64_t kr_ = key_in ? key : 0;
  const int ki = (int)(key < (1 << 30) ? key : (1 << 30));
  RowFrag<T, D> kf, vf;
  kf.load(static_cast<const T*>(p.k) + (base + kr_) * p.k_stride + kvh * D, key_in, h);
  vf.load(static_cast<const T*>(p.v) + (base + kr_) * p.v_stride + kvh * D, key_in, h);
  const float sl2 = p.scale * kLog2e;
  bf16x8 ones_k, ones_2;
  if constexpr (FOLD) {
#pragma unroll
    for (int s_ = 0; s_ < D / 16; ++s_)
#pragma unroll
      for (int j = 0; j < 8; ++j) kf.v[s_][j] = (__bf16)((float)kf.v[s_][j] * sl2);
#pragma unroll
    for (int j = 0; j < 8; ++j) { ones_k[j] = (__bf16)0.f; ones_2[j] = (__bf16)0.f; }
    if (h == 0) {
      ones_k[0] = ones_2[0] = (__bf16)1.f; ones_k[1] = ones_2[1] = (__bf16)1.f;
      ones_k[2] = key_ok ? (__bf16)0.f : (__bf16)1.f;        // this lane's key is past kv_len: its scores get -2^100
    }
  }
  f32x16 dk[DB], dv[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk[d][i] = 0.f; dv[d][i] = 0.f; }
  if (k_tile0 < kvlen) {                                     // block-uniform: else nothing to accumulate
    const int t0 = (int)(k_tile0 / QT), ntiles = (int)((l_ + QT - 1) / QT);    // t0 < ntiles since k_tile0 < l_
    TileRegs<T, D, QT, NT> qr, dor;
    qr.init(p.q_stride, tid);
    dor.init(x.dout_stride, tid);
    for (int g = 0; g < x.group; ++g) {
      const int64_t hd = kvh * x.group + g;
      const int64_t lse_base = p.cu ? hd * p.lq + base : (b * p.h + hd) * p.lq;   // [hq, T] or [b, hq, l], as seq_view()
      const T* qg = static_cast<const T*>(p.q) + base * p.q_stride + hd * D;
      const T* dog = static_cast<const T*>(p.dout) + base * x.dout_stride + hd * D;
      const float* lse_g = p.lse + lse_base;
      const float* dl_g = p.delta + lse_base;
      float lr = 0.f, dr = 0.f;
      auto load_small = [&](int64_t q0) {
        if (tid < QT) {
          const bool ok = q0 + tid < l_;
          lr = ok ? lse_g[q0 + tid] * kLog2e : INFINITY;     // +inf: probability 0 for a row past the sequence
          dr = ok ? dl_g[q0 + tid] : 0.f;
        }
      };
      auto store_small = [&](int buf) {
        if (tid < QT) {
          lse_s[buf][tid] = lr; dl_s[buf][tid] = dr;
          if constexpr (FOLD) {
            const float l2 = lr < 0x1p100f ? lr : 0x1p100f;
            const float lh = (float)(__bf16)l2, ll = (float)(__bf16)(l2 - lh);
            const float dh = (float)(__bf16)dr, dlo = (float)(__bf16)(dr - dh);
            bf16x8 es, ed, z;
#pragma unroll
            for (int j = 0; j < 8; ++j) { es[j] = (__bf16)0.f; ed[j] = (__bf16)0.f; z[j] = (__bf16)0.f; }
            es[0] = (__bf16)(-lh); es[1] = (__bf16)(-ll); es[2] = (__bf16)(-0x1p100f);
            ed[0] = (__bf16)(-dh); ed[1] = (__bf16)(-dlo);
            *reinterpret_cast<bf16x8*>(&ext_s[buf][tid * 16]) = es;
            *reinterpret_cast<bf16x8*>(&ext_s[buf][tid * 16 + 8]) = z;
            *reinterpret_cast<bf16x8*>(&ext_d[buf][tid * 16]) = ed;
            *reinterpret_cast<bf16x8*>(&ext_d[buf][tid * 16 + 8]) = z;
          }
        }
      };
      if (g > 0) __syncthreads();                            // the previous head's last tile may still be read (block-uniform)
      qr.load(qg, p.q_stride, (int64_t)t0 * QT, l_, tid);
      dor.load(dog, x.dout_stride, (int64_t)t0 * QT, l_, tid);
      load_small((int64_t)t0 * QT);
      qr.store(qs[0], tid);
      dor.store(dos[0], tid);
      store_small(0);
      __syncthreads();
      for (int t = t0; t < ntiles; ++t) {
        const int64_t q0 = (int64_t)t * QT;
        const int cur = DBUF ? ((t - t0) & 1) : 0;
        const bool more = t + 1 < ntiles;
        if (DBUF && more) {
          qr.load(qg, p.q_stride, q0 + QT, l_, tid);
          dor.load(dog, x.dout_stride, q0 + QT, l_, tid);
          load_small(q0 + QT);
        }
        // query blocks before this wave's keys are fully masked for it (q0 and k_wave0 are multiples of 32)
        if (wave_live && q0 >= k_wave0) {
          const bool diag = q0 == k_wave0;                    // wave-uniform
          f32x16 s, dp;
#pragma unroll
          for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
          if constexpr (FOLD) {
            const bf16x8 ea = *reinterpret_cast<const bf16x8*>(&ext_s[cur][r * 16 + 8 * h]);   // A row r = query r of the block
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ea, ones_k, s, 0, 0, 0);
            const bf16x8 da = *reinterpret_cast<const bf16x8*>(&ext_d[cur][r * 16 + 8 * h]);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(da, ones_2, dp, 0, 0, 0);
          }
          mma_rows<D>(qs[cur], PITCH, 0, kf, s, r, h);
          mma_rows<D>(dos[cur], PITCH, 0, vf, dp, r, h);
          if constexpr (FOLD) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
              float pr = fast_exp2(s[i]);
              if (diag) pr = (int)q0 + acc_row(i, h) >= ki ? pr : 0.f;     // select: see dq_kernel
              s[i] = pr;
              dp[i] = pr * dp[i];
            }
          } else {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
              const int q4 = 8 * g4 + 4 * h;                 // accumulator registers 4*g4 .. 4*g4+3 = queries q4 .. q4+3
              const float4 l4 = *reinterpret_cast<const float4*>(&lse_s[cur][q4]);
              const float4 d4 = *reinterpret_cast<const float4*>(&dl_s[cur][q4]);
              const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv4[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int i = 4 * g4 + j;
                const bool on = key_ok && (!diag || (int)q0 + q4 + j >= ki);
                const float pr = fast_exp2(on ? fmaf(s[i], sl2, -lv[j]) : -INFINITY);
                s[i] = pr;
                dp[i] = pr * (dp[i] - dv4[j]);
              }
            }
          }
          mma_acc<D>(dos[cur], PITCH, 0, s, dv, lane);
          mma_acc<D>(qs[cur], PITCH, 0, dp, dk, lane);
        }
        if (DBUF) {
          if (more) {
            qr.store(qs[cur ^ 1], tid);
            dor.store(dos[cur ^ 1], tid);
            store_small(cur ^ 1);
          }
          __syncthreads();
        } else if (more) {
          __syncthreads();
          qr.load(qg, p.q_stride, q0 + QT, l_, tid);
          dor.load(dog, x.dout_stride, q0 + QT, l_, tid);
          load_small(q0 + QT);
          qr.store(qs[0], tid);
          dor.store(dos[0], tid);
          store_small(0);
          __syncthreads();
        }
      }
    }
  }
  if (key_in) {
    T* dkg = static_cast<T*>(p.dk) + (base + key) * p.dk_stride + kvh * D;
    T* dvg = static_cast<T*>(p.dv) + (base + key) * p.dv_stride + kvh * D;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      store_t<T>(dkg + d * 32, dk[d], p.scale, h);
      store_t<T>(dvg + d * 32, dv[d], 1.f, h);
    }
  }
}

// the checks of attn_host.hpp up to the empty-problem return, with this family's head dim, layout rules and work-item bound;
// fills the launch parameters.  sizes_ok: what the entry point adds to the size test (the varlen entries' own bounds)
static int setup(const char* who, Params& x, const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b,
                 int64_t hq, int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                 float scale, float dropout_p, const void* out_lo, int dtype, bool sizes_ok = true) {
  int rc = attn_check_shape(who, sizes_ok && b >= 0 && hq > 0 && hkv > 0 && lq >= 0 && lk >= 0, d == 128, d, "this entry point takes 128",
                            dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(lq == lk, "%s: causal self-attention needs lq == lk (got %ld and %ld)", who, (long)lq, (long)lk);
  GMLM_REQUIRE(hq % hkv == 0, "%s: %ld query heads are not a multiple of %ld KV heads", who, (long)hq, (long)hkv);
  if ((rc = attn_check_rates(who, dropout_p, false, scale)) != GMLM_OK) return rc;
  GMLM_REQUIRE(lq < ((int64_t)1 << 30) && cdiv(lq, BQ) * b * hq < ((int64_t)1 << 31), "%s: too many work items", who);
  x = Params{};
  attn_fill(x.a, q, k, v, kv_len, b, hq, lq, lk, q_stride, k_stride, v_stride, scale, 0.f, 0, nullptr);
  x.dout_stride = hq * D;
  x.group = (int32_t)(hq / hkv);
  return GMLM_OK;
}

// packed (varlen) layout: `seqs` sequences, sequence i = rows [cu[i], cu[i + 1]) of `rows` packed rows, none longer than
// max_len.  Same kernels with AttnParams::cu set: b = seqs, lq = lk = rows (lse / delta [hq, rows]); a tile past its
// sequence returns block-uniformly.
static int setup_varlen(const char* who, Params& x, const void* q, const void* k, const void* v, const int32_t* cu, int64_t seqs,
                        int64_t max_len, int64_t rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride, int64_t k_stride,
                        int64_t v_stride, float scale, float dropout_p, const void* out_lo, int dtype) {
  GMLM_REQUIRE(cu, "%s: null cu_seqlens", who);
  GMLM_REQUIRE(max_len > 0, "%s: max_len %ld must be positive", who, (long)max_len);
  GMLM_REQUIRE(seqs >= 0 && rows >= 0 && rows < ((int64_t)1 << 30), "%s: %ld packed rows (must be >= 0 and < 2^30)", who, (long)rows);
  int rc = setup(who, x, q, k, v, nullptr, 0, hq, hkv, 0, 0, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype,
                 max_len < ((int64_t)1 << 30) && seqs < ((int64_t)1 << 30));
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(cdiv(max_len, BQ) * seqs * hq < ((int64_t)1 << 31), "%s: too many work items", who);
  x.a.b = seqs; x.a.lq = x.a.lk = rows; x.a.cu = cu;
  return GMLM_OK;
}

}  // namespace causal128
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::causal128;

#define GMLM_CAUSAL_LAUNCH(KERNEL, grid, st, prm)                         \
  do {                                                                    \
    if (dtype == GMLM_BF16) KERNEL<bf16_t><<<grid, NT, 0, st>>>(prm);     \
    else KERNEL<float><<<grid, NT, 0, st>>>(prm);                         \
  } while (0)

extern "C" int gmlm_attention_causal_d128_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b,
                                              int64_t hq, int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride,
                                              int64_t k_stride, int64_t v_stride, float scale, float dropout_p, void* out,
                                              void* out_lo, float* lse, int dtype, gmlm_stream_t stream) {
  static const char* who = "attention_causal_d128_fwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, hq, hkv, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, hq * D, hkv * D, dtype)) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(cdiv(lq, BQ) * b * hq));
  GMLM_CAUSAL_LAUNCH(fwd_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_causal_d128_workspace_bytes(int64_t b, int64_t hq, int64_t lq) {
  return attn_delta_bytes(b, hq, lq);
}

extern "C" int gmlm_attention_causal_d128_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                              const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq,
                                              int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                              int64_t v_stride, float scale, float dropout_p, void* dq, void* dk, void* dv,
                                              int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                              size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "attention_causal_d128_bwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, hq, hkv, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  AttnParams& p = x.a;
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, p, hq * D, hkv * D, dtype, workspace_bytes, attn_delta_bytes(b, hq, lq))) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t rows = b * lq * hq;
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, rows, dtype == GMLM_BF16 ? 16 : 32, st, lq, hq);
  GMLM_LAUNCH_CHECK();
  const dim3 gq((unsigned)(cdiv(lq, BQ) * b * hq));
  GMLM_CAUSAL_LAUNCH(dq_kernel, gq, st, x);
  GMLM_LAUNCH_CHECK();
  const dim3 gk((unsigned)(cdiv(lk, BQ) * b * hkv));
  GMLM_CAUSAL_LAUNCH(dkv_kernel, gk, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" int gmlm_attention_causal_d128_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                                     int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq,
                                                     int64_t hkv, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                                     float scale, float dropout_p, void* out, void* out_lo, float* lse, int dtype,
                                                     gmlm_stream_t stream) {
  static const char* who = "attention_causal_d128_varlen_fwd";
  Params x;
  int rc = setup_varlen(who, x, q, k, v, cu_seqlens, num_seqs, max_len, total_rows, hq, hkv, d, q_stride, k_stride, v_stride, scale,
                        dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (num_seqs == 0 || total_rows == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, hq * D, hkv * D, dtype)) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(cdiv(max_len, BQ) * num_seqs * hq));
  GMLM_CAUSAL_LAUNCH(fwd_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_causal_d128_varlen_workspace_bytes(int64_t total_rows, int64_t hq) {
  return attn_delta_bytes(1, hq, total_rows);   // delta [hq, total_rows]
}

extern "C" int gmlm_attention_causal_d128_varlen_bwd(const void* q, const void* k, const void* v, const void* out,
                                                     const void* out_lo, const void* dout, const float* lse,
                                                     const int32_t* cu_seqlens, int64_t num_seqs, int64_t max_len,
                                                     int64_t total_rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride,
                                                     int64_t k_stride, int64_t v_stride, float scale, float dropout_p, void* dq,
                                                     void* dk, void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride,
                                                     int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "attention_causal_d128_varlen_bwd";
  Params x;
  int rc = setup_varlen(who, x, q, k, v, cu_seqlens, num_seqs, max_len, total_rows, hq, hkv, d, q_stride, k_stride, v_stride, scale,
                        dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (num_seqs == 0 || total_rows == 0) return GMLM_OK;
  AttnParams& p = x.a;
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, p, hq * D, hkv * D, dtype, workspace_bytes, attn_delta_bytes(1, hq, total_rows))) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t rows = total_rows * hq;                         // delta as one sequence of total_rows: [hq, total_rows]
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, rows, dtype == GMLM_BF16 ? 16 : 32, st, total_rows, hq);
  GMLM_LAUNCH_CHECK();
  const dim3 gq((unsigned)(cdiv(max_len, BQ) * num_seqs * hq));
  GMLM_CAUSAL_LAUNCH(dq_kernel, gq, st, x);
  GMLM_LAUNCH_CHECK();
  const dim3 gk((unsigned)(cdiv(max_len, BQ) * num_seqs * hkv));
  GMLM_CAUSAL_LAUNCH(dkv_kernel, gk, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
