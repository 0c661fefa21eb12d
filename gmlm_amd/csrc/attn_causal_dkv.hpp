// dK / dV of attention with grouped KV heads: the loop nest shared by causal128::dkv_kernel (attn_causal.hip, D = 128),
// gqa::causal64_dkv_kernel (attn_gqa.hip, D = 64) and, with CAUSAL = false, bidir::gqa_dkv_kernel (attn_bidir.hip, D = 64 / 128).
// One text for both head dims and both masks, as the streaming bodies of attn_stream.hpp are.
// A workgroup owns NW * 32 keys (32 per wave) of one (sequence, KV head); for each query head of the group, in order, it walks
// the query tiles of 32 from the one holding its first key (CAUSAL = false: from the first) to the end of the sequence and
// accumulates into the same registers: no atomics, no expanded K / V or dK / dV in HBM, every sum in a fixed order.  Every wave
// reaches every barrier: a wave whose keys lie past kv_len still stages Q / dO.  bf16: lse, delta and the kv_len mask ride in
// one extra contraction step; the causal mask is not rank-1, so the diagonal block selects P = 0 explicitly before dS.
#pragma once
#include "attn_common.hpp"

namespace gmlm {

// work item of the 1-D dK/dV grid -> key tile, sequence, KV head, and the rows of that sequence: padded, sequence b owns rows
// [b * lq, (b + 1) * lq); packed, rows [cu[b], cu[b + 1]) of lq = T rows in all (block-uniform)
struct CausalKeyTile { int64_t kt, b, kvh, base, l; };
__device__ __forceinline__ CausalKeyTile causal_key_tile(const AttnParams& p, int group) {
  const int64_t hkv = p.h / group, pairs = p.b * hkv, item = blockIdx.x;
  const int64_t bh = item % pairs;
  CausalKeyTile it{item / pairs, bh / hkv, bh % hkv, (bh / hkv) * p.lq, p.lq};
  if (p.cu) { it.base = p.cu[it.b]; it.l = p.cu[it.b + 1] - it.base; }
  return it;
}

// p.h = query heads; `group` = query heads per KV head; dout_stride = row stride of dO; kvlen = the sequence's kv_len clamped
// into [0, it.l] by the caller
template <typename T, int D, int NW, int QT, bool DBUF, bool CAUSAL = true>
__device__ __forceinline__ void causal_dkv_body(const AttnParams& p, int64_t dout_stride, int group, const CausalKeyTile& it,
                                                int64_t kvlen) {
  constexpr int NT = NW * 64, BQ = NW * 32;
  constexpr int PITCH = D + Pad<T>::v, DB = D / 32, NBUF = DBUF ? 2 : 1;
  static_assert(QT == 32, "the diagonal test below is written for one 32-query block per tile");
  __shared__ __attribute__((aligned(16))) T qs[NBUF][QT * PITCH];
  __shared__ __attribute__((aligned(16))) T dos[NBUF][QT * PITCH];
  __shared__ __attribute__((aligned(16))) float lse_s[NBUF][QT];
  __shared__ __attribute__((aligned(16))) float dl_s[NBUF][QT];
  constexpr bool FOLD = sizeof(T) == 2;
  __shared__ __attribute__((aligned(16))) bf16_t ext_s[FOLD ? NBUF : 1][FOLD ? QT * 16 : 8];
  __shared__ __attribute__((aligned(16))) bf16_t ext_d[FOLD ? NBUF : 1][FOLD ? QT * 16 : 8];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t kvh = it.kvh, b = it.b, base = it.base, l_ = it.l;
  const int64_t k_tile0 = it.kt * BQ;
  if (k_tile0 >= l_) return;                // also a packed sequence of length 0: before any operand load
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
    const int t0 = CAUSAL ? (int)(k_tile0 / QT) : 0, ntiles = (int)((l_ + QT - 1) / QT);    // t0 < ntiles since k_tile0 < l_
    TileRegs<T, D, QT, NT> qr, dor;
    qr.init(p.q_stride, tid);
    dor.init(dout_stride, tid);
    for (int g = 0; g < group; ++g) {
      const int64_t hd = kvh * group + g;
      const int64_t lse_base = p.cu ? hd * p.lq + base : (b * p.h + hd) * p.lq;   // [hq, T] or [b, hq, l], as seq_view()
      const T* qg = static_cast<const T*>(p.q) + base * p.q_stride + hd * D;
      const T* dog = static_cast<const T*>(p.dout) + base * dout_stride + hd * D;
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
      dor.load(dog, dout_stride, (int64_t)t0 * QT, l_, tid);
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
          dor.load(dog, dout_stride, q0 + QT, l_, tid);
          load_small(q0 + QT);
        }
        // CAUSAL: query blocks before this wave's keys are fully masked for it (q0 and k_wave0 are multiples of 32)
        if (wave_live && (!CAUSAL || q0 >= k_wave0)) {
          const bool diag = CAUSAL && q0 == k_wave0;          // wave-uniform
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
              if (diag) pr = (int)q0 + acc_row(i, h) >= ki ? pr : 0.f;     // select: see attn_dq_body
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
          dor.load(dog, dout_stride, q0 + QT, l_, tid);
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

}  // namespace gmlm
