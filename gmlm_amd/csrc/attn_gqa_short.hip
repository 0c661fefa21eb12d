// LDS-resident short-sequence attention with grouped KV heads (bf16, d = 64, packed layout with seq_groups), forward and
// backward, bidirectional or causal, gfx950 MFMA: gmlm_attention_gqa_short_* (C ABI in include/gmlm_hip_gqa_short.h), all in
// namespace gmlm::gqas.  The grouped form of attn_short.hip, for the Llama / Qwen2 / Mistral encoders (causal) and EuroBERT
// (bidirectional) on batches of sequences of <= 128 tokens.
//
// A work item is a GROUP of consecutive sequences of the packed batch (<= 13 sequences, <= R rows), so a workgroup stages full
// tiles from one contiguous row range.  Attention stays inside a sequence through the block-diagonal mask step of
// attn_short.hpp (one extra contraction step at the head of every score chain, no VALU work) and a wave-uniform range of
// 32-row blocks.  CAUSAL: inside a group, tile-row order is position order within each sequence, so "key position <= query
// position" is "key tile row <= query tile row" on top of the block-diagonal mask: blocks on the far side of the wave's own
// block are skipped, blocks on the near side run compare-free, and the diagonal block alone takes a select.
//
// Forward: one work item per (group, query head); K / V of KV head h / (hq / hkv).  The query heads of a KV head are adjacent
// work items, so their K / V reads after the first come from L2.
// Backward: ONE launch, one work item per (group, KV head).  K and V are staged once; then for each query head of the KV head,
// in order: stage Q, dO and lse | phase 1 (query on the lane): P and dP of all key blocks in registers, delta in fp32 from
// them, dS, dQ stored | phase 2 (key on the lane): dK, dV accumulate in the SAME registers over the heads.  dK / dV are stored
// once after the last head: a fixed-order sum over (query head, query row), no atomics, no per-head partials in HBM, no
// expanded K / V, no delta pass and no read of the forward output.
#include "attn_short.hpp"
#include "attn_host.hpp"
#include "../../include/gmlm_hip_gqa_short.h"

namespace gmlm {
namespace gqas {

constexpr int D = 64;
constexpr float kMasked = -1.2676506e30f;   // -2^100, the value of the block-diagonal mask step: exp2 of it is exactly 0

struct Params {
  AttnParams a;       // a.h = query heads, a.lq = total rows (lse is [hq, total_rows]), a.cu / a.groups set
  int32_t group;      // query heads per KV head (hq / hkv)
  int32_t hkv;
};

// ------------------------------------------------------------------------------------------------
// forward: attn_fwd_short_kernel (attn_short.hip) with K / V of the query head's KV head
// ------------------------------------------------------------------------------------------------
template <bool CAUSAL, int R>
__global__ __launch_bounds__(2 * R, 4) void fwd_kernel(Params x) {
  using T = bf16_t;
  const AttnParams& p = x.a;
  constexpr int NT = 2 * R, PITCH = D, DB = D / 32, CPR = D / 8, PER = R * CPR / NT, NB = R / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tk = reinterpret_cast<T*>(smem_raw);
  T* tv = tk + R * PITCH;
  ShortMeta mt;
  mt.q2k_lo = reinterpret_cast<int16_t*>(tv + R * PITCH);
  mt.q2k_hi = mt.q2k_lo + R; mt.k2q_lo = mt.q2k_hi + R; mt.k2q_hi = mt.k2q_lo + R;
  mt.qid = reinterpret_cast<uint8_t*>(mt.k2q_hi + R);
  mt.kid = mt.qid + R;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t item = blockIdx.x / p.h, hd = blockIdx.x % p.h, kvh = hd / x.group;
  int64_t qbase, kbase, lse_base;
  int nq, nk;
  short_item_setup<R>(p, item, tid, mt, qbase, kbase, nq, nk, lse_base, hd);
  const T* qg = static_cast<const T*>(p.q) + qbase * p.q_stride + hd * D;
  const T* kg = static_cast<const T*>(p.k) + kbase * p.k_stride + kvh * D;
  const T* vg = static_cast<const T*>(p.v) + kbase * p.v_stride + kvh * D;
  const int q_row = w * 32 + r;
  RowFrag<T, D> qf;
  qf.load(qg + (uint32_t)((q_row < nq ? q_row : 0) * (int)p.q_stride), q_row < nq, h);
  uint4 rk[PER], rv[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = tid + k * NT, row = i / CPR, col = (i % CPR) * 8;
    rk[k] = rv[k] = make_uint4(0, 0, 0, 0);
    if (row < nk) {
      rk[k] = *reinterpret_cast<const uint4*>(kg + (uint32_t)(row * (int)p.k_stride + col));
      rv[k] = *reinterpret_cast<const uint4*>(vg + (uint32_t)(row * (int)p.v_stride + col));
    }
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int i = tid + k * NT, row = i / CPR;
    const int c = i % CPR;                                      // 16-byte chunk of the row -> swizzled slot (attn_common.hpp)
    *reinterpret_cast<uint4*>(tk + row * PITCH + ((c ^ sw_row(row)) << 3)) = rk[k];
    *reinterpret_cast<uint4*>(tv + row * PITCH + ((c ^ sw_tr(row)) << 3)) = rv[k];
  }
  __syncthreads();
  if (w * 32 >= nq) return;                                   // (no barrier below)
  const bf16x8 qm = antihot_frag(mt.qid[q_row], h);
  int b0, b1;
  block_range(mt.q2k_lo, mt.q2k_hi, w, nq, b0, b1);           // key blocks that hold a key of this wave's sequences
  if (CAUSAL) b1 = b1 < w + 1 ? b1 : w + 1;                   // key blocks above the wave's own hold later positions only
  const float sl2 = p.scale * kLog2e;
  f32x16 s[NB];
  float rmax = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) {
    if (kb < b0 || kb >= b1) continue;
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.f;
    s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(onehot_frag(mt.kid[kb * 32 + r], h), qm, z, 0, 0, 0);   // block-diagonal mask
    mma_rows_sw(tk, kb * 32, qf, s[kb], r, h);
    if (CAUSAL && kb == w) {                                  // the diagonal block: key tile row <= query tile row
#pragma unroll
      for (int i = 0; i < 16; ++i) s[kb][i] = acc_row(i, h) <= r ? s[kb][i] : kMasked;
    }
    rmax = fmaxf(rmax, max16(s[kb]));
  }
  const float m = b1 > b0 ? xhalf_max(rmax) * sl2 : 0.f;      // finite for a real query row (it sees at least itself / its sequence)
  f32x16 o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[d][i] = 0.f;
  float l = 0.f;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) {
    if (kb < b0 || kb >= b1) continue;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      const float e0 = fast_exp2(fmaf(s[kb][i], sl2, -m)), e1 = fast_exp2(fmaf(s[kb][i + 1], sl2, -m));   // masked: exp2(-2e29) = 0
      l += e0 + e1;
      s[kb][i] = e0;
      s[kb][i + 1] = e1;
    }
    mma_acc_sw(tv, kb * 32, s[kb], o, lane);
  }
  l = xhalf_sum(l);
  if (q_row < nq) {
    const float inv = l > 0.f ? 1.f / l : 0.f;
    T* og = static_cast<T*>(p.o_w) + ((qbase + q_row) * p.h + hd) * D;
#pragma unroll
    for (int d = 0; d < DB; ++d) store_t<T>(og + d * 32, o[d], inv, h);
    if (h == 0 && p.lse_w) p.lse_w[lse_base + q_row] = l > 0.f ? (m + __log2f(l)) * kLn2 : -INFINITY;
  }
}

// ------------------------------------------------------------------------------------------------
// backward: one work item per (group, KV head), looping over the query heads of the KV head
// ------------------------------------------------------------------------------------------------
// Waves per SIMD the register allocation is bounded for (the second __launch_bounds__ argument).  dK / dV (64 accumulator
// registers) live across the heads on top of phase 1's P and dP of every key block, dQ and the row fragments: from R = 64 on
// the compiler does not fit that into the 256 registers of two waves per SIMD and spills to scratch.  So R >= 64 is bounded
// for one wave per SIMD (the whole 512-register file; at R = 128 one workgroup per CU) and R = 32 for two.  Parking dK / dV in
// LDS between heads instead (64 KB beside the 74 KB of tiles at R = 128: one workgroup per CU as well) measured 4-5 % slower
// (DESIGN.md section 4 has the table and the numbers).
template <bool CAUSAL, int R>
__global__ __launch_bounds__(2 * R, R >= 64 ? 1 : 2) void bwd_kernel(Params x) {
  using T = bf16_t;
  const AttnParams& p = x.a;
  constexpr int NT = 2 * R, PITCH = D + Pad<T>::v, DB = D / 32, CPR = D / 8, PER = R * CPR / NT, NB = R / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tk = reinterpret_cast<T*>(smem_raw);
  T* tv = tk + R * PITCH;
  T* tq = tv + R * PITCH;
  T* tdo = tq + R * PITCH;
  float* lse_s = reinterpret_cast<float*>(tdo + R * PITCH);
  float* dl_s = lse_s + R;
  ShortMeta mt;
  mt.q2k_lo = reinterpret_cast<int16_t*>(dl_s + R);
  mt.q2k_hi = mt.q2k_lo + R; mt.k2q_lo = mt.q2k_hi + R; mt.k2q_hi = mt.k2q_lo + R;
  mt.qid = reinterpret_cast<uint8_t*>(mt.k2q_hi + R);
  mt.kid = mt.qid + R;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t item = blockIdx.x / x.hkv, kvh = blockIdx.x % x.hkv;
  const int64_t hd0 = kvh * x.group;                         // first query head of this KV head
  int64_t qbase, kbase, row0;
  int nq, nk;
  short_item_setup<R>(p, item, tid, mt, qbase, kbase, nq, nk, row0, 0);      // lse base of head 0 = first row of the item
  const int n = nq;                                          // packed self-attention: nq == nk
  const T* qg = static_cast<const T*>(p.q) + qbase * p.q_stride + hd0 * D;
  const T* kg = static_cast<const T*>(p.k) + kbase * p.k_stride + kvh * D;
  const T* vg = static_cast<const T*>(p.v) + kbase * p.v_stride + kvh * D;
  const T* dog = static_cast<const T*>(p.dout) + (qbase * p.h + hd0) * D;
  const int do_stride = (int)(p.h * D);
  // ---- K, V: staged once (32-bit offsets: rows <= 128, strides < 2^24) ----
  {
    uint4 rk[PER], rv[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * NT, row = i / CPR, col = (i % CPR) * 8;
      rk[k] = rv[k] = make_uint4(0, 0, 0, 0);
      if (row < n) {
        rk[k] = *reinterpret_cast<const uint4*>(kg + (uint32_t)(row * (int)p.k_stride + col));
        rv[k] = *reinterpret_cast<const uint4*>(vg + (uint32_t)(row * (int)p.v_stride + col));
      }
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * NT, row = i / CPR, col = (i % CPR) * 8;
      *reinterpret_cast<uint4*>(tk + row * PITCH + col) = rk[k];
      *reinterpret_cast<uint4*>(tv + row * PITCH + col) = rv[k];
    }
  }
  // Q, dO and lse of query head hd0 + g: global -> registers, registers -> LDS (the loads of head g + 1 are issued before
  // phase 2 of head g and land in LDS behind its closing barrier)
  uint4 rq[PER], rdo[PER];
  float rl = INFINITY;
  auto head_load = [&](int g) {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * NT, row = i / CPR, col = (i % CPR) * 8;
      rq[k] = rdo[k] = make_uint4(0, 0, 0, 0);
      if (row < n) {
        rq[k] = *reinterpret_cast<const uint4*>(qg + (uint32_t)(row * (int)p.q_stride + g * D + col));
        rdo[k] = *reinterpret_cast<const uint4*>(dog + (uint32_t)(row * do_stride + g * D + col));
      }
    }
    // +inf: a row past the item gets probability 0
    if (tid < R) rl = tid < n ? p.lse[(hd0 + g) * p.lq + row0 + tid] * kLog2e : INFINITY;
  };
  auto head_store = [&]() {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = tid + k * NT, row = i / CPR, col = (i % CPR) * 8;
      *reinterpret_cast<uint4*>(tq + row * PITCH + col) = rq[k];
      *reinterpret_cast<uint4*>(tdo + row * PITCH + col) = rdo[k];
    }
    if (tid < R) lse_s[tid] = rl;
  };
  auto frag = [&](const T* tile, int row, RowFrag<T, D>& f) {          // MFMA B-operand fragment of a staged row
#pragma unroll
    for (int s = 0; s < D / 16; ++s) f.v[s] = *reinterpret_cast<const bf16x8*>(tile + row * PITCH + 16 * s + 8 * h);
  };
  const float sl2 = p.scale * kLog2e;
  const bool active = w * 32 < n;                            // wave-uniform: a wave whose rows lie past the item stages and skips the math
  const int row = w * 32 + r;                                // the lane's query row (phase 1) and key row (phase 2)
  f32x16 dk[DB], dv[DB];                                     // accumulate over the query heads of this KV head
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) { dk[d][i] = 0.f; dv[d][i] = 0.f; }
  head_load(0);
  for (int g = 0; g < x.group; ++g) {
    head_store();
    __syncthreads();                                         // this head's Q, dO, lse (and, the first time, K, V and the meta arrays)
    // ---- phase 1: delta and dQ (query on the lane; K, V as MFMA A operands) -------------------------------
    if (active) {
      RowFrag<T, D> qf, dof;
      frag(tq, row, qf);
      frag(tdo, row, dof);
      const float lse2 = lse_s[row];
      const bf16x8 qm = antihot_frag(mt.qid[row], h);
      int b0, b1;
      block_range(mt.q2k_lo, mt.q2k_hi, w, n, b0, b1);
      if (CAUSAL) b1 = b1 < w + 1 ? b1 : w + 1;
      // pass A: P and dP of every key block, kept in registers; delta = sum_k P dP in fp32
      f32x16 pr[NB], dpm[NB];
      float dsum = 0.f;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) {
        if (kb < b0 || kb >= b1) continue;                    // wave-uniform
        f32x16 z;
#pragma unroll
        for (int i = 0; i < 16; ++i) { z[i] = 0.f; dpm[kb][i] = 0.f; }
        pr[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(onehot_frag(mt.kid[kb * 32 + r], h), qm, z, 0, 0, 0);
        mma_rows<D>(tk, PITCH, kb * 32, qf, pr[kb], r, h);
        mma_rows<D>(tv, PITCH, kb * 32, dof, dpm[kb], r, h);
        const bool diag = CAUSAL && kb == w;                  // wave-uniform
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float p0 = fast_exp2(fmaf(pr[kb][i], sl2, -lse2));  // other sequences' keys: exactly 0
          if (diag) p0 = acc_row(i, h) <= r ? p0 : 0.f;       // key tile row <= query tile row
          dsum = fmaf(p0, dpm[kb][i], dsum);
          pr[kb][i] = p0;
        }
      }
      const float dl = xhalf_sum(dsum);
      if (h == 0) dl_s[row] = dl;
      // pass B: dS = P (dP - delta); dQ^T += K^T dS^T
      f32x16 dq[DB];
#pragma unroll
      for (int d = 0; d < DB; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) dq[d][i] = 0.f;
#pragma unroll
      for (int kb = 0; kb < NB; ++kb) {
        if (kb < b0 || kb >= b1) continue;
#pragma unroll
        for (int i = 0; i < 16; ++i) pr[kb][i] *= dpm[kb][i] - dl;
        mma_acc<D>(tk, PITCH, kb * 32, pr[kb], dq, lane);
      }
      if (row < n) {
        T* dqg = static_cast<T*>(p.dq) + (qbase + row) * p.dq_stride + (hd0 + g) * D;
#pragma unroll
        for (int d = 0; d < DB; ++d) store_t<T>(dqg + d * 32, dq[d], p.scale, h);
      }
    } else if (lane < 32) {
      dl_s[w * 32 + lane] = 0.f;                             // rows past the item: never read with a non-zero probability
    }
    if (g + 1 < x.group) head_load(g + 1);                   // in flight during phase 2
    __syncthreads();                                         // delta of every query row is in LDS
    // ---- phase 2: dK, dV (key on the lane; Q, dO as MFMA A operands) -------------------------------------
    if (active) {
      int b0, b1;
      block_range(mt.k2q_lo, mt.k2q_hi, w, n, b0, b1);
      if (CAUSAL) b0 = b0 > w ? b0 : w;                       // query blocks below the wave's own hold earlier positions only
      if (b1 > b0) {
        RowFrag<T, D> kf, vf;
        frag(tk, row, kf);
        frag(tv, row, vf);
        const bf16x8 km = antihot_frag(mt.kid[row], h);
#pragma unroll
        for (int qb = 0; qb < NB; ++qb) {
          if (qb < b0 || qb >= b1) continue;                  // wave-uniform
          f32x16 s, dp, z;
#pragma unroll
          for (int i = 0; i < 16; ++i) { z[i] = 0.f; dp[i] = 0.f; }
          s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(onehot_frag(mt.qid[qb * 32 + r], h), km, z, 0, 0, 0);
          mma_rows<D>(tq, PITCH, qb * 32, kf, s, r, h);
          mma_rows<D>(tdo, PITCH, qb * 32, vf, dp, r, h);
          const bool diag = CAUSAL && qb == w;                // wave-uniform
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const int q4 = qb * 32 + 8 * g4 + 4 * h;           // accumulator registers 4*g4 .. 4*g4+3 = queries q4 .. q4+3
            const float4 l4 = *reinterpret_cast<const float4*>(lse_s + q4);
            const float4 d4 = *reinterpret_cast<const float4*>(dl_s + q4);
            const float lq4[4] = {l4.x, l4.y, l4.z, l4.w}, dq4[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int i = 4 * g4 + j;
              // rows past the item carry lse = +inf in LDS, other sequences' rows sit at -1.3e30: probability 0
              float p0 = fast_exp2(fmaf(s[i], sl2, -lq4[j]));
              if (diag) p0 = r <= acc_row(i, h) ? p0 : 0.f;    // key tile row <= query tile row
              s[i] = p0;
              dp[i] = p0 * (dp[i] - dq4[j]);
            }
          }
          mma_acc<D>(tdo, PITCH, qb * 32, s, dv, lane);
          mma_acc<D>(tq, PITCH, qb * 32, dp, dk, lane);
        }
      }
    }
    __syncthreads();                                         // every wave is done with this head's Q, dO, lse, delta
  }
  if (row < n) {
    T* dkg = static_cast<T*>(p.dk) + (kbase + row) * p.dk_stride + kvh * D;
    T* dvg = static_cast<T*>(p.dv) + (kbase + row) * p.dv_stride + kvh * D;
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      store_t<T>(dkg + d * 32, dk[d], p.scale, h);
      store_t<T>(dvg + d * 32, dv[d], 1.f, h);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static size_t fwd_lds(int r) { return (size_t)2 * r * 64 * sizeof(bf16_t) + (size_t)r * (4 * sizeof(int16_t) + 2); }
static size_t bwd_lds(int r) { return (size_t)4 * r * (64 + 8) * sizeof(bf16_t) + 2 * r * sizeof(float) + (size_t)r * (4 * sizeof(int16_t) + 2); }

// no group holds more rows than the batch has, nor more than 128: the tile height, a multiple of 32
static int tile_rows(int64_t total_rows) { return (int)((total_rows < 128 ? total_rows : 128) + 31) / 32 * 32; }

// Validation up to the nothing-to-do return, in the order of include/gmlm_hip_gqa_short.h; fills the launch parameters
static int setup(const char* who, Params& x, const void* q, const void* k, const void* v, const int32_t* cu, int64_t seqs,
                 int64_t max_len, int64_t rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride, int64_t k_stride,
                 int64_t v_stride, float scale, float dropout_p, int causal, const int32_t* groups, int64_t num_groups, int dtype) {
  GMLM_REQUIRE(seqs >= 0 && hq > 0 && hkv > 0, "%s: bad sizes", who);
  GMLM_REQUIRE(d == 64, "%s: head dim %ld not supported (this entry point takes 64)", who, (long)d);
  GMLM_REQUIRE(dtype == GMLM_BF16, "%s: unsupported dtype (the short-sequence grouped kernels take bf16)", who);
  GMLM_REQUIRE(hq % hkv == 0, "%s: %ld query heads are not a multiple of %ld KV heads", who, (long)hq, (long)hkv);
  GMLM_REQUIRE(dropout_p == 0.f, "%s: attention-probability dropout is not implemented for the grouped kernels (dropout_p must be 0)", who);
  GMLM_REQUIRE(scale > 0.f, "%s: scale must be positive", who);
  GMLM_REQUIRE(causal == 0 || causal == 1, "%s: causal must be 0 or 1 (got %d)", who, causal);
  GMLM_REQUIRE(cu, "%s: null cu_seqlens", who);
  GMLM_REQUIRE(groups, "%s: null seq_groups", who);
  GMLM_REQUIRE(num_groups >= 0, "%s: num_groups %ld must be >= 0", who, (long)num_groups);
  GMLM_REQUIRE(max_len > 0 && max_len <= 128, "%s: max_len %ld must be in 1..128", who, (long)max_len);
  GMLM_REQUIRE(rows >= 0 && rows < ((int64_t)1 << 30), "%s: %ld packed rows (must be >= 0 and < 2^30)", who, (long)rows);
  GMLM_REQUIRE(num_groups <= (((int64_t)1 << 31) - 1) / hq, "%s: too many work items", who);
  x = Params{};
  attn_fill(x.a, q, k, v, nullptr, seqs, hq, rows, rows, q_stride, k_stride, v_stride, scale, 0.f, 0, nullptr);
  x.a.cu = cu; x.a.groups = groups;
  x.group = (int32_t)(hq / hkv);
  x.hkv = (int32_t)hkv;
  return GMLM_OK;
}

#define GMLM_GQAS_FOR_R(M) M(128) M(96) M(64) M(32)

static int launch_fwd(const Params& x, int causal, int top, int64_t num_groups, hipStream_t st) {
  static PerDeviceOnce once;
  int rc = once([&]() -> int {
#define GMLM_GQAS_ATTR(RR)                                                                                                         \
    GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fwd_kernel<false, RR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fwd_lds(RR))); \
    GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fwd_kernel<true, RR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fwd_lds(RR)));
    GMLM_GQAS_FOR_R(GMLM_GQAS_ATTR)
#undef GMLM_GQAS_ATTR
    return GMLM_OK;
  });
  if (rc != GMLM_OK) return rc;
  const unsigned grid = (unsigned)(num_groups * x.a.h);
#define GMLM_GQAS_LAUNCH(RR)                                                                    \
  if (RR == top) {                                                                              \
    if (causal) fwd_kernel<true, RR><<<grid, 2 * RR, fwd_lds(RR), st>>>(x);                     \
    else fwd_kernel<false, RR><<<grid, 2 * RR, fwd_lds(RR), st>>>(x);                           \
  }
  GMLM_GQAS_FOR_R(GMLM_GQAS_LAUNCH)
#undef GMLM_GQAS_LAUNCH
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

static int launch_bwd(const Params& x, int causal, int top, int64_t num_groups, hipStream_t st) {
  static PerDeviceOnce once;
  int rc = once([&]() -> int {
#define GMLM_GQAS_ATTR(RR)                                                                                                         \
    GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&bwd_kernel<false, RR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bwd_lds(RR))); \
    GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&bwd_kernel<true, RR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bwd_lds(RR)));
    GMLM_GQAS_FOR_R(GMLM_GQAS_ATTR)
#undef GMLM_GQAS_ATTR
    return GMLM_OK;
  });
  if (rc != GMLM_OK) return rc;
  const unsigned grid = (unsigned)(num_groups * x.hkv);
#define GMLM_GQAS_LAUNCH(RR)                                                                    \
  if (RR == top) {                                                                              \
    if (causal) bwd_kernel<true, RR><<<grid, 2 * RR, bwd_lds(RR), st>>>(x);                     \
    else bwd_kernel<false, RR><<<grid, 2 * RR, bwd_lds(RR), st>>>(x);                           \
  }
  GMLM_GQAS_FOR_R(GMLM_GQAS_LAUNCH)
#undef GMLM_GQAS_LAUNCH
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

}  // namespace gqas
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::gqas;

extern "C" int gmlm_attention_gqa_short_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens, int64_t num_seqs,
                                            int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride,
                                            int64_t k_stride, int64_t v_stride, float scale, float dropout_p, int causal,
                                            const int32_t* seq_groups, int64_t num_groups, void* out, float* lse, int dtype,
                                            gmlm_stream_t stream) {
  static const char* who = "attention_gqa_short_fwd";
  Params x;
  int rc = setup(who, x, q, k, v, cu_seqlens, num_seqs, max_len, total_rows, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p,
                 causal, seq_groups, num_groups, dtype);
  if (rc != GMLM_OK) return rc;
  if (num_groups == 0 || num_seqs == 0 || total_rows == 0) return GMLM_OK;
  x.a.o_w = out; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, hq * d, hkv * d, dtype)) != GMLM_OK) return rc;
  GMLM_REQUIRE(lse, "%s: null lse", who);
  return launch_fwd(x, causal, tile_rows(total_rows), num_groups, as_stream(stream));
}

extern "C" int gmlm_attention_gqa_short_bwd(const void* q, const void* k, const void* v, const void* dout, const float* lse,
                                            const int32_t* cu_seqlens, int64_t num_seqs, int64_t max_len, int64_t total_rows,
                                            int64_t hq, int64_t hkv, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                            float scale, float dropout_p, int causal, const int32_t* seq_groups, int64_t num_groups,
                                            void* dq, void* dk, void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride,
                                            int dtype, gmlm_stream_t stream) {
  static const char* who = "attention_gqa_short_bwd";
  Params x;
  int rc = setup(who, x, q, k, v, cu_seqlens, num_seqs, max_len, total_rows, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p,
                 causal, seq_groups, num_groups, dtype);
  if (rc != GMLM_OK) return rc;
  if (num_groups == 0 || num_seqs == 0 || total_rows == 0) return GMLM_OK;
  attn_fill_bwd(x.a, nullptr, nullptr, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, nullptr);
  const int64_t wq = hq * d, wkv = hkv * d;
  if ((rc = attn_stride_check(who, "q", x.a.q, x.a.q_stride, wq, dtype)) != GMLM_OK) return rc;
  if ((rc = attn_stride_check(who, "k", x.a.k, x.a.k_stride, wkv, dtype)) != GMLM_OK) return rc;
  if ((rc = attn_stride_check(who, "v", x.a.v, x.a.v_stride, wkv, dtype)) != GMLM_OK) return rc;
  if ((rc = attn_stride_check(who, "dq", x.a.dq, x.a.dq_stride, wq, dtype)) != GMLM_OK) return rc;
  if ((rc = attn_stride_check(who, "dk", x.a.dk, x.a.dk_stride, wkv, dtype)) != GMLM_OK) return rc;
  if ((rc = attn_stride_check(who, "dv", x.a.dv, x.a.dv_stride, wkv, dtype)) != GMLM_OK) return rc;
  GMLM_REQUIRE(x.a.dout && x.a.lse && aligned16(x.a.dout), "%s: null or misaligned dout/lse", who);
  return launch_bwd(x, causal, tile_rows(total_rows), num_groups, as_stream(stream));
}
