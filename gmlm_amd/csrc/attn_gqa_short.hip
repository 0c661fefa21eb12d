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
//
// Where the pieces live: the forward body (short_fwd_d64, shared with attn_fwd_short_kernel), the staging helpers and the
// phase 1 / phase 2 block loops are in attn_short.hpp; the launcher and the packed-and-grouped argument checks in
// attn_short_host.hpp.  This file keeps the backward's head loop with its prefetch order, the causal-diagonal policy and the
// entry points.
#include "attn_short.hpp"        // device side: mask step, item bookkeeping, staging, forward body, backward block loops
#include "attn_short_host.hpp"   // host side: launcher, tile height, argument checks, bias-sum tail
#include "../../include/gmlm_hip_gqa_short.h"

namespace gmlm {
namespace gqas {

constexpr int D = 64;

struct Params {
  AttnParams a;       // a.h = query heads, a.lq = total rows (lse is [hq, total_rows]), a.cu / a.groups set
  int32_t group;      // query heads per KV head (hq / hkv)
  int32_t hkv;
};

// ------------------------------------------------------------------------------------------------
// forward: the d = 64 body of attn_short.hpp with K / V of the query head's KV head
// ------------------------------------------------------------------------------------------------
template <bool CAUSAL, int R>
__global__ __launch_bounds__(2 * R, 4) void fwd_kernel(Params x) {
  const int64_t hd = blockIdx.x % x.a.h;
  short_fwd_d64<false, CAUSAL, R>(x.a, blockIdx.x / x.a.h, hd, hd / x.group);
}

// ------------------------------------------------------------------------------------------------
// backward: one work item per (group, KV head), looping over the query heads of the KV head
// ------------------------------------------------------------------------------------------------
constexpr ShortLds kBwdLds{4, kShortPitch, 2, 0};            // tiles K, V, Q, dO | lse, delta [R] | meta

// the policy of the block loops: no dropout, no bias sums; CAUSAL zeroes the probabilities above the diagonal of the wave's own
// block w (key tile row <= query tile row), the lane's own row being 32 w + r
template <bool CAUSAL>
struct BwdPolicy {
  static constexpr bool bias = false;
  int w, r, h;
  __device__ __forceinline__ void pair_q(int kb, int i, float& p0, float& p1, float&, float&) const {
    if (CAUSAL && kb == w) {                                  // wave-uniform
      p0 = acc_row(i, h) <= r ? p0 : 0.f;
      p1 = acc_row(i + 1, h) <= r ? p1 : 0.f;
    }
  }
  __device__ __forceinline__ void pair_k(int qb, int i, float& p0, float& p1, float&, float&) const {
    if (CAUSAL && qb == w) {
      p0 = r <= acc_row(i, h) ? p0 : 0.f;
      p1 = r <= acc_row(i + 1, h) ? p1 : 0.f;
    }
  }
};

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
  constexpr int PITCH = kShortPitch, DB = D / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tk = reinterpret_cast<T*>(smem_raw);
  T* tv = tk + R * PITCH;
  T* tq = tv + R * PITCH;
  T* tdo = tq + R * PITCH;
  float* lse_s = reinterpret_cast<float*>(smem_raw + kBwdLds.floats_at(R));
  float* dl_s = lse_s + R;
  const ShortMeta mt = ShortMeta::carve(smem_raw + kBwdLds.meta_at(R), R);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t item = blockIdx.x / x.hkv, kvh = blockIdx.x % x.hkv;
  const int64_t hd0 = kvh * x.group;                         // first query head of this KV head
  int64_t qbase, kbase, row0;
  int nq, nk;
  short_item_setup<R>(p, item, tid, mt, qbase, kbase, nq, nk, row0, 0);      // lse base of head 0 = first row of the item
  const int n = nq;                                          // packed self-attention: nq == nk
  const T* qg = static_cast<const T*>(p.q) + qbase * p.q_stride + hd0 * D;
  const T* dog = static_cast<const T*>(p.dout) + (qbase * p.h + hd0) * D;
  const int do_stride = (int)(p.h * D);
  {                                                          // K, V: staged once
    uint4 rkv[2][4];
    short_rows_load<R, 2>(rkv, {static_cast<const T*>(p.k) + kbase * p.k_stride + kvh * D, static_cast<const T*>(p.v) + kbase * p.v_stride + kvh * D},
                          {(int)p.k_stride, (int)p.v_stride}, {n}, tid);
    short_rows_store<R, 2>({tk, tv}, rkv, tid);
  }
  // Q, dO and lse of query head hd0 + g: global -> registers, registers -> LDS (the loads of head g + 1 are issued before
  // phase 2 of head g and land in LDS behind its closing barrier)
  uint4 rqo[2][4];
  float rl = INFINITY;
  auto head_load = [&](int g) {
    short_rows_load<R, 2>(rqo, {qg + g * D, dog + g * D}, {(int)p.q_stride, do_stride}, {n}, tid);
    // +inf: a row past the item gets probability 0
    if (tid < R) rl = tid < n ? p.lse[(hd0 + g) * p.lq + row0 + tid] * kLog2e : INFINITY;
  };
  auto head_store = [&]() {
    short_rows_store<R, 2>({tq, tdo}, rqo, tid);
    if (tid < R) lse_s[tid] = rl;
  };
  const float sl2 = p.scale * kLog2e;
  const bool active = w * 32 < n;                            // wave-uniform: a wave whose rows lie past the item stages and skips the math
  const int row = w * 32 + r;                                // the lane's query row (phase 1) and key row (phase 2)
  const BwdPolicy<CAUSAL> pol{w, r, h};
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
      const bf16x8 qm = antihot_frag(mt.qid[row], h);
      int b0, b1;
      block_range(mt.q2k_lo, mt.q2k_hi, w, n, b0, b1);
      if (CAUSAL) b1 = b1 < w + 1 ? b1 : w + 1;               // key blocks above the wave's own hold later positions only
      f32x16 dq[DB];
      short_bwd_phase1<D, R>(tk, tv, tq, tdo, lse_s, dl_s, mt, qm, b0, b1, sl2, pol, row, lane, dq);
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
      if (b1 > b0) short_bwd_phase2<D, R>(tk, tv, tq, tdo, lse_s, dl_s, mt, antihot_frag(mt.kid[row], h), b0, b1, sl2, pol, row, lane, dk, dv);
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
  int rc;
  if ((rc = short_check_packed(who, cu, groups, num_groups, max_len, rows)) != GMLM_OK) return rc;
  if ((rc = short_check_items(who, num_groups, hq)) != GMLM_OK) return rc;
  x = Params{};
  attn_fill(x.a, q, k, v, nullptr, seqs, hq, rows, rows, q_stride, k_stride, v_stride, scale, 0.f, 0, nullptr);
  x.a.cu = cu; x.a.groups = groups;
  x.group = (int32_t)(hq / hkv);
  x.hkv = (int32_t)hkv;
  return GMLM_OK;
}

#define GMLM_GQAS_FWD(F, RR) fwd_kernel<F, RR>
#define GMLM_GQAS_BWD(F, RR) bwd_kernel<F, RR>

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
  static ShortKernels<Params> t{GMLM_SHORT_KERNELS(GMLM_GQAS_FWD), kShortFwdLds};
  return short_launch(t, short_tile_rows(total_rows), causal != 0, (unsigned)(num_groups * hq), as_stream(stream), x);
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
  if ((rc = attn_check_short_bwd_operands(who, x.a, hq * d, hkv * d, dtype)) != GMLM_OK) return rc;
  static ShortKernels<Params> t{GMLM_SHORT_KERNELS(GMLM_GQAS_BWD), kBwdLds};
  return short_launch(t, short_tile_rows(total_rows), causal != 0, (unsigned)(num_groups * hkv), as_stream(stream), x);
}
