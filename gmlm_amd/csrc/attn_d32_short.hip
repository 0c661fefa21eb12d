// LDS-resident short-sequence attention at head dim 32 (bf16, packed layout with seq_groups), forward and one-launch backward,
// gfx950 MFMA: gmlm_attention_d32_short_* (C ABI in include/gmlm_hip_d32_short.h), all in namespace gmlm::d32s.  The d = 32 form
// of attn_short.hip for the 384-wide sentence encoders (12 heads x 32: MiniLM-L6/L12, bge-small, e5-small, gte-small) on
// batches of sequences of <= 128 tokens.
//
// One workgroup = one (GROUP, PAIR OF ADJACENT HEADS) item.  A group is a run of consecutive sequences of the packed batch
// (<= 13 sequences, <= R rows: ops.pack_sequence_groups), so a workgroup stages full tiles from ONE contiguous row range.  Two
// adjacent d = 32 heads are one contiguous 128-byte row piece of the fused QKV buffer: staging issues exactly the global-load
// pattern of the d = 64 kernel (8 lanes x 16 B per row piece) and the LDS images keep the d = 64 layouts (the XOR swizzle of
// attn_common.hpp in the forward, 8 elements of padding per row in the backward).  The waves then run the two heads one after
// the other over the staged tiles: QK^T of head i contracts 16-byte chunks 4i..4i+3 of the row (two 32x32x16 steps), P V of head
// i is d-block i of the d = 64 image.  Half as many work items as one per (group, head), and K, V, Q, dO of both heads are in
// flight in one staging phase.  The number of heads must be even (the entry points refuse an odd one).
//
// Attention stays inside a sequence through the block-diagonal mask step of attn_short.hpp (one extra contraction step at the
// head of every score chain, no VALU work) and a wave-uniform range of 32-row blocks; blocks that cannot hold a row of the wave's
// sequences are skipped.
// Forward: all keys of a row are resident, so the softmax is two plain passes over the score blocks held in registers.
// Backward: ONE launch.  Phase 1 (query on the lane), per head: P and dP of all key blocks in registers, delta = sum_k P dP in
// fp32 from them, dS = P (dP - delta), dQ.  Phase 2 (key on the lane), per head: delta from LDS, dK and dV.  Neither out nor
// out_lo is read and there is no delta workspace.  Optionally the column sums of dQ | dK | dV (the bias gradient of the fused
// QKV projection) come out as matrix-vector products on the MFMA pipe, as in attn_short.hip.  Fixed summation orders, no
// atomics: identical calls give identical bits.
//
// Dropout: the mask every other head dim draws (attn_common.hpp), per (SEQUENCE, head): slab = head * total_rows + first row of
// the sequence, query and key counted from the sequence's first row - the packed streaming kernels of attn_d32.hip draw the same
// words, so the route does not change the mask.  A sequence may start at an odd tile row; then the two elements of an adjacent
// register pair lie in different 2 x 2 hash tiles, so this file evaluates two words per register pair (equal when the start is
// even) instead of the one of the group-relative mask of attn_short.hip.
//
// Where the pieces live: the forward staging (short_stage_fwd), the backward staging helpers and the phase 1 / phase 2 block
// loops of one head (shared with attn_short.hip and attn_gqa_short.hip) are in attn_short.hpp; the launcher, the
// packed-and-grouped argument checks and the bias-sum tail in attn_short_host.hpp.  This file keeps the head-pair frames, the
// one-head views of the swizzled images, the per-sequence dropout policy and its own bias-sum stage (pm as hi + lo).
#include "attn_short.hpp"        // device side: mask step, item bookkeeping, staging, forward body, backward block loops
#include "attn_short_host.hpp"   // host side: launcher, tile height, argument checks, bias-sum tail
#include "../../include/gmlm_hip_d32_short.h"

namespace gmlm {
namespace d32s {

constexpr int D = 32;        // head dim
constexpr int W = 2 * D;     // elements of a staged row: two adjacent heads

// ---- per-sequence dropout multipliers of a register pair --------------------------------------------------------------------
// The lane's own row sits at `own` (relative to its sequence), the pair's rows on the other axis at rel, rel + 1 (rel may be odd
// or negative: rows of another sequence, whose probability is exactly 0 whatever the multiplier).  u = base + (own >> 1) * C_own.
// QUERY_OWN: the lane holds a query (fields 16 (q & 1) + 8 (k & 1), other axis = keys, C2), else a key (other axis = queries, C1).
template <bool QUERY_OWN>
__device__ __forceinline__ void drop_pair_rel(uint32_t u, int own_odd, int rel, uint32_t th8, float ks, float& m0, float& m1) {
  constexpr uint32_t C = QUERY_OWN ? kDropC2 : kDropC1;
  constexpr int own_bits = QUERY_OWN ? 16 : 8, oth_bits = QUERY_OWN ? 8 : 16;
  const int par = rel & 1, a = rel >> 1;                      // arithmetic shift: floor
  const uint32_t w0 = lowbias32(u + (uint32_t)a * C), w1 = lowbias32(u + (uint32_t)(a + par) * C);
  m0 = drop_keep8(w0 >> (own_bits * own_odd + oth_bits * par), th8, ks);
  m1 = drop_keep8(w1 >> (own_bits * own_odd + oth_bits * (1 - par)), th8, ks);
}

// ---- the d = 64 swizzled images (attn_common.hpp), one head (32 columns = d-block hh) at a time -------------------------------
__device__ __forceinline__ void mma_rows_sw_head(const bf16_t* ts, int row0, const bf16x8& f0, const bf16x8& f1, f32x16& acc, int r,
                                                 int h, int hh) {
  const bf16_t* rowp = ts + (row0 + r) * W;
  const int x = sw_row(row0 + r);
  const bf16x8 a0 = *reinterpret_cast<const bf16x8*>(rowp + (((4 * hh + h) ^ x) << 3));
  const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(rowp + (((4 * hh + 2 + h) ^ x) << 3));
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, f0, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, f1, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma_acc_sw_head(const bf16_t* ts, int row0, const f32x16& x, f32x16& out, int lane, int hh) {
  const int g = lane >> 4, i = lane & 15, qq = i >> 2, pp = i & 3, hf = g >> 1;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bf16x8 b;
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = (__bf16)x[8 * s + j];
    const int row = row0 + 16 * s + 4 * hf + qq;                        // the +8 row of the hi half has the same swizzle phase
    const bf16_t* rowp = ts + row * W + 4 * (pp & 1);
    const int slot = (4 * hh + 2 * (g & 1) + (pp >> 1)) ^ sw_tr(row);
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(GMLM_LDS3(bf16x4, rowp + (slot << 3)));
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(GMLM_LDS3(bf16x4, rowp + (slot << 3) + 8 * W));
    bf16x8 a;
#pragma unroll
    for (int j = 0; j < 4; ++j) { a[j] = lo[j]; a[4 + j] = hi[j]; }
    out = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, out, 0, 0, 0);
  }
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <bool DROP, int R>
__global__ __launch_bounds__(2 * R, 4) void fwd_kernel(AttnParams p) {
  using T = bf16_t;
  constexpr int NB = R / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tk = reinterpret_cast<T*>(smem_raw);
  T* tv = tk + R * W;
  const ShortMeta mt = ShortMeta::carve(smem_raw + kShortFwdLds.meta_at(R), R);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t pairs = p.h >> 1, item = blockIdx.x / pairs, hp = blockIdx.x % pairs;
  int64_t qbase, kbase, row0;
  int nq, nk;
  short_item_setup<R>(p, item, tid, mt, qbase, kbase, nq, nk, row0, 0);      // lse base of head 0 = first row of the item
  // K and V of both heads are staged (MFMA A operands of every wave); the query row goes straight into the B-operand registers,
  // both heads at once
  const int q_row = w * 32 + r;
  RowFrag<T, W> qf;
  short_stage_fwd<R>(p, static_cast<const T*>(p.q) + qbase * p.q_stride + hp * W, static_cast<const T*>(p.k) + kbase * p.k_stride + hp * W,
                     static_cast<const T*>(p.v) + kbase * p.v_stride + hp * W, nq, nk, tk, tv, qf, tid, q_row, h);
  if (w * 32 >= nq) return;                                   // (no barrier below)
  const bf16x8 qm = antihot_frag(mt.qid[q_row], h);
  int b0, b1;
  block_range(mt.q2k_lo, mt.q2k_hi, w, nq, b0, b1);           // key blocks that hold a key of this wave's sequences
  const float sl2 = p.scale * kLog2e;
  const int lo = mt.q2k_lo[q_row];                            // first tile row of the lane's sequence
  const int q_rel = q_row - lo, q_odd = q_rel & 1, k_off = 4 * h - lo;
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const int64_t hd = 2 * hp + hh;
    f32x16 s[NB];
    float rmax = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      if (kb < b0 || kb >= b1) continue;
      f32x16 z;
#pragma unroll
      for (int i = 0; i < 16; ++i) z[i] = 0.f;
      s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(onehot_frag(mt.kid[kb * 32 + r], h), qm, z, 0, 0, 0);   // block-diagonal / padding mask
      mma_rows_sw_head(tk, kb * 32, qf.v[2 * hh], qf.v[2 * hh + 1], s[kb], r, h, hh);
      rmax = fmaxf(rmax, max16(s[kb]));
    }
    const float m = b1 > b0 ? xhalf_max(rmax) * sl2 : 0.f;    // finite for a real query row (its own sequence has >= 1 key)
    const uint32_t dq_u = drop_base(attn_seed(p), hd * p.lq + row0 + lo) + (uint32_t)(q_rel >> 1) * kDropC1;
    f32x16 o;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = 0.f;
    float l = 0.f;
#pragma unroll
    for (int kb = 0; kb < NB; ++kb) {
      if (kb < b0 || kb >= b1) continue;
#pragma unroll
      for (int i = 0; i < 16; i += 2) {
        const float e0 = fast_exp2(fmaf(s[kb][i], sl2, -m)), e1 = fast_exp2(fmaf(s[kb][i + 1], sl2, -m));   // masked: exp2(-2e29) = 0
        l += e0 + e1;                                         // the normaliser uses the un-dropped probabilities
        float m0 = 1.f, m1 = 1.f;
        if (DROP) drop_pair_rel<true>(dq_u, q_odd, kb * 32 + acc_row(i, 0) + k_off, p.drop_thresh, p.keep_scale, m0, m1);
        s[kb][i] = e0 * m0;
        s[kb][i + 1] = e1 * m1;
      }
      mma_acc_sw_head(tv, kb * 32, s[kb], o, lane, hh);
    }
    l = xhalf_sum(l);
    if (q_row < nq) {
      const float inv = l > 0.f ? 1.f / l : 0.f;
      T* og = static_cast<T*>(p.o_w) + ((qbase + q_row) * p.h + hd) * D;
      store_t<T>(og, o, inv, h);
      if (h == 0) p.lse_w[hd * p.lq + row0 + q_row] = l > 0.f ? (m + __log2f(l)) * kLn2 : -INFINITY;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
// tiles K, V, Q, dO | lse, delta [2][R] each: per head of the pair | bias-gradient coefficients (p.dbias_part), bf16 hi + lo
// pairs, per head: per key c_k = sum_q dS[q,k], per query pm_q = sum_k P'[q,k] (1 without dropout; with it any value around 1, and
// one bf16 rounding of it is 2^-9 of the dV sums): [2][4][R] | meta
constexpr ShortLds kBwdLds{4, kShortPitch, 4, 8};

// the per-sequence dropout mask as the policy of the block loops.  u: base + (own >> 1) * C_own for the lane's own row counted from
// its sequence's first row, odd: that row's parity, off: 4 h - first tile row of the sequence (tile row on the other axis -> row
// of the sequence)
template <bool DROP>
struct BwdPolicy {
  bool bias;
  uint32_t u, th;
  int odd, off;
  float ks;
  __device__ __forceinline__ void pair_q(int kb, int i, float&, float&, float& m0, float& m1) const {
    if (DROP) drop_pair_rel<true>(u, odd, kb * 32 + acc_row(i, 0) + off, th, ks, m0, m1);
  }
  __device__ __forceinline__ void pair_k(int qb, int i, float&, float&, float& m0, float& m1) const {
    if (DROP) drop_pair_rel<false>(u, odd, qb * 32 + acc_row(i, 0) + off, th, ks, m0, m1);
  }
};

template <bool DROP, int R>
__global__ __launch_bounds__(2 * R, R >= 96 ? 2 : 3) void bwd_kernel(AttnParams p) {
  using T = bf16_t;
  constexpr int NT = 2 * R, PITCH = kShortPitch;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tk = reinterpret_cast<T*>(smem_raw);
  T* tv = tk + R * PITCH;
  T* tq = tv + R * PITCH;
  T* tdo = tq + R * PITCH;
  float* lse_s = reinterpret_cast<float*>(smem_raw + kBwdLds.floats_at(R));   // [2][R]
  float* dl_s = lse_s + 2 * R;                                                // [2][R]
  T* coef = reinterpret_cast<T*>(smem_raw + kBwdLds.coef_at(R));
  const ShortMeta mt = ShortMeta::carve(smem_raw + kBwdLds.meta_at(R), R);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t pairs = p.h >> 1, item = blockIdx.x / pairs, hp = blockIdx.x % pairs;
  const bool bgrad = p.dbias_part != nullptr;                // block-uniform
  if (bgrad)
    for (int i = tid; i < 8 * R; i += NT) coef[i] = f32_to_bf16(0.f);     // waves that skip a phase leave zeros
  int64_t qbase, kbase, row0;
  int nq, nk;
  short_item_setup<R>(p, item, tid, mt, qbase, kbase, nq, nk, row0, 0);
  const int do_stride = (int)(p.h * D);
  uint4 rg[4][4];
  short_rows_load<R, 4>(rg, {static_cast<const T*>(p.k) + kbase * p.k_stride + hp * W, static_cast<const T*>(p.v) + kbase * p.v_stride + hp * W,
                             static_cast<const T*>(p.q) + qbase * p.q_stride + hp * W, static_cast<const T*>(p.dout) + qbase * do_stride + hp * W},
                        {(int)p.k_stride, (int)p.v_stride, (int)p.q_stride, do_stride}, {nk, nq}, tid);
  {                                                          // +inf: a row past the item gets probability 0
    const int hh = tid / R, row = tid % R;                    // NT = 2 R threads: one (head, row) each
    lse_s[tid] = row < nq ? p.lse[(2 * hp + hh) * p.lq + row0 + row] * kLog2e : INFINITY;
  }
  short_rows_store<R, 4>({tk, tv, tq, tdo}, rg, tid);
  __syncthreads();
  const float sl2 = p.scale * kLog2e;
  const uint32_t seed_mix = drop_base(attn_seed(p), 0);
  // ---- phase 1: delta and dQ (query on the lane; K, V as MFMA A operands), head after head -----------------
  if (w * 32 < nq) {
    const int q_row = w * 32 + r;
    const bf16x8 qm = antihot_frag(mt.qid[q_row], h);
    int b0, b1;
    block_range(mt.q2k_lo, mt.q2k_hi, w, nq, b0, b1);
    const int lo = mt.q2k_lo[q_row];
    const int q_rel = q_row - lo;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int64_t hd = 2 * hp + hh;
      const BwdPolicy<DROP> pol{bgrad, seed_mix + (uint32_t)(hd * p.lq + row0 + lo) * kDropC3 + (uint32_t)(q_rel >> 1) * kDropC1, p.drop_thresh,
                                q_rel & 1, 4 * h - lo, p.keep_scale};
      f32x16 dq[1];
      float pm = short_bwd_phase1<D, R>(tk + hh * D, tv + hh * D, tq + hh * D, tdo + hh * D, lse_s + hh * R, dl_s + hh * R, mt, qm, b0, b1, sl2,
                                        pol, q_row, lane, dq);
      if (q_row < nq) {
        T* dqg = static_cast<T*>(p.dq) + (qbase + q_row) * p.dq_stride + hd * D;
        store_t<T>(dqg, dq[0], p.scale, h);
      }
      if (bgrad) {
        pm = xhalf_sum(pm);
        if (h == 0) {
          const bf16_t hi = f32_to_bf16(pm);
          coef[(4 * hh + 2) * R + q_row] = hi;
          coef[(4 * hh + 3) * R + q_row] = f32_to_bf16(pm - bf16_to_f32(hi));
        }
      }
    }
  }
  // rows past the item (their waves skipped phase 1): delta 0, never read with a non-zero probability
  if (w * 32 >= nq && lane < 32) { dl_s[w * 32 + lane] = 0.f; dl_s[R + w * 32 + lane] = 0.f; }
  __syncthreads();                                          // delta of every query row and head is in LDS
  // ---- phase 2: dK, dV (key on the lane; Q, dO as MFMA A operands), head after head -----------------------
  if (w * 32 < nk) {
    const int key = w * 32 + r;
    int b0, b1;
    block_range(mt.k2q_lo, mt.k2q_hi, w, nk, b0, b1);       // empty when the wave holds padding keys only
    const bf16x8 km = antihot_frag(mt.kid[key], h);
    const int lo = mt.k2q_lo[key];
    const int k_rel = key - lo;
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int64_t hd = 2 * hp + hh;
      f32x16 dk[1], dv[1];
#pragma unroll
      for (int i = 0; i < 16; ++i) { dk[0][i] = 0.f; dv[0][i] = 0.f; }
      if (b1 > b0) {
        const BwdPolicy<DROP> pol{bgrad, seed_mix + (uint32_t)(hd * p.lq + row0 + lo) * kDropC3 + (uint32_t)(k_rel >> 1) * kDropC2, p.drop_thresh,
                                  k_rel & 1, 4 * h - lo, p.keep_scale};
        float ck = short_bwd_phase2<D, R>(tk + hh * D, tv + hh * D, tq + hh * D, tdo + hh * D, lse_s + hh * R, dl_s + hh * R, mt, km, b0, b1, sl2,
                                          pol, key, lane, dk, dv);
        if (bgrad) {
          ck = xhalf_sum(ck);
          if (h == 0) {
            const bf16_t hi = f32_to_bf16(ck);
            coef[4 * hh * R + key] = hi;
            coef[(4 * hh + 1) * R + key] = f32_to_bf16(ck - bf16_to_f32(hi));
          }
        }
      }
      if (key < nk) {
        T* dkg = static_cast<T*>(p.dk) + (kbase + key) * p.dk_stride + hd * D;
        T* dvg = static_cast<T*>(p.dv) + (kbase + key) * p.dv_stride + hd * D;
        store_t<T>(dkg, dk[0], p.scale, h);
        store_t<T>(dvg, dv[0], 1.f, h);
      }
    }
  }
  // ---- bias gradients: column sums of this workgroup's dQ, dK, dV rows as matrix-vector products (attn_short.hip) ----------
  //   sum_q dQ[q,:] = scale * sum_k c_k K[k,:]      sum_k dV[k,:] = sum_q pm_q dO[q,:]      sum_k dK[k,:] = 0 (rows of dS sum to zero)
  if (bgrad) {
    __syncthreads();                                       // coefficients of every wave are in LDS
    float* outp = p.dbias_part + item * 3 * p.h * D + hp * W;
    for (int u = w; u < 4; u += R / 32) {                  // wave-uniform: one (tensor, head) unit per wave and turn
      const int t = u >> 1, hh = u & 1;                    // t = 0: dQ sums from (K tile, c), t = 1: dV sums from (dO tile, pm)
      const T* tile = (t == 0 ? tk : tdo) + hh * D;
      const T* cf = coef + (4 * hh + 2 * t) * R;          // this unit's hi | lo pair
      const int rows = t == 0 ? nk : nq;
      f32x16 acc[1];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[0][i] = 0.f;
#pragma unroll
      for (int rb = 0; rb < R / 32; ++rb) {
        if (rb * 32 >= rows) break;
        mma_acc_coef<D>(tile, PITCH, rb * 32, cf + R, acc, lane);            // lo first: the small terms accumulate before the large
        mma_acc_coef<D>(tile, PITCH, rb * 32, cf, acc, lane);
      }
      if (r == 0) {                                        // every column holds the same vector: column 0 of each half writes its rows
        const float mul = t == 0 ? p.scale : 1.f;
        float* o2 = outp + (t == 0 ? 0 : 2) * p.h * D + hh * D;
#pragma unroll
        for (int i = 0; i < 16; ++i) o2[acc_row(i, h)] = acc[0][i] * mul;
      }
    }
    if (tid < W) outp[p.h * D + tid] = 0.f;                // dK column sums
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// Validation up to the nothing-to-do return, in the order of include/gmlm_hip_d32_short.h; fills the launch parameters
static int setup(const char* who, AttnParams& p, const void* q, const void* k, const void* v, const int32_t* cu, int64_t seqs,
                 int64_t max_len, int64_t rows, int64_t h, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                 float dropout_p, uint64_t seed, const uint64_t* seed_dev, const int32_t* groups, int64_t num_groups, int dtype) {
  GMLM_REQUIRE(seqs >= 0 && h > 0, "%s: bad sizes", who);
  GMLM_REQUIRE(d == 32, "%s: head dim d = %ld not supported (this entry point takes 32)", who, (long)d);
  GMLM_REQUIRE(dtype == GMLM_BF16, "%s: unsupported dtype (the short-sequence head-dim-32 kernels take bf16)", who);
  GMLM_REQUIRE(h % 2 == 0, "%s: h = %ld heads: a work item is a pair of adjacent heads, h must be even", who, (long)h);
  GMLM_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout_p must be in [0,1)", who);
  GMLM_REQUIRE(scale > 0.f, "%s: scale must be positive", who);
  int rc;
  if ((rc = short_check_packed(who, cu, groups, num_groups, max_len, rows)) != GMLM_OK) return rc;
  GMLM_REQUIRE(num_groups > 0 || rows == 0 || seqs == 0, "%s: num_groups must be > 0 with rows present", who);
  // what the host can see of the group bounds without reading device memory (the kernels clamp the rest)
  GMLM_REQUIRE(num_groups == 0 || seqs <= num_groups * kShortMaxSeq, "%s: seq_groups: %ld sequences in %ld groups, a group takes at most %d",
               who, (long)seqs, (long)num_groups, kShortMaxSeq);
  GMLM_REQUIRE(num_groups == 0 || rows <= num_groups * 128, "%s: seq_groups: %ld rows in %ld groups, a group takes at most 128", who,
               (long)rows, (long)num_groups);
  if ((rc = short_check_items(who, num_groups, h)) != GMLM_OK) return rc;
  p = AttnParams{};
  attn_fill(p, q, k, v, nullptr, seqs, h, rows, rows, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev);
  p.cu = cu; p.groups = groups;
  return GMLM_OK;
}

#define GMLM_D32S_FWD(F, RR) fwd_kernel<F, RR>
#define GMLM_D32S_BWD(F, RR) bwd_kernel<F, RR>

}  // namespace d32s
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::d32s;

extern "C" int gmlm_attention_d32_short_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens, int64_t num_seqs,
                                            int64_t max_len, int64_t total_rows, int64_t h, int64_t d, int64_t q_stride,
                                            int64_t k_stride, int64_t v_stride, float scale, float dropout_p, uint64_t seed,
                                            const uint64_t* seed_dev, const int32_t* seq_groups, int64_t num_groups, void* out,
                                            float* lse, int dtype, gmlm_stream_t stream) {
  static const char* who = "attention_d32_short_fwd";
  AttnParams p;
  int rc = setup(who, p, q, k, v, cu_seqlens, num_seqs, max_len, total_rows, h, d, q_stride, k_stride, v_stride, scale, dropout_p, seed,
                 seed_dev, seq_groups, num_groups, dtype);
  if (rc != GMLM_OK) return rc;
  if (num_groups == 0 || num_seqs == 0 || total_rows == 0) return GMLM_OK;
  p.o_w = out; p.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, p, h * d, h * d, dtype)) != GMLM_OK) return rc;
  GMLM_REQUIRE(lse, "%s: null lse", who);
  static ShortKernels<AttnParams> t{GMLM_SHORT_KERNELS(GMLM_D32S_FWD), kShortFwdLds};
  return short_launch(t, short_tile_rows(total_rows), p.drop_thresh != 0, (unsigned)(num_groups * (h / 2)), as_stream(stream), p);
}

extern "C" int gmlm_attention_d32_short_bwd(const void* q, const void* k, const void* v, const void* dout, const float* lse,
                                            const int32_t* cu_seqlens, int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t h,
                                            int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                            float dropout_p, uint64_t seed, const uint64_t* seed_dev, const int32_t* seq_groups,
                                            int64_t num_groups, void* dq, void* dk, void* dv, int64_t dq_stride, int64_t dk_stride,
                                            int64_t dv_stride, float* dbias_partial, float* dbias, int dtype, gmlm_stream_t stream) {
  static const char* who = "attention_d32_short_bwd";
  AttnParams p;
  int rc = setup(who, p, q, k, v, cu_seqlens, num_seqs, max_len, total_rows, h, d, q_stride, k_stride, v_stride, scale, dropout_p, seed,
                 seed_dev, seq_groups, num_groups, dtype);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE((dbias == nullptr) == (dbias_partial == nullptr), "%s: dbias and dbias_partial go together (both or neither)", who);
  if (num_groups == 0 || num_seqs == 0 || total_rows == 0) return GMLM_OK;
  attn_fill_bwd(p, nullptr, nullptr, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, nullptr);
  p.dbias_part = dbias_partial;
  if ((rc = attn_check_short_bwd_operands(who, p, h * d, h * d, dtype)) != GMLM_OK) return rc;
  static ShortKernels<AttnParams> t{GMLM_SHORT_KERNELS(GMLM_D32S_BWD), kBwdLds};
  rc = short_launch(t, short_tile_rows(total_rows), p.drop_thresh != 0, (unsigned)(num_groups * (h / 2)), as_stream(stream), p);
  if (rc != GMLM_OK || !dbias) return rc;
  return short_bias_sums(p.dbias_part, num_groups, 3 * h * d, dbias, as_stream(stream));   // [groups, 3 h d] -> [3 h d]
}
