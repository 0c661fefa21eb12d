// K5 for sequences of <= 128 tokens (bf16, d = 64): the text encoder's attention, forward and backward, gfx950.
// Reference: BertSelfAttention's softmax(QK^T d^-1/2 + padding mask)V (hf:modeling_bert.py:188-201) on what the reference's
// tokeniser produces (max_length = 128, main.py:340), and its autograd backward.
//
// One workgroup = one (GROUP, head) item.  A group is a run of consecutive sequences of the packed batch whose rows add up
// to <= R (= 128) - at most 13 of them - so a workgroup always stages full tiles: its Q / K / V (/ dO) rows are ONE contiguous
// row range of the packed tensors, fetched with the coalesced pattern (8 lanes x 16 B per 128-byte row piece), all loads in
// flight at once.  (One workgroup per sequence left a third of every 128-row tile empty at the 16..128-token mix and kept too
// few bytes in flight per CU: 3.0-3.9 TB/s.)  Attention stays inside a sequence through a block-diagonal mask that costs no
// VALU work: every score chain starts with ONE extra contraction step
//        onehot(sequence id of the tile row) x [ -2^100 where column != sequence id of the lane's row ]
// so a score between rows of different sequences (or against a padding row: id 15, which nobody matches) leaves the MFMA chain
// at about -1.3e30 and its probability is exactly 0.  32-row blocks that cannot hold a row of the wave's sequences are skipped
// (wave-uniform block range).  Padded batches (kv_len) run as one sequence per group through the same code.
//
// Forward: all keys of a row are resident, so the softmax is two plain passes over the score blocks held in registers.
// Backward: ONE launch.  Phase 1 (query on the lane) computes P and dP = dO V^T of all its key blocks, keeps them in
// registers, forms  delta = sum_k P dP  from them IN FP32 and only then dS = P (dP - delta) and dQ.  That delta is exact for
// the P the kernel uses: the rows of dS sum to zero to fp32 precision.  The usual flash-attention form delta = rowsum(dO * O)
// reads the bf16-ROUNDED forward output: its error (2^-9 |dO||O|) does not cancel and was the whole reason why the query / key
// projection gradients of the deep encoder layers had a cosine of 0.4 against fp32 (measured: oracle/bf16_emulation.py,
// DESIGN.md section 4); it also needed a fifth tensor read (O).  Phase 2 (key on the lane) takes delta from LDS and forms
// dK, dV.  Optionally the column sums of dQ | dK | dV (the fused QKV projection's bias gradient) come out as three
// matrix-vector products on the MFMA pipe; their per-key coefficients c_k = sum_q dS[q,k] sum to zero over a sequence, so
// they are carried as a bf16 hi + lo pair (2^-17) instead of one rounded bf16 value.
//
// Where the pieces live: the forward body (short_fwd_d64, shared with gqas::fwd_kernel), the staging and the phase 1 / phase 2
// block loops (shared with attn_gqa_short.hip and attn_d32_short.hip) are in attn_short.hpp; the launcher, the LDS sizes'
// host use and the bias-sum tail in attn_short_host.hpp.  This file keeps the two kernels' frames, the group-relative dropout
// policy and the bias-sum stage.
#include "attn_short.hpp"        // device side: mask step, item bookkeeping, staging, forward body, backward block loops
#include "attn_short_host.hpp"   // host side: launcher, tile height, argument checks, bias-sum tail

namespace gmlm {

#ifndef GMLM_SHORT_FWD_OCC
#define GMLM_SHORT_FWD_OCC 4
#endif

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
template <int D, bool DROP, int R>
__global__ __launch_bounds__(2 * R, GMLM_SHORT_FWD_OCC) void attn_fwd_short_kernel(AttnParams p) {
  static_assert(D == 64, "dense swizzled images are laid out for d = 64");
  const int64_t hd = blockIdx.x % p.h;
  short_fwd_d64<DROP, false, R>(p, blockIdx.x / p.h, hd, hd);
}

// ------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------
// tiles K, V, Q, dO | lse, delta [R] | bias-gradient coefficients (p.dbias_part), bf16: per key c_k = sum_q dS[q,k] as hi + lo,
// per query pm_q = sum_k P'[q,k]: [3][R] | meta
constexpr ShortLds kShortBwdLds{4, kShortPitch, 2, 3};

// the group-relative dropout mask (attn_common.hpp: one hash per register pair) as the policy of the block loops.  u: the
// lane's own share of the hash argument, odd: the parity of its own tile row
template <bool DROP>
struct K5BwdPolicy {
  bool bias;
  uint32_t u, th;
  int odd;
  float ks;
  __device__ __forceinline__ void pair_q(int kb, int i, float&, float&, float& m0, float& m1) const {
    if (DROP) drop_pair_q(u + (uint32_t)((kb * 32 + acc_row(i, 0)) >> 1) * kDropC2, odd, th, ks, m0, m1);
  }
  __device__ __forceinline__ void pair_k(int qb, int i, float&, float&, float& m0, float& m1) const {
    if (DROP) drop_pair_k(u + (uint32_t)((qb * 32 + acc_row(i, 0)) >> 1) * kDropC1, odd, th, ks, m0, m1);
  }
};

template <int D, bool DROP, int R>
__global__ __launch_bounds__(2 * R, R >= 96 ? 2 : 3) void attn_bwd_short_kernel(AttnParams p) {
  using T = bf16_t;
  static_assert(D == 64, "the staged row piece is 64 elements");
  constexpr int NT = 2 * R, PITCH = kShortPitch, DB = D / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tk = reinterpret_cast<T*>(smem_raw);
  T* tv = tk + R * PITCH;
  T* tq = tv + R * PITCH;
  T* tdo = tq + R * PITCH;
  float* lse_s = reinterpret_cast<float*>(smem_raw + kShortBwdLds.floats_at(R));
  float* dl_s = lse_s + R;
  T* coef = reinterpret_cast<T*>(smem_raw + kShortBwdLds.coef_at(R));
  const ShortMeta mt = ShortMeta::carve(smem_raw + kShortBwdLds.meta_at(R), R);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int64_t item = blockIdx.x / p.h, hd = blockIdx.x % p.h;
  const bool bgrad = p.dbias_part != nullptr;                // block-uniform
  if (bgrad)
    for (int i = tid; i < 3 * R; i += NT) coef[i] = f32_to_bf16(0.f);     // waves that skip a phase leave zeros
  int64_t qbase, kbase, lse_base;
  int nq, nk;
  short_item_setup<R>(p, item, tid, mt, qbase, kbase, nq, nk, lse_base, hd);
  const int do_stride = (int)(p.h * D);
  uint4 rg[4][4];
  short_rows_load<R, 4>(rg, {static_cast<const T*>(p.k) + kbase * p.k_stride + hd * D, static_cast<const T*>(p.v) + kbase * p.v_stride + hd * D,
                             static_cast<const T*>(p.q) + qbase * p.q_stride + hd * D, static_cast<const T*>(p.dout) + (qbase * p.h + hd) * D},
                        {(int)p.k_stride, (int)p.v_stride, (int)p.q_stride, do_stride}, {nk, nq}, tid);
  if (tid < R) lse_s[tid] = tid < nq ? p.lse[lse_base + tid] * kLog2e : INFINITY;   // +inf: a row past the item gets probability 0
  short_rows_store<R, 4>({tk, tv, tq, tdo}, rg, tid);
  __syncthreads();
  const float sl2 = p.scale * kLog2e;
  const uint32_t d_base = drop_base(attn_seed(p), lse_base);
  // ---- phase 1: delta and dQ (query on the lane; K, V as MFMA A operands) -------------------------------
  if (w * 32 < nq) {
    const int q_row = w * 32 + r;
    const bf16x8 qm = antihot_frag(mt.qid[q_row], h);
    int b0, b1;
    block_range(mt.q2k_lo, mt.q2k_hi, w, nq, b0, b1);
    const K5BwdPolicy<DROP> pol{bgrad, d_base + (uint32_t)(q_row >> 1) * kDropC1 + (uint32_t)(2 * h) * kDropC2, p.drop_thresh, q_row & 1,
                                p.keep_scale};
    f32x16 dq[DB];
    float pm = short_bwd_phase1<D, R>(tk, tv, tq, tdo, lse_s, dl_s, mt, qm, b0, b1, sl2, pol, q_row, lane, dq);
    if (q_row < nq) {
      T* dqg = static_cast<T*>(p.dq) + (qbase + q_row) * p.dq_stride + hd * D;
#pragma unroll
      for (int d = 0; d < DB; ++d) store_t<T>(dqg + d * 32, dq[d], p.scale, h);
    }
    if (bgrad) {
      pm = xhalf_sum(pm);
      if (h == 0) coef[2 * R + q_row] = f32_to_bf16(pm);
    }
  }
  // rows past the item (their waves skipped phase 1): delta 0, never read with a non-zero probability
  if (w * 32 >= nq && lane < 32) dl_s[w * 32 + lane] = 0.f;
  __syncthreads();                                          // delta of every query row is in LDS
  // ---- phase 2: dK, dV (key on the lane; Q, dO as MFMA A operands) -------------------------------------
  if (w * 32 < nk) {
    const int key = w * 32 + r;
    int b0, b1;
    block_range(mt.k2q_lo, mt.k2q_hi, w, nk, b0, b1);       // empty when the wave holds padding keys only
    f32x16 dk[DB], dv[DB];
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
      for (int i = 0; i < 16; ++i) { dk[d][i] = 0.f; dv[d][i] = 0.f; }
    if (b1 > b0) {
      const bf16x8 km = antihot_frag(mt.kid[key], h);
      const K5BwdPolicy<DROP> pol{bgrad, d_base + (uint32_t)(key >> 1) * kDropC2 + (uint32_t)(2 * h) * kDropC1, p.drop_thresh, key & 1,
                                  p.keep_scale};
      float ck = short_bwd_phase2<D, R>(tk, tv, tq, tdo, lse_s, dl_s, mt, km, b0, b1, sl2, pol, key, lane, dk, dv);
      if (bgrad) {
        ck = xhalf_sum(ck);
        if (h == 0) {
          const bf16_t hi = f32_to_bf16(ck);
          coef[key] = hi;
          coef[R + key] = f32_to_bf16(ck - bf16_to_f32(hi));
        }
      }
    }
    if (key < nk) {
      T* dkg = static_cast<T*>(p.dk) + (kbase + key) * p.dk_stride + hd * D;
      T* dvg = static_cast<T*>(p.dv) + (kbase + key) * p.dv_stride + hd * D;
#pragma unroll
      for (int d = 0; d < DB; ++d) {
        store_t<T>(dkg + d * 32, dk[d], p.scale, h);
        store_t<T>(dvg + d * 32, dv[d], 1.f, h);
      }
    }
  }
  // ---- bias gradients: column sums of this workgroup's dQ, dK, dV rows, WITHOUT a cross-lane reduction ----------
  //   sum_q dQ[q,:] = scale * sum_k c_k K[k,:],  c_k = sum_q dS[q,k]          sum_k dV[k,:] = sum_q pm_q dO[q,:],  pm_q = sum_k P'[q,k]
  //   sum_k dK[k,:] = scale * sum_q (sum_k dS[q,k]) Q[q,:] = 0: the rows of dS sum to zero (a key bias shifts every score of
  //   a query alike and the softmax does not see it; the reference's autograd returns rounding noise of order 1e-8 there).
  // Matrix-vector products with tiles that are already in LDS: tile^T on the MFMA A side (ds_read_b64_tr_b16), the coefficient
  // vector broadcast on the B side; one (tensor, 32-column block) unit per wave.  The c_k of a sequence sum to zero, so the
  // product is what is left after a cancellation: c goes in as hi + lo (two passes), not as one bf16 value.
  // (attn_d32_short.hip has its own copy of this stage: there pm goes in as hi + lo too and a unit is a (tensor, head).)
  if (bgrad) {
    __syncthreads();                                       // coefficients of every wave are in LDS
    float* outp = p.dbias_part + (item * 3 * p.h + hd) * D;
    for (int u = w; u < 2 * DB; u += R / 32) {             // wave-uniform
      const int t = u / DB, db = u % DB;                   // t = 0: dQ sums from (K tile, c), t = 1: dV sums from (dO tile, pm)
      const T* tile = (t == 0 ? tk : tdo) + db * 32;
      const int rows = t == 0 ? nk : nq;
      f32x16 acc[1];
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[0][i] = 0.f;
#pragma unroll
      for (int rb = 0; rb < R / 32; ++rb) {
        if (rb * 32 >= rows) break;
        if (t == 0) {
          mma_acc_coef<32>(tile, PITCH, rb * 32, coef + R, acc, lane);        // lo first: the small terms accumulate before the large
          mma_acc_coef<32>(tile, PITCH, rb * 32, coef, acc, lane);
        } else {
          mma_acc_coef<32>(tile, PITCH, rb * 32, coef + 2 * R, acc, lane);
        }
      }
      if (r == 0) {                                        // every column holds the same vector: column 0 of each half writes its rows
        const float mul = t == 0 ? p.scale : 1.f;
        float* o2 = outp + (t == 0 ? 0 : 2) * p.h * D + db * 32;
#pragma unroll
        for (int i = 0; i < 16; ++i) o2[acc_row(i, h)] = acc[0][i] * mul;
      }
    }
    if (tid < D) outp[p.h * D + tid] = 0.f;               // dK column sums
  }
}

// ------------------------------------------------------------------------------------------------
// host side: the two symbols attn_kernels.hip calls.  rows: capacity needed (longest sequence, or 128 with groups); items:
// workgroups per head
// ------------------------------------------------------------------------------------------------
#define GMLM_K5_FWD(F, RR) attn_fwd_short_kernel<64, F, RR>
#define GMLM_K5_BWD(F, RR) attn_bwd_short_kernel<64, F, RR>

int attn_short_fwd_launch(const AttnParams& p, int64_t rows, int64_t items, hipStream_t st) {
  static ShortKernels<AttnParams> t{GMLM_SHORT_KERNELS(GMLM_K5_FWD), kShortFwdLds};
  return short_launch(t, short_tile_rows(rows), p.drop_thresh != 0, (unsigned)(items * p.h), st, p);
}

int attn_short_bwd_launch(const AttnParams& p, int64_t rows, int64_t items, float* dbias, hipStream_t st) {
  static ShortKernels<AttnParams> t{GMLM_SHORT_KERNELS(GMLM_K5_BWD), kShortBwdLds};
  const int rc = short_launch(t, short_tile_rows(rows), p.drop_thresh != 0, (unsigned)(items * p.h), st, p);
  if (rc != GMLM_OK || !dbias) return rc;
  return short_bias_sums(p.dbias_part, items, 3 * p.h * 64, dbias, st);
}

}  // namespace gmlm
