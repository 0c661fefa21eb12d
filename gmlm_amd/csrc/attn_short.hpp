// Device side shared by the LDS-resident short-sequence attention kernels (attn_short.hip: K5, d = 64, one KV head per query
// head; attn_gqa_short.hip: gqas::, d = 64, grouped KV heads; attn_d32_short.hip: d32s::, d = 32, a pair of heads per item).  Every
// family stages 64-element row pieces (a d32s row is two heads), so one copy serves all three:
//   mask step, item bookkeeping, block range      onehot_frag / antihot_frag, ShortMeta + short_item_setup, block_range
//   LDS layout                                    ShortLds: the kernels carve with it, the host sizes the launch with it
//   forward                                       short_stage_fwd (K / V -> swizzled images, Q -> registers), short_fwd_d64 (the d = 64 body)
//   backward                                      short_rows_load / short_rows_store (staging at kShortPitch), short_frag,
//                                                 short_bwd_phase1 / short_bwd_phase2 (the block loops of one head)
// What differs between the families in the backward block loops is a policy object (see short_bwd_phase1).  The host side is
// attn_short_host.hpp.
#pragma once
#include "attn_common.hpp"

namespace gmlm {

typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

constexpr int kShortMaxSeq = 13;   // sequences per group: ids 0..12; 14 = padding query row, 15 = padding key row

// A fragment of the mask step for a tile row with sequence id `id`: 1 in column id (elements j = 0..7 <-> columns 8h + j)
__device__ __forceinline__ bf16x8 onehot_frag(int id, int h) {
  const int e = id - 8 * h;
  u32x4 w;
#pragma unroll
  for (int t = 0; t < 4; ++t) w[t] = (e >> 1) == t ? (0x3F80u << (16 * (e & 1))) : 0u;          // bf16 1.0 = 0x3F80
  return __builtin_bit_cast(bf16x8, w);
}
// B fragment of the mask step for the lane's own row: -2^100 (bf16 0xF180) in every column except its sequence id
__device__ __forceinline__ bf16x8 antihot_frag(int id, int h) {
  const int e = id - 8 * h;
  u32x4 w;
#pragma unroll
  for (int t = 0; t < 4; ++t) w[t] = (e >> 1) == t ? (0xF180F180u & ~(0xFFFFu << (16 * (e & 1)))) : 0xF180F180u;
  return __builtin_bit_cast(bf16x8, w);
}

// row bookkeeping of one item, in LDS: sequence id of every Q-side / K-side tile row and the row range a row may attend to
struct ShortMeta {
  uint8_t* qid;      // [R]
  uint8_t* kid;      // [R]
  int16_t* q2k_lo;   // [R] first key row (tile-relative) of the query row's sequence
  int16_t* q2k_hi;   // [R] one past its last key row
  int16_t* k2q_lo;   // [R] same for a key row -> query rows
  int16_t* k2q_hi;   // [R]
  // the meta block of `rows` tile rows at `at` (ShortLds::meta_at): four int16 arrays, then the two id arrays
  __device__ __forceinline__ static ShortMeta carve(void* at, int rows) {
    ShortMeta mt;
    mt.q2k_lo = reinterpret_cast<int16_t*>(at);
    mt.q2k_hi = mt.q2k_lo + rows; mt.k2q_lo = mt.q2k_hi + rows; mt.k2q_hi = mt.k2q_lo + rows;
    mt.qid = reinterpret_cast<uint8_t*>(mt.k2q_hi + rows);
    mt.kid = mt.qid + rows;
    return mt;
  }
};

// LDS of a short kernel at tile height r: `tiles` bf16 tiles of r x pitch elements | `frows` fp32 rows of r | `crows` bf16
// coefficient rows of r | the meta block.  The kernels carve with it and the host asks for bytes(r): one statement of the sizes.
struct ShortLds {
  int tiles, pitch, frows, crows;
  constexpr size_t floats_at(int r) const { return (size_t)tiles * r * pitch * sizeof(bf16_t); }
  constexpr size_t coef_at(int r) const { return floats_at(r) + (size_t)frows * r * sizeof(float); }
  constexpr size_t meta_at(int r) const { return coef_at(r) + (size_t)crows * r * sizeof(bf16_t); }
  constexpr size_t bytes(int r) const { return meta_at(r) + (size_t)r * (4 * sizeof(int16_t) + 2); }
};
constexpr int kShortPitch = 64 + Pad<bf16_t>::v;     // backward tiles: 64-element rows + 8 of padding
constexpr ShortLds kShortFwdLds{2, 64, 0, 0};        // every forward: the swizzled K and V images

// item -> row ranges; fills the meta arrays (threads 0..R-1).  nq / nk = rows of the Q-side / K-side tiles that exist.
template <int R>
__device__ __forceinline__ void short_item_setup(const AttnParams& p, int64_t item, int tid, const ShortMeta& mt, int64_t& qbase,
                                                 int64_t& kbase, int& nq, int& nk, int64_t& lse_base, int64_t hd) {
  if (p.cu) {
    const int s0 = p.groups ? p.groups[item] : (int)item, s1 = p.groups ? p.groups[item + 1] : (int)item + 1;
    const int row0 = p.cu[s0];
    int n = p.cu[s1] - row0;
    n = n < 0 ? 0 : (n > R ? R : n);                          // the host builds groups of <= R rows; never index past the tiles
    qbase = kbase = row0;
    nq = nk = n;
    lse_base = hd * p.lq + row0;                              // lse laid out [h, total_rows]
    if (tid < R) {
      int id = 14, kidv = 15, lo = 0, hi = 0;
      if (tid < n) {
        const int grow = row0 + tid;
        id = 0;
        for (int j = s0 + 1; j < s1; ++j) id += grow >= p.cu[j] ? 1 : 0;
        id = id < kShortMaxSeq ? id : kShortMaxSeq - 1;
        kidv = id;
        lo = p.cu[s0 + id] - row0;
        hi = p.cu[s0 + id + 1] - row0;
        hi = hi > n ? n : hi;
      }
      mt.qid[tid] = (uint8_t)id; mt.kid[tid] = (uint8_t)kidv;
      mt.q2k_lo[tid] = mt.k2q_lo[tid] = (int16_t)lo;
      mt.q2k_hi[tid] = mt.k2q_hi[tid] = (int16_t)hi;
    }
  } else {
    const int64_t b = item;
    qbase = b * p.lq; kbase = b * p.lk;
    nq = (int)p.lq; nk = (int)p.lk;
    int kvl = nk;
    if (p.kv_len) { kvl = p.kv_len[b]; kvl = kvl > nk ? nk : (kvl < 0 ? 0 : kvl); }
    lse_base = (b * p.h + hd) * p.lq;
    if (tid < R) {
      mt.qid[tid] = tid < nq ? 0 : 14;
      mt.kid[tid] = tid < kvl ? 0 : 15;
      mt.q2k_lo[tid] = 0; mt.q2k_hi[tid] = (int16_t)kvl;
      mt.k2q_lo[tid] = 0; mt.k2q_hi[tid] = (int16_t)((tid & ~31) < kvl ? nq : 0);      // per 32-key block: any valid key -> all query rows
    }
  }
}

// wave-uniform range of 32-row blocks on the OTHER side that rows [32w, 32w + 32) of this side (n rows exist) can touch
__device__ __forceinline__ void block_range(const int16_t* lo, const int16_t* hi, int w, int n, int& b0, int& b1) {
  const int first = 32 * w, last = (32 * w + 31 < n ? 32 * w + 31 : n - 1);
  int l = lo[first], hgh = hi[last < first ? first : last];
  l = __builtin_amdgcn_readfirstlane(l);
  hgh = __builtin_amdgcn_readfirstlane(hgh);
  b0 = l >> 5;
  b1 = (hgh + 31) >> 5;
}

// ------------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------------
// Staging of a forward item (2 R threads): K and V rows [0, nk) of a 64-element row piece -> registers -> the swizzled d = 64
// images (attn_common.hpp), all loads in flight at once; the lane's own query row -> its B-operand registers, issued with
// them (a query row is used by its own lane pair alone: q_row = 32 w + r, half h).  Closes with the barrier.
template <int R>
__device__ __forceinline__ void short_stage_fwd(const AttnParams& p, const bf16_t* qg, const bf16_t* kg, const bf16_t* vg, int nq, int nk,
                                                bf16_t* tk, bf16_t* tv, RowFrag<bf16_t, 64>& qf, int tid, int q_row, int h) {
  constexpr int NT = 2 * R, CPR = 8, PER = R * CPR / NT;
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
    *reinterpret_cast<uint4*>(tk + row * 64 + ((c ^ sw_row(row)) << 3)) = rk[k];
    *reinterpret_cast<uint4*>(tv + row * 64 + ((c ^ sw_tr(row)) << 3)) = rv[k];
  }
  __syncthreads();
}

constexpr float kShortMasked = -1.2676506e30f;   // -2^100, the value of the block-diagonal mask step: exp2 of it is exactly 0

// The d = 64 forward of one (item, query head hd) with K / V of head kvh: attn_fwd_short_kernel (kvh = hd) and gqas::fwd_kernel
// (kvh = hd / group) are this body.  All keys of a row are resident, so the softmax is two plain passes over the score blocks
// held in registers.  CAUSAL: inside a group tile-row order is position order within each sequence, so key blocks above the
// wave's own are skipped and the diagonal block alone takes a select.
template <bool DROP, bool CAUSAL, int R>
__device__ __forceinline__ void short_fwd_d64(const AttnParams& p, int64_t item, int64_t hd, int64_t kvh) {
  using T = bf16_t;
  constexpr int D = 64, DB = D / 32, NB = R / 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  T* tk = reinterpret_cast<T*>(smem_raw);
  T* tv = tk + R * D;
  const ShortMeta mt = ShortMeta::carve(smem_raw + kShortFwdLds.meta_at(R), R);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  int64_t qbase, kbase, lse_base;
  int nq, nk;
  short_item_setup<R>(p, item, tid, mt, qbase, kbase, nq, nk, lse_base, hd);
  // Only K and V are staged (they are MFMA A operands of every wave): 32 KB at R = 128 = five workgroups per CU, and with them
  // five items' worth of loads in flight per CU.
  const int q_row = w * 32 + r;
  RowFrag<T, D> qf;
  short_stage_fwd<R>(p, static_cast<const T*>(p.q) + qbase * p.q_stride + hd * D, static_cast<const T*>(p.k) + kbase * p.k_stride + kvh * D,
                     static_cast<const T*>(p.v) + kbase * p.v_stride + kvh * D, nq, nk, tk, tv, qf, tid, q_row, h);
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
    s[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(onehot_frag(mt.kid[kb * 32 + r], h), qm, z, 0, 0, 0);   // block-diagonal / padding mask
    mma_rows_sw(tk, kb * 32, qf, s[kb], r, h);
    if (CAUSAL && kb == w) {                                  // the diagonal block: key tile row <= query tile row
#pragma unroll
      for (int i = 0; i < 16; ++i) s[kb][i] = acc_row(i, h) <= r ? s[kb][i] : kShortMasked;
    }
    rmax = fmaxf(rmax, max16(s[kb]));
  }
  const float m = b1 > b0 ? xhalf_max(rmax) * sl2 : 0.f;      // finite for a real query row (its own sequence has >= 1 key)
  const uint32_t dq_u = drop_base(attn_seed(p), lse_base) + (uint32_t)(q_row >> 1) * kDropC1 + (uint32_t)(2 * h) * kDropC2;
  const int q_odd = q_row & 1;
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
      l += e0 + e1;                                           // the normaliser uses the un-dropped probabilities
      float m0 = 1.f, m1 = 1.f;
      if (DROP) drop_pair_q(dq_u + (uint32_t)((kb * 32 + acc_row(i, 0)) >> 1) * kDropC2, q_odd, p.drop_thresh, p.keep_scale, m0, m1);
      s[kb][i] = e0 * m0;
      s[kb][i + 1] = e1 * m1;
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
// backward
// ------------------------------------------------------------------------------------------------
// Staging (2 R threads): the 64-element row pieces of N tensors -> registers, all loads first (32-bit offsets: rows <= 128,
// strides < 2^24).  The tensors come in pairs that share a row bound, rows [0, n[t / 2]): K, V | Q, dO ...
template <int R, int N>
__device__ __forceinline__ void short_rows_load(uint4 (&rg)[N][4], const bf16_t* const (&g)[N], const int (&stride)[N],
                                                const int (&n)[N / 2], int tid) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + k * 2 * R, row = i / 8, col = (i % 8) * 8;
#pragma unroll
    for (int t = 0; t < N; ++t) rg[t][k] = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int t = 0; t < N; t += 2)
      if (row < n[t / 2]) {
        rg[t][k] = *reinterpret_cast<const uint4*>(g[t] + (uint32_t)(row * stride[t] + col));
        rg[t + 1][k] = *reinterpret_cast<const uint4*>(g[t + 1] + (uint32_t)(row * stride[t + 1] + col));
      }
  }
}
// ... then the LDS images at kShortPitch
template <int R, int N>
__device__ __forceinline__ void short_rows_store(bf16_t* const (&tile)[N], const uint4 (&rg)[N][4], int tid) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = tid + k * 2 * R, row = i / 8, col = (i % 8) * 8;
#pragma unroll
    for (int t = 0; t < N; ++t) *reinterpret_cast<uint4*>(tile[t] + row * kShortPitch + col) = rg[t][k];
  }
}
// MFMA B-operand fragment of a staged row (D = 64), or of one head's half of it (D = 32, tile + head * 32)
template <int D>
__device__ __forceinline__ void short_frag(const bf16_t* tile, int row, int h, RowFrag<bf16_t, D>& f) {
#pragma unroll
  for (int s = 0; s < D / 16; ++s) f.v[s] = *reinterpret_cast<const bf16x8*>(tile + row * kShortPitch + 16 * s + 8 * h);
}

// The block loops of one head take a policy `pol` for what the families do to a register pair (i, i + 1) of 32-row block b of
// the OTHER side (tile rows 32 b + acc_row(i, h), + 1):
//   pol.bias                           accumulate the bias coefficients (pm in phase 1, ck in phase 2)
//   pol.pair_q / pol.pair_k(b, i, p0, p1, m0, m1)    query / key on the lane: may zero the probabilities p0, p1 (the causal
//                                      diagonal) and sets the multipliers m0, m1 of dP and P' (dropout; 1 otherwise)
// (the causal clamp of the block range is the caller's, next to its block_range call).
//
// Phase 1 of one head (query row 32 w + r on the lane; K, V tiles as MFMA A operands).  Pass A: P and dP' (= dP through the
// dropout mask) of every key block in [b0, b1), kept in registers; delta = sum_k P dP' IN FP32, written to dl_s.  Pass B:
// dS = P (dP' - delta); dQ^T += K^T dS^T, unscaled, in dq.  Returns this half-wave's share of pm = sum_k P'[q,k].
template <int D, int R, class Pol>
__device__ __forceinline__ float short_bwd_phase1(const bf16_t* tk, const bf16_t* tv, const bf16_t* tq, const bf16_t* tdo, const float* lse_s,
                                                  float* dl_s, const ShortMeta& mt, const bf16x8& qm, int b0, int b1, float sl2,
                                                  const Pol& pol, int q_row, int lane, f32x16 (&dq)[D / 32]) {
  constexpr int NB = R / 32;
  const int r = lane & 31, h = lane >> 5;
  RowFrag<bf16_t, D> qf, dof;
  short_frag<D>(tq, q_row, h, qf);
  short_frag<D>(tdo, q_row, h, dof);
  const float lse2 = lse_s[q_row];
  f32x16 pr[NB], dpm[NB];
  float dsum = 0.f, pm = 0.f;                               // this half-wave's shares of delta and of sum_k P'[q,k]
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) {
    if (kb < b0 || kb >= b1) continue;                      // wave-uniform
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) { z[i] = 0.f; dpm[kb][i] = 0.f; }
    pr[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(onehot_frag(mt.kid[kb * 32 + r], h), qm, z, 0, 0, 0);
    mma_rows<D>(tk, kShortPitch, kb * 32, qf, pr[kb], r, h);
    mma_rows<D>(tv, kShortPitch, kb * 32, dof, dpm[kb], r, h);
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      float p0 = fast_exp2(fmaf(pr[kb][i], sl2, -lse2)), p1 = fast_exp2(fmaf(pr[kb][i + 1], sl2, -lse2));   // masked: exactly 0
      float m0 = 1.f, m1 = 1.f;
      pol.pair_q(kb, i, p0, p1, m0, m1);
      const float d0 = dpm[kb][i] * m0, d1 = dpm[kb][i + 1] * m1;
      dsum = fmaf(p1, d1, fmaf(p0, d0, dsum));
      if (pol.bias) pm = fmaf(p1, m1, fmaf(p0, m0, pm));
      pr[kb][i] = p0; pr[kb][i + 1] = p1;
      dpm[kb][i] = d0; dpm[kb][i + 1] = d1;
    }
  }
  const float dl = xhalf_sum(dsum);
  if (h == 0) dl_s[q_row] = dl;
#pragma unroll
  for (int d = 0; d < D / 32; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) dq[d][i] = 0.f;
#pragma unroll
  for (int kb = 0; kb < NB; ++kb) {
    if (kb < b0 || kb >= b1) continue;
#pragma unroll
    for (int i = 0; i < 16; ++i) pr[kb][i] *= dpm[kb][i] - dl;
    mma_acc<D>(tk, kShortPitch, kb * 32, pr[kb], dq, lane);
  }
  return pm;
}

// Phase 2 of one head (key row `key` on the lane; Q, dO tiles as MFMA A operands) over the query blocks [b0, b1): lse and delta
// from LDS as float4, dV += P'^T dO and dK += dS^T Q (unscaled) on top of what dk / dv hold.  Returns this half-wave's share of
// ck = sum_q dS[q,key].
template <int D, int R, class Pol>
__device__ __forceinline__ float short_bwd_phase2(const bf16_t* tk, const bf16_t* tv, const bf16_t* tq, const bf16_t* tdo, const float* lse_s,
                                                  const float* dl_s, const ShortMeta& mt, const bf16x8& km, int b0, int b1, float sl2,
                                                  const Pol& pol, int key, int lane, f32x16 (&dk)[D / 32], f32x16 (&dv)[D / 32]) {
  constexpr int NB = R / 32;
  const int r = lane & 31, h = lane >> 5;
  RowFrag<bf16_t, D> kf, vf;
  short_frag<D>(tk, key, h, kf);
  short_frag<D>(tv, key, h, vf);
  float ck = 0.f;                                           // this half-wave's share of sum_q dS[q,key]
#pragma unroll
  for (int qb = 0; qb < NB; ++qb) {
    if (qb < b0 || qb >= b1) continue;                      // wave-uniform
    f32x16 s, dp, z;
#pragma unroll
    for (int i = 0; i < 16; ++i) { z[i] = 0.f; dp[i] = 0.f; }
    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(onehot_frag(mt.qid[qb * 32 + r], h), km, z, 0, 0, 0);
    mma_rows<D>(tq, kShortPitch, qb * 32, kf, s, r, h);
    mma_rows<D>(tdo, kShortPitch, qb * 32, vf, dp, r, h);
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int q4 = qb * 32 + 8 * g4 + 4 * h;               // accumulator registers 4*g4 .. 4*g4+3 = queries q4 .. q4+3
      const float4 l4 = *reinterpret_cast<const float4*>(lse_s + q4);
      const float4 d4 = *reinterpret_cast<const float4*>(dl_s + q4);
      const float lq4[4] = {l4.x, l4.y, l4.z, l4.w}, dq4[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int j = 0; j < 4; j += 2) {
        const int i = 4 * g4 + j;                            // registers i, i+1 = queries q4 + j, + 1 (even, odd tile rows)
        // rows past the item carry lse = +inf in LDS, other sequences' rows / padding keys sit at -1.3e30: probability 0
        float p0 = fast_exp2(fmaf(s[i], sl2, -lq4[j])), p1 = fast_exp2(fmaf(s[i + 1], sl2, -lq4[j + 1]));
        float m0 = 1.f, m1 = 1.f;
        pol.pair_k(qb, i, p0, p1, m0, m1);
        s[i] = p0 * m0;
        s[i + 1] = p1 * m1;
        const float x1 = dp[i + 1] * m1 - dq4[j + 1];
        dp[i] = p0 * (dp[i] * m0 - dq4[j]);
        dp[i + 1] = p1 * x1;
        // dS[i] + dS[i + 1] with the second product fused into the sum: what the compiler's contraction made of the plain sum in
        // the kernels this body came from, written out so that the bits of the bias sums do not hang on that choice
        if (pol.bias) ck += fmaf(p1, x1, dp[i]);
      }
    }
    mma_acc<D>(tdo, kShortPitch, qb * 32, s, dv, lane);
    mma_acc<D>(tq, kShortPitch, qb * 32, dp, dk, lane);
  }
  return ck;
}

}  // namespace gmlm
