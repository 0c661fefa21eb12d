// Device helpers shared by the LDS-resident short-sequence attention kernels (attn_short.hip: one KV head per query head;
// attn_gqa_short.hip: grouped KV heads): the block-diagonal mask step, the row bookkeeping of one work item (a group of
// consecutive sequences of at most R rows) and the wave-uniform range of 32-row blocks a wave has to visit.
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
};

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

}  // namespace gmlm
