// Self-attention with a learned relative-position bias at head dim 64, forward + backward, gfx950 MFMA
// (gmlm_attention_relbias_*; C ABI in include/gmlm_hip_relbias.h): the attention of an MPNet encoder, whose scores are
//     s_ij = q_i . k_j * scale + rel_bias[h, M - 1 + (j - i)]
// with one fp32 table [h, 2M - 1] shared by all layers.  Padded layout [b, l, h*64] with row strides and an optional key count
// per sequence, or packed [total_rows, h*64] with cu_seqlens (positions relative to the start of each sequence).
// The forward, dQ and dK/dV kernels ARE the streaming bodies of attn_stream.hpp instantiated with their BIAS template flag
// (default false: the existing kernels' instantiations are unchanged) at D = 64, 4 waves = 128 rows per workgroup; bf16: 64-row
// K / V tiles and 32-row Q / dO tiles, double-buffered in LDS; fp32: 32-row tiles, one buffer.  What the flag changes: each
// score gets bias * log2 e in the exp2 domain, one 4-byte load per score through the vector cache (a head's table is at most
// 4,092 bytes and stays resident; staging it in LDS would add to the 36 KiB of the bf16 tile buffers and put its reads on the
// pipe that already feeds every MFMA operand, while the vector memory pipe idles inside the key loop).
// The gradient of the table is two kernels of its own (dbias_kernel, dbias_sum_kernel; see dbias_body), not more state in the dQ
// body.  1-D grids of (tile, (batch or sequence, head)) work items.  Every sum runs in a fixed order with no atomics.
// The argument checks and the AttnParams filling shared with the other attention entry points are in attn_host.hpp.
#include "attn_stream.hpp"
#include "attn_host.hpp"
#include "../../include/gmlm_hip_relbias.h"

namespace gmlm {
namespace relb {

constexpr int D = 64, NW = 4, NT = NW * 64, BQ = NW * 32;
constexpr int ROW = 2 * GMLM_RELBIAS_MAX_LEN;      // LDS floats of one wave's gradient row (>= 2M - 1)
constexpr int TP = 33;                             // pitch of a wave's 32 x 32 dS tile in LDS: a diagonal walks all banks

struct RelParams {
  AttnParams a;
  const float* bias;     // [h, 2m - 1]
  float* dpart;          // [tiles * b, h, 2m - 1] partial gradient rows
  int m;
};

// Cfg<T> (tile sizes) is attn_stream.hpp's, decode() (1-D grid -> tile, sequence, head) attn_common.hpp's

// forward: workgroup = 128 query rows of one (sequence, head), loop over key tiles
template <typename T, bool DROP>
__global__ __launch_bounds__(NT) void fwd_kernel(RelParams x) {
  const Item it = decode(x.a);
  attn_fwd_body<T, D, NW, DROP, Cfg<T>::KT, Cfg<T>::DBUF, false, false, false, true>(x.a, it.tile, it.b, it.hd, x.a.h * D, 0, 0, x.bias, x.m);
}

// backward: delta = rowsum(dO * O) over rows of [b * l, h, 64] (O = out + out_lo when the forward stored the residual)
template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                    int64_t rows /* b * l * h */, int64_t lq, int64_t hn, float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);
}

// backward: dQ.  workgroup = 128 queries of one (sequence, head), loop over key tiles
template <typename T, bool DROP>
__global__ __launch_bounds__(NT) void dq_kernel(RelParams x) {
  const Item it = decode(x.a);
  attn_dq_body<T, D, NW, DROP, Cfg<T>::KT, Cfg<T>::DBUF, false, false, false, true>(x.a, it.tile, it.b, it.hd, x.a.h * D, 0, 0, x.bias, x.m);
}

// backward: dK, dV.  workgroup = 128 keys of one (sequence, head), loop over query tiles in order
template <typename T, bool DROP>
__global__ __launch_bounds__(NT) void dkv_kernel(RelParams x) {
  const Item it = decode(x.a);
  attn_dkv_body<T, D, NW, DROP, Cfg<T>::QT, Cfg<T>::DBUF, false, true>(x.a, it.tile, it.b, it.hd, x.a.h * D, 0, x.bias, x.m);
}

// ------------------------------------------------------------------------------------------------
// backward: the table's gradient, first pass.  workgroup = 128 queries of one (sequence, head), loop over key tiles, as dQ:
//   S^T = K Q^T, P^T = exp2(S^T * scale * log2 e + bias * log2 e - lse * log2 e), dP^T = V dO^T, dS^T = P^T * (D * dP^T - delta)
// with the query on the lane and the 16 accumulator registers over the keys of a 32-key block.  Q is NOT pre-scaled here
// (bf16: one rounding less than the dQ kernel's folded form); masked keys and rows past the sequence select the exponent -inf.
// Each wave puts its 32 x 32 dS tile in LDS ([key][query], pitch 33), then lane d = 1 .. 63 sums diagonal key - query = d - 32
// over the queries 0 .. 31 in order and adds the sum to entry M - 1 + (first key - first query) + d - 32 of the wave's own row
// of [2M - 1] floats in LDS (a lane owns its entry: no race; the tile and the row are the wave's own, so the exchange needs
// no workgroup barrier).  After the key loop the four rows are summed in wave order and stored as the work item's partial row;
// a work item past its sequence stores zeros.  LDS: bf16 36,864 (K / V) + 16,896 (tiles) + 16,384 (rows) = 70,144 bytes,
// fp32 17,408 + 16,896 + 16,384 = 50,688 bytes.
// ------------------------------------------------------------------------------------------------
template <typename T, bool DROP, int KT, bool DBUF>
__device__ __forceinline__ void dbias_body(const RelParams& x, int64_t tile, int64_t b, int64_t hd, int64_t o_stride,
                                           float* __restrict__ part_row) {
  const AttnParams& p = x.a;
  constexpr int KB = KT / 32, PITCH = D + Pad<T>::v, NBUF = DBUF ? 2 : 1;
  __shared__ __attribute__((aligned(16))) T ks[NBUF][KT * PITCH];
  __shared__ __attribute__((aligned(16))) T vs[NBUF][KT * PITCH];
  __shared__ float ds_s[NW][32 * TP];
  __shared__ float row_s[NW][ROW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  const int m = x.m, width = 2 * m - 1;
  for (int i = tid; i < NW * ROW; i += NT) (&row_s[0][0])[i] = 0.f;
  int64_t lq_, lk_, qbase, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, qbase, kbase, lse_base);
  if (tile * BQ < lq_) {                                    // else (varlen): tile past this sequence (block-uniform): zeros
    const int64_t q_row = tile * BQ + w * 32 + r;
    const bool q_ok = q_row < lq_;
    const bool wave_live = tile * BQ + w * 32 < lq_;        // else: staging helper only
    const int64_t kvlen = clamp_kvlen(p, b, lk_);
    const int64_t qr = q_ok ? q_row : 0;
    const T* kg = static_cast<const T*>(p.k) + kbase * p.k_stride + hd * D;
    const T* vg = static_cast<const T*>(p.v) + kbase * p.v_stride + hd * D;
    RowFrag<T, D> qf, dof;
    qf.load(static_cast<const T*>(p.q) + (qbase + qr) * p.q_stride + hd * D, q_ok, h);
    dof.load(static_cast<const T*>(p.dout) + (qbase + qr) * o_stride + hd * D, q_ok, h);
    const float sl2 = p.scale * kLog2e;
    const float lse2 = q_ok ? p.lse[lse_base + q_row] * kLog2e : INFINITY;   // +inf: probability 0 for a row past the sequence
    const float dl = q_ok ? p.delta[lse_base + q_row] : 0.f;
    const int kvl = (int)(kvlen < (1 << 30) ? kvlen : (1 << 30));
    const int qi = (int)(q_row < (1 << 30) ? q_row : (1 << 30));
    const uint32_t dq_u = drop_base(attn_seed(p), lse_base) + (uint32_t)(q_row >> 1) * kDropC1 + (uint32_t)(2 * h) * kDropC2;
    const int q_odd = (int)(q_row & 1);
    const float* bh = x.bias + hd * width + (m - 1);        // entry 0 = the diagonal
    const int q_wave0 = (int)(tile * BQ) + w * 32;          // tile * BQ < lq_ < 2^30 (host check)
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
          const int kvb = (int)kv0 + kb * 32;               // first key of the block
          if (kvb >= kvl) continue;                         // block-uniform: no key of the block takes part
          f32x16 s, dp;
#pragma unroll
          for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
          mma_rows<D>(ks[cur], PITCH, kb * 32, qf, s, r, h);
          mma_rows<D>(vs[cur], PITCH, kb * 32, dof, dp, r, h);
#pragma unroll
          for (int i = 0; i < 16; i += 2) {
            const int kl = acc_row(i, h), key = kvb + kl;   // even; registers i, i + 1 = keys key, key + 1
            const int rel = key - qi, lo = 1 - m, hi = m - 1;
            const float b0 = bh[rel < lo ? lo : (rel > hi ? hi : rel)] * kLog2e;
            const float b1 = bh[rel + 1 < lo ? lo : (rel + 1 > hi ? hi : rel + 1)] * kLog2e;
            const float a0 = key < kvl ? fmaf(s[i], sl2, b0 - lse2) : -INFINITY;
            const float a1 = key + 1 < kvl ? fmaf(s[i + 1], sl2, b1 - lse2) : -INFINITY;
            const float p0 = fast_exp2(a0), p1 = fast_exp2(a1);
            float m0 = 1.f, m1 = 1.f;
            if (DROP) drop_pair_q(dq_u + ((uint32_t)(t * (KT / 2)) + (uint32_t)((kb * 32 + acc_row(i, 0)) >> 1)) * kDropC2, q_odd, p.drop_thresh, p.keep_scale, m0, m1);
            ds_s[w][kl * TP + r] = p0 * (dp[i] * m0 - dl);
            ds_s[w][(kl + 1) * TP + r] = p1 * (dp[i + 1] * m1 - dl);
          }
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          // lane = diagonal lane - 32 of the tile (lane 0: none); queries in order
          float acc = 0.f;
#pragma unroll
          for (int q = 0; q < 32; ++q) {
            const int kk = q + lane - 32;
            acc += (kk >= 0 && kk < 32) ? ds_s[w][(kk & 31) * TP + q] : 0.f;
          }
          const int idx = (m - 1) + kvb - q_wave0 + lane - 32;
          if (lane > 0 && idx >= 0 && idx < width) row_s[w][idx] += acc;
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
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
  }
  __syncthreads();
  // one chain per entry, one entry per trip: the loop vectoriser pairs the trips into v_pk_add_f32 otherwise (Makefile)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
  for (int i = tid; i < width; i += NT) part_row[i] = ((row_s[0][i] + row_s[1][i]) + row_s[2][i]) + row_s[3][i];
}

template <typename T, bool DROP>
__global__ __launch_bounds__(NT) void dbias_kernel(RelParams x) {
  const Item it = decode(x.a);
  // partial rows [tile * b + sequence][head][2m - 1]: the second pass sums over the first index
  float* row = x.dpart + ((it.tile * x.a.b + it.b) * x.a.h + it.hd) * (int64_t)(2 * x.m - 1);
  dbias_body<T, DROP, Cfg<T>::KT, Cfg<T>::DBUF>(x, it.tile, it.b, it.hd, x.a.h * D, row);
}

// backward: the table's gradient, second pass.  out[c] = sum_r part[r][c] over the nrows partial rows of width h * (2m - 1):
// block = 32 columns x 8 row lanes, four loads in flight per lane, fixed-order LDS tree (the shape of colreduce.hpp's second pass)
__global__ __launch_bounds__(256) void dbias_sum_kernel(const float* __restrict__ part, int64_t nrows, int64_t width,
                                                        float* __restrict__ out) {
  __shared__ float red[8][32];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t c = (int64_t)blockIdx.x * 32 + tx;
  float acc = 0.f;
  if (c < width) {
    int64_t rr = ty;
    for (; rr + 24 < nrows; rr += 32) {
      const float a0 = part[rr * width + c], a1 = part[(rr + 8) * width + c];
      const float a2 = part[(rr + 16) * width + c], a3 = part[(rr + 24) * width + c];
      acc += (a0 + a1) + (a2 + a3);
    }
    for (; rr < nrows; rr += 8) acc += part[rr * width + c];
  }
  red[ty][tx] = acc;
  __syncthreads();
  if (ty == 0 && c < width)
    out[c] = ((red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx])) + ((red[4][tx] + red[5][tx]) + (red[6][tx] + red[7][tx]));
}

// rows of the call that decide the grid and bound the table: l padded, max_len packed
static inline int64_t call_rows(int64_t lq, const int32_t* cu_seqlens, int64_t max_len) { return cu_seqlens ? max_len : lq; }

// bytes of delta, rounded up to 16 so that the partial rows behind it stay aligned
static inline size_t delta_bytes16(int64_t nb, int64_t h, int64_t lq) { return (attn_delta_bytes(nb, h, lq) + 15) & ~(size_t)15; }
static inline size_t part_bytes(int64_t b, int64_t h, int64_t rows, int64_t m) {
  return (size_t)(b > 0 && h > 0 && rows > 0 && m > 0 ? cdiv(rows, (int64_t)BQ) * b * h * (2 * m - 1) : 1) * sizeof(float);
}

// the checks of attn_host.hpp up to the empty-problem return, with this family's head dim, layout rules, table bound and
// work-item bound; fills the launch parameters
static int setup(const char* who, RelParams& x, const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b,
                 int64_t h, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                 float dropout_p, uint64_t seed, const uint64_t* seed_dev, int64_t rel_m, const void* out_lo, int dtype,
                 const int32_t* cu_seqlens, int64_t max_len) {
  int rc = attn_check_shape(who, b >= 0 && h > 0 && lq >= 0 && lk >= 0, d == 64, d, "this entry point takes 64", dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(lq == lk, "%s: self-attention with a relative-position bias needs lq == lk (got %ld and %ld)", who, (long)lq, (long)lk);
  GMLM_REQUIRE(!cu_seqlens || (max_len > 0 && !kv_len), "%s: packed mode needs lq == lk = total rows, max_len > 0, kv_len NULL", who);
  const int64_t rows = call_rows(lq, cu_seqlens, max_len);
  GMLM_REQUIRE(rel_m >= rows && rel_m >= 1 && rel_m <= GMLM_RELBIAS_MAX_LEN,
               "%s: rel_m %ld must be in [%ld, %d] (the longest sequence of the call up to GMLM_RELBIAS_MAX_LEN)", who, (long)rel_m,
               (long)(rows > 1 ? rows : 1), GMLM_RELBIAS_MAX_LEN);
  if ((rc = attn_check_rates(who, dropout_p, nullptr, scale)) != GMLM_OK) return rc;
  // each factor and each partial product is bounded before the next multiply: no int64 overflow on the way to the answer
  const int64_t tiles = cdiv(rows, (int64_t)BQ), lim = (int64_t)1 << 31;
  GMLM_REQUIRE(lq < ((int64_t)1 << 30) && b < lim && h < lim && b * h < lim && tiles * (b * h) < lim, "%s: too many work items", who);
  x = RelParams{};
  attn_fill(x.a, q, k, v, kv_len, b, h, lq, lk, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev);
  x.a.cu = cu_seqlens;
  x.m = (int)rel_m;
  return GMLM_OK;
}

}  // namespace relb
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::relb;

#define GMLM_RELB_LAUNCH_T(KERNEL, T, grid, st, prm)                         \
  do {                                                                       \
    if ((prm).a.drop_thresh) KERNEL<T, true><<<grid, NT, 0, st>>>(prm);      \
    else KERNEL<T, false><<<grid, NT, 0, st>>>(prm);                         \
  } while (0)
#define GMLM_RELB_LAUNCH(KERNEL, grid, st, prm)                              \
  do {                                                                       \
    if (dtype == GMLM_BF16) GMLM_RELB_LAUNCH_T(KERNEL, bf16_t, grid, st, prm); \
    else GMLM_RELB_LAUNCH_T(KERNEL, float, grid, st, prm);                   \
  } while (0)

extern "C" int gmlm_attention_relbias_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                                          int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                          float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev,
                                          const float* rel_bias, int64_t rel_m, void* out, void* out_lo, float* lse, int dtype,
                                          const int32_t* cu_seqlens, int64_t max_len, gmlm_stream_t stream) {
  static const char* who = "attention_relbias_fwd";
  RelParams x;
  int rc = setup(who, x, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev, rel_m,
                 out_lo, dtype, cu_seqlens, max_len);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, h * D, h * D, dtype)) != GMLM_OK) return rc;
  GMLM_REQUIRE(rel_bias && aligned16(rel_bias), "%s: null or misaligned rel_bias", who);
  x.bias = rel_bias;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(cdiv(call_rows(lq, cu_seqlens, max_len), (int64_t)BQ) * b * h));
  GMLM_RELB_LAUNCH(fwd_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_relbias_workspace_bytes(int64_t b, int64_t h, int64_t lq, int64_t max_len, int64_t rel_m) {
  const bool packed = max_len > 0;
  return delta_bytes16(packed ? 1 : b, h, lq) + part_bytes(b, h, packed ? max_len : lq, rel_m);
}

extern "C" int gmlm_attention_relbias_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                          const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t h,
                                          int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                          float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev,
                                          const float* rel_bias, int64_t rel_m, void* dq, void* dk, void* dv, float* d_rel_bias,
                                          int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                          const int32_t* cu_seqlens, int64_t max_len, void* workspace, size_t workspace_bytes,
                                          gmlm_stream_t stream) {
  static const char* who = "attention_relbias_bwd";
  RelParams x;
  int rc = setup(who, x, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev, rel_m,
                 out_lo, dtype, cu_seqlens, max_len);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  AttnParams& p = x.a;
  const int64_t nb = cu_seqlens ? 1 : b;        // delta: packed tensors are one [total_rows, h, 64] block, delta is [h, total_rows]
  const int64_t rows = call_rows(lq, cu_seqlens, max_len), tiles = cdiv(rows, (int64_t)BQ);
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  GMLM_REQUIRE(rel_bias && aligned16(rel_bias), "%s: null or misaligned rel_bias", who);
  GMLM_REQUIRE(d_rel_bias && aligned16(d_rel_bias), "%s: null or misaligned d_rel_bias", who);
  if ((rc = attn_check_bwd_operands(who, p, h * D, h * D, dtype, workspace_bytes, delta_bytes16(nb, h, lq) + part_bytes(b, h, rows, rel_m))) != GMLM_OK)
    return rc;
  x.bias = rel_bias;
  x.dpart = reinterpret_cast<float*>(static_cast<char*>(workspace) + delta_bytes16(nb, h, lq));
  hipStream_t st = as_stream(stream);
  const int64_t drows = nb * lq * h;
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, drows, dtype == GMLM_BF16 ? 8 : 16, st, lq, h);   // attn_delta_body: 64 / V lanes per row
  GMLM_LAUNCH_CHECK();
  const dim3 grid((unsigned)(tiles * b * h));
  GMLM_RELB_LAUNCH(dq_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  GMLM_RELB_LAUNCH(dkv_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  GMLM_RELB_LAUNCH(dbias_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  const int64_t width = h * (2 * rel_m - 1);
  dbias_sum_kernel<<<(unsigned)cdiv(width, (int64_t)32), 256, 0, st>>>(x.dpart, tiles * b, width, d_rel_bias);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
