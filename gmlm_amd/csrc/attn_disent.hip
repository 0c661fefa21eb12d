// Disentangled self-attention at head dim 64, forward + backward, gfx950 MFMA (gmlm_attention_disent_*; C ABI in
// include/gmlm_hip_disent.h): the attention of a DeBERTa-v2 / v3 encoder, whose scores are
//     s_ij = (q_i . k_j + C[i, col[i - j]] + Pt[j, col[i - j]]) * scale
// with two fp32 tables of one row of W columns per (head, token), C = Q Kr^T (content-to-position) and Pt = K Qr^T
// (position-to-content), and one int32 column table col[2M - 1] over the relative positions i - j of a sequence.  Padded
// layout [b, l, h*64] with row strides and an optional key count per sequence, or packed [total_rows, h*64] with cu_seqlens.
// The forward, dQ and dK/dV kernels ARE the streaming bodies of attn_stream.hpp instantiated with their DISENT template flag
// (default false: every other instantiation is unchanged) at D = 64, 4 waves = 128 rows per workgroup, with the tile sizes of
// attn_relbias.hip.  The table entries are read through the vector cache, two 4-byte loads per score next to one load of the
// column: with the key in the register and the query on the lane (forward, dQ) the Pt loads of one register are 32 neighbouring
// columns of ONE row, and a lane's 16 C loads walk one row; staging a work item's table tile in LDS would need a skewed
// [128 x (128 + KT)] fp32 image per tile (82 KiB at KT = 32) next to the K / V buffers for data that is read once.
// The gradients of the two tables are one kernel body of their own (dtab_body), launched once per table.  1-D grids of (tile,
// (batch or sequence, head)) work items.  Every sum runs in a fixed order with no atomics.
#include "attn_stream.hpp"
#include "attn_host.hpp"
#include "../../include/gmlm_hip_disent.h"

namespace gmlm {
namespace disent {

constexpr int D = 64, NW = 4, NT = NW * 64, BQ = NW * 32;
constexpr int TP = 33;                             // pitch of a wave's 32 x 32 dS tile in LDS: a column walk crosses all banks

struct DisParams {
  AttnParams a;
  DisentTabs t;
  float* dc;             // [h, rows, w] gradient of t.c
  float* dpt;            // [h, rows, w] gradient of t.pt
};

// Cfg<T> (tile sizes) is attn_stream.hpp's, decode() (1-D grid -> tile, sequence, head) attn_common.hpp's

template <typename T, bool DROP>
__global__ __launch_bounds__(NT) void fwd_kernel(DisParams x) {
  const Item it = decode(x.a);
  attn_fwd_body<T, D, NW, DROP, Cfg<T>::KT, Cfg<T>::DBUF, false, false, false, false, true>(x.a, it.tile, it.b, it.hd, x.a.h * D, 0, 0,
                                                                                            nullptr, 0, &x.t);
}

template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                    int64_t rows /* b * l * h */, int64_t lq, int64_t hn, float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);
}

template <typename T, bool DROP>
__global__ __launch_bounds__(NT) void dq_kernel(DisParams x) {
  const Item it = decode(x.a);
  attn_dq_body<T, D, NW, DROP, Cfg<T>::KT, Cfg<T>::DBUF, false, false, false, false, true>(x.a, it.tile, it.b, it.hd, x.a.h * D, 0, 0,
                                                                                           nullptr, 0, &x.t);
}

template <typename T, bool DROP>
__global__ __launch_bounds__(NT) void dkv_kernel(DisParams x) {
  const Item it = decode(x.a);
  attn_dkv_body<T, D, NW, DROP, Cfg<T>::QT, Cfg<T>::DBUF, false, false, true>(x.a, it.tile, it.b, it.hd, x.a.h * D, 0, nullptr, 0, &x.t);
}

// ------------------------------------------------------------------------------------------------
// backward: the gradient of one table.  PT = false: dC[row i][w] = sum over the keys j with col[i - j] = w of dS_ij;
// PT = true: dPt[row j][w] = sum over the queries i with col[i - j] = w of dS_ij.
// workgroup = 128 rows x of one (sequence, head) - queries (dC) or keys (dPt) - with x on the lane, and a loop over tiles of
// the other index y - keys or queries - staged in LDS, as dQ and dK/dV do:
//   S = A fa^T, P = exp2((S + C + Pt) * scale * log2 e - lse * log2 e), dP = B fb^T, dS = P * (D * dP - delta)
// with (A, B) = (K, V) tiles and (fa, fb) = the lane's (Q, dO) rows for dC, (Q, dO) tiles and the lane's (K, V) rows for dPt;
// lse and delta belong to the query: the lane's own (dC) or one load per register (dPt).  Nothing is pre-scaled (bf16: one
// rounding less than the dQ kernel's folded form); a masked key and a row past the sequence select the exponent -inf.
// Each wave puts its 32 x 32 dS tile in LDS ([y][x], pitch 33); then lane x = 0 .. 31 walks y = 0 .. 31 in order.  col is
// monotone in i - j, so the columns a row meets on its walk over y never turn back: the lane adds to ONE open sum while the
// column stays, and stores the sum times `scale` (the tables sit before the scale, as Q K^T does; a plain store: the column is
// never met again) when the column changes or the walk over all tiles ends.  In the identity region of the buckets every
// sum has one term; in the logarithmic and clamped regions it is a run.  Columns a walk steps over get zeros on the way,
// and after the walk the wave stores zeros to every column outside [first, last] of each of its rows, so EVERY entry of a
// row is written exactly once.  The order of each sum is the order of y: identical calls give identical bits.  LDS: bf16 36,864 (tiles) + 16,896 (dS) = 53,760 bytes, fp32 17,408 + 16,896.
// ------------------------------------------------------------------------------------------------
template <typename T, bool DROP, bool PT, int KT, bool DBUF>
__device__ __forceinline__ void dtab_body(const DisParams& x, int64_t tile, int64_t b, int64_t hd, int64_t o_stride) {
  const AttnParams& p = x.a;
  const DisentTabs& dt = x.t;
  constexpr int KB = KT / 32, PITCH = D + Pad<T>::v, NBUF = DBUF ? 2 : 1;
  __shared__ __attribute__((aligned(16))) T as[NBUF][KT * PITCH];
  __shared__ __attribute__((aligned(16))) T bs[NBUF][KT * PITCH];
  __shared__ float ds_s[NW][32 * TP];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
  int64_t lq_, lk_, base, kbase, lse_base;
  seq_view(p, b, hd, lq_, lk_, base, kbase, lse_base);      // lq == lk: base == kbase
  if (tile * BQ >= lq_) return;                             // varlen: tile past this sequence (block-uniform): no rows to write
  const int64_t kvlen = clamp_kvlen(p, b, lk_);
  const int rows = (int)lq_;                                // < 2^30 (host check)
  const int x_wave0 = (int)(tile * BQ) + w * 32, xi = x_wave0 + r;
  const bool x_in = xi < rows;                              // the row exists in memory
  const bool x_on = PT ? xi < (int)kvlen : x_in;            // and takes part in the softmax
  const bool wave_live = x_wave0 < rows;                    // else: staging helper only
  const int ylim = PT ? rows : (int)kvlen;                  // the other index: queries below lq, keys below kv_len
  const int64_t xr = x_in ? xi : 0;
  const int64_t a_stride = PT ? p.q_stride : p.k_stride, b_stride = PT ? o_stride : p.v_stride;
  const T* ag = static_cast<const T*>(PT ? p.q : p.k) + base * a_stride + hd * D;
  const T* bg = static_cast<const T*>(PT ? p.dout : p.v) + base * b_stride + hd * D;
  RowFrag<T, D> fa, fb;
  fa.load(static_cast<const T*>(PT ? p.k : p.q) + (base + xr) * (PT ? p.k_stride : p.q_stride) + hd * D, x_in, h);
  fb.load(static_cast<const T*>(PT ? p.v : p.dout) + (base + xr) * (PT ? p.v_stride : o_stride) + hd * D, x_in, h);
  const float sl2 = p.scale * kLog2e;
  const float* lse_g = p.lse + lse_base;
  const float* dl_g = p.delta + lse_base;
  const float lse_x = (!PT && x_in) ? lse_g[xi] * kLog2e : INFINITY;   // dC: the lane's query
  const float dl_x = (!PT && x_in) ? dl_g[xi] : 0.f;
  constexpr uint32_t CX = PT ? kDropC2 : kDropC1, CY = PT ? kDropC1 : kDropC2;   // hash factors of the lane's and the register's index
  const uint32_t xu = drop_base(attn_seed(p), lse_base) + (uint32_t)(xi >> 1) * CX + (uint32_t)(2 * h) * CY;
  const int x_odd = xi & 1;
  const int64_t W = dt.w;
  const float* own_row = (PT ? dt.pt : dt.c) + disent_row(p, dt, hd, base + xr);      // the lane's row of its own table
  const float* other = (PT ? dt.c : dt.pt) + disent_row(p, dt, hd, base);             // + y * W: row y of the other table
  float* out_tab = (PT ? x.dpt : x.dc) + disent_row(p, dt, hd, base);                 // + row * W
  float* orow = out_tab + xr * W;
  int wfirst = -1, wcur = -1;                               // first and open column of the lane's walk (lanes 0 .. 31)
  float acc = 0.f;
  const int ntiles = (ylim + KT - 1) / KT;
  TileRegs<T, D, KT, NT> ar, br;
  ar.init(a_stride, tid);
  br.init(b_stride, tid);
  if (ntiles > 0) {
    ar.load(ag, a_stride, 0, lk_, tid);
    br.load(bg, b_stride, 0, lk_, tid);
    ar.store(as[0], tid);
    br.store(bs[0], tid);
  }
  __syncthreads();
  for (int t = 0; t < ntiles; ++t) {
    const int y0 = t * KT;
    const int cur = DBUF ? (t & 1) : 0;
    const bool more = t + 1 < ntiles;
    if (DBUF && more) {
      ar.load(ag, a_stride, y0 + KT, lk_, tid);
      br.load(bg, b_stride, y0 + KT, lk_, tid);
    }
    if (wave_live) {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const int yb = y0 + kb * 32;                        // first y of the block
        if (yb >= ylim) continue;                           // block-uniform: no y of the block takes part
        f32x16 s, dp;
#pragma unroll
        for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
        mma_rows<D>(as[cur], PITCH, kb * 32, fa, s, r, h);
        mma_rows<D>(bs[cur], PITCH, kb * 32, fb, dp, r, h);
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          const int yl = acc_row(i, h), y = yb + yl;        // even; registers i, i + 1 = y, y + 1
          const int yc0 = y < rows ? y : rows - 1, yc1 = y + 1 < rows ? y + 1 : rows - 1;   // rows that exist
          const bool ok0 = x_on && y < ylim, ok1 = x_on && y + 1 < ylim;
          float l0 = lse_x, l1 = lse_x, d0 = dl_x, d1 = dl_x;
          if constexpr (PT) {                               // the register's query
            l0 = lse_g[yc0] * kLog2e; l1 = lse_g[yc1] * kLog2e;
            d0 = dl_g[yc0]; d1 = dl_g[yc1];
          }
          // relative position query - key of the pair
          const float e0 = disent_term(dt, PT ? other + (int64_t)yc0 * W : own_row, PT ? own_row : other + (int64_t)yc0 * W, PT ? y - xi : xi - y);
          const float e1 = disent_term(dt, PT ? other + (int64_t)yc1 * W : own_row, PT ? own_row : other + (int64_t)yc1 * W, PT ? y + 1 - xi : xi - y - 1);
          const float a0 = ok0 ? fmaf(s[i], sl2, e0 * sl2 - l0) : -INFINITY;
          const float a1 = ok1 ? fmaf(s[i + 1], sl2, e1 * sl2 - l1) : -INFINITY;
          const float p0 = fast_exp2(a0), p1 = fast_exp2(a1);
          float m0 = 1.f, m1 = 1.f;
          if (DROP) {
            const uint32_t u = xu + ((uint32_t)(t * (KT / 2)) + (uint32_t)((kb * 32 + acc_row(i, 0)) >> 1)) * CY;
            if (PT) drop_pair_k(u, x_odd, p.drop_thresh, p.keep_scale, m0, m1);
            else drop_pair_q(u, x_odd, p.drop_thresh, p.keep_scale, m0, m1);
          }
          ds_s[w][yl * TP + r] = p0 * (dp[i] * m0 - d0);
          ds_s[w][(yl + 1) * TP + r] = p1 * (dp[i + 1] * m1 - d1);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (lane < 32 && x_on) {
          for (int yy = 0; yy < 32; ++yy) {
            const int y = yb + yy;
            if (y >= ylim) break;
            const int c = disent_col(dt, PT ? y - xi : xi - y);
            if (c != wcur) {
              if (wcur >= 0) {
                orow[wcur] = acc * p.scale;
                for (int u = (c < wcur ? c : wcur) + 1; u < (c < wcur ? wcur : c); ++u) orow[u] = 0.f;   // stepped over
              } else {
                wfirst = c;
              }
              wcur = c;
              acc = 0.f;
            }
            acc += ds_s[w][yy * TP + lane];
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
    if (DBUF) {
      if (more) {
        ar.store(as[cur ^ 1], tid);
        br.store(bs[cur ^ 1], tid);
      }
      __syncthreads();
    } else if (more) {
      __syncthreads();
      ar.load(ag, a_stride, y0 + KT, lk_, tid);
      br.load(bg, b_stride, y0 + KT, lk_, tid);
      ar.store(as[0], tid);
      br.store(bs[0], tid);
      __syncthreads();
    }
  }
  if (!wave_live) return;                                   // no barrier below
  if (lane < 32 && wcur >= 0) orow[wcur] = acc * p.scale;             // the sum still open
  // zeros outside [lo, hi] of each of the wave's rows (a row that met no pair: everywhere), 64 columns per step
  const int lo = wcur < 0 ? (int)W : (wfirst < wcur ? wfirst : wcur), hi = wcur < 0 ? -1 : (wfirst < wcur ? wcur : wfirst);
  for (int rr = 0; rr < 32; ++rr) {
    if (x_wave0 + rr >= rows) break;                        // wave-uniform
    const int lo_r = __shfl(lo, rr, 64), hi_r = __shfl(hi, rr, 64);
    float* zr = out_tab + (int64_t)(x_wave0 + rr) * W;
    for (int u = lane; u < (int)W; u += 64)
      if (u < lo_r || u > hi_r) zr[u] = 0.f;
  }
}

template <typename T, bool DROP>
__global__ __launch_bounds__(NT) void dc_kernel(DisParams x) {
  const Item it = decode(x.a);
  dtab_body<T, DROP, false, Cfg<T>::KT, Cfg<T>::DBUF>(x, it.tile, it.b, it.hd, x.a.h * D);
}
template <typename T, bool DROP>
__global__ __launch_bounds__(NT) void dpt_kernel(DisParams x) {
  const Item it = decode(x.a);
  dtab_body<T, DROP, true, Cfg<T>::KT, Cfg<T>::DBUF>(x, it.tile, it.b, it.hd, x.a.h * D);
}

// rows of the call that decide the grid and bound the column table: l padded, max_len packed
static inline int64_t call_rows(int64_t lq, const int32_t* cu_seqlens, int64_t max_len) { return cu_seqlens ? max_len : lq; }

// the checks of attn_host.hpp up to the empty-problem return, with this family's head dim, layout rules, table bounds and
// work-item bound; fills the launch parameters
static int setup(const char* who, DisParams& x, const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b,
                 int64_t h, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                 float dropout_p, uint64_t seed, const uint64_t* seed_dev, int64_t col_m, int64_t tab_w, const void* out_lo,
                 int dtype, const int32_t* cu_seqlens, int64_t max_len) {
  int rc = attn_check_shape(who, b >= 0 && h > 0 && lq >= 0 && lk >= 0, d == 64, d, "this entry point takes 64", dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(lq == lk, "%s: disentangled self-attention needs lq == lk (got %ld and %ld)", who, (long)lq, (long)lk);
  GMLM_REQUIRE(!cu_seqlens || (max_len > 0 && !kv_len), "%s: packed mode needs lq == lk = total rows, max_len > 0, kv_len NULL", who);
  const int64_t rows = call_rows(lq, cu_seqlens, max_len);
  GMLM_REQUIRE(col_m >= rows && col_m >= 1 && col_m <= GMLM_DISENT_MAX_LEN,
               "%s: col_m %ld must be in [%ld, %d] (the longest sequence of the call up to GMLM_DISENT_MAX_LEN)", who, (long)col_m,
               (long)(rows > 1 ? rows : 1), GMLM_DISENT_MAX_LEN);
  GMLM_REQUIRE(tab_w >= 1 && tab_w <= 2 * col_m - 1, "%s: tab_w %ld must be in [1, %ld] (no more columns than relative positions)", who,
               (long)tab_w, (long)(2 * col_m - 1));
  if ((rc = attn_check_rates(who, dropout_p, nullptr, scale)) != GMLM_OK) return rc;
  // each factor and each partial product is bounded before the next multiply: no int64 overflow on the way to the answer
  const int64_t tiles = cdiv(rows, (int64_t)BQ), lim = (int64_t)1 << 31;
  GMLM_REQUIRE(lq < ((int64_t)1 << 30) && b < lim && h < lim && b * h < lim && tiles * (b * h) < lim, "%s: too many work items", who);
  x = DisParams{};
  attn_fill(x.a, q, k, v, kv_len, b, h, lq, lk, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev);
  x.a.cu = cu_seqlens;
  x.t.m = (int)col_m;
  x.t.w = (int)tab_w;
  return GMLM_OK;
}

static int check_tabs(const char* who, DisParams& x, const float* c2p, const float* p2c, const int32_t* col) {
  GMLM_REQUIRE(c2p && aligned16(c2p) && p2c && aligned16(p2c), "%s: null or misaligned c2p / p2c table", who);
  GMLM_REQUIRE(col && aligned16(col), "%s: null or misaligned col", who);
  x.t.c = c2p; x.t.pt = p2c; x.t.col = col;
  return GMLM_OK;
}

}  // namespace disent
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::disent;

#define GMLM_DIS_LAUNCH_T(KERNEL, T, grid, st, prm)                          \
  do {                                                                       \
    if ((prm).a.drop_thresh) KERNEL<T, true><<<grid, NT, 0, st>>>(prm);      \
    else KERNEL<T, false><<<grid, NT, 0, st>>>(prm);                         \
  } while (0)
#define GMLM_DIS_LAUNCH(KERNEL, grid, st, prm)                               \
  do {                                                                       \
    if (dtype == GMLM_BF16) GMLM_DIS_LAUNCH_T(KERNEL, bf16_t, grid, st, prm); \
    else GMLM_DIS_LAUNCH_T(KERNEL, float, grid, st, prm);                    \
  } while (0)

extern "C" int gmlm_attention_disent_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                                         int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                         float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, const float* c2p,
                                         const float* p2c, const int32_t* col, int64_t col_m, int64_t tab_w, void* out, void* out_lo,
                                         float* lse, int dtype, const int32_t* cu_seqlens, int64_t max_len, gmlm_stream_t stream) {
  static const char* who = "attention_disent_fwd";
  DisParams x;
  int rc = setup(who, x, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev, col_m, tab_w,
                 out_lo, dtype, cu_seqlens, max_len);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, h * D, h * D, dtype)) != GMLM_OK) return rc;
  if ((rc = check_tabs(who, x, c2p, p2c, col)) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(cdiv(call_rows(lq, cu_seqlens, max_len), (int64_t)BQ) * b * h));
  GMLM_DIS_LAUNCH(fwd_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_disent_workspace_bytes(int64_t b, int64_t h, int64_t lq, int64_t max_len) {
  return attn_delta_bytes(max_len > 0 ? 1 : b, h, lq);
}

extern "C" int gmlm_attention_disent_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                         const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t h, int64_t lq,
                                         int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                         float dropout_p, uint64_t seed, const uint64_t* seed_dev, const float* c2p, const float* p2c,
                                         const int32_t* col, int64_t col_m, int64_t tab_w, void* dq, void* dk, void* dv, float* d_c2p,
                                         float* d_p2c, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                         const int32_t* cu_seqlens, int64_t max_len, void* workspace, size_t workspace_bytes,
                                         gmlm_stream_t stream) {
  static const char* who = "attention_disent_bwd";
  DisParams x;
  int rc = setup(who, x, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev, col_m, tab_w,
                 out_lo, dtype, cu_seqlens, max_len);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  AttnParams& p = x.a;
  const int64_t nb = cu_seqlens ? 1 : b;        // delta: packed tensors are one [total_rows, h, 64] block, delta is [h, total_rows]
  const int64_t tiles = cdiv(call_rows(lq, cu_seqlens, max_len), (int64_t)BQ);
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = check_tabs(who, x, c2p, p2c, col)) != GMLM_OK) return rc;
  GMLM_REQUIRE(d_c2p && aligned16(d_c2p) && d_p2c && aligned16(d_p2c), "%s: null or misaligned d_c2p / d_p2c", who);
  if ((rc = attn_check_bwd_operands(who, p, h * D, h * D, dtype, workspace_bytes, attn_delta_bytes(nb, h, lq))) != GMLM_OK) return rc;
  x.dc = d_c2p; x.dpt = d_p2c;
  hipStream_t st = as_stream(stream);
  const int64_t drows = nb * lq * h;
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, drows, dtype == GMLM_BF16 ? 8 : 16, st, lq, h);   // attn_delta_body: 64 / V lanes per row
  GMLM_LAUNCH_CHECK();
  const dim3 grid((unsigned)(tiles * b * h));
  GMLM_DIS_LAUNCH(dq_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  GMLM_DIS_LAUNCH(dkv_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  GMLM_DIS_LAUNCH(dc_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  GMLM_DIS_LAUNCH(dpt_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
