// K5/K7 — multi-head attention core with streaming softmax, forward + backward, gfx950 MFMA.
// Reference: K5 = BertSelfAttention's attention call softmax(QK^T*d^-1/2 + padding mask)V
// (hf:modeling_bert.py:188-201, eager form 111-136); K7 = CrossAttention.forward's dense
// [1,8,N,N] softmax over all nodes (main.py:159-163).
//
// Design (wave64, one process per GPU, no score matrix in HBM):
//  * forward: a workgroup = 4 waves = 128 query rows of one (batch, head); each wave owns 32 rows.
//    K/V tiles of 64 keys are staged row-major in LDS.  Scores are computed TRANSPOSED,
//    S^T = K Q^T, with v_mfma_f32_32x32x16_bf16 (bf16) or v_mfma_f32_32x32x2_f32 (exact f32):
//    the query column then sits on the lane and the 32 keys in the accumulator registers, so the
//    row max / row sum are register reductions plus one half-wave exchange, the running rescale is
//    lane-local, and the probability tile feeds the next MFMA (O^T += V^T P^T) straight from the
//    accumulator registers as its B operand (no LDS round trip).  V^T fragments come from the same
//    row-major LDS image through ds_read_b64_tr_b16 (hardware transpose read).
//  * backward = three launches, no atomics (deterministic): delta = rowsum(dO*O); a dQ kernel
//    (workgroup = 128 queries, loops over key tiles) and a dK/dV kernel (workgroup = 128 keys,
//    loops over query tiles).  P is recomputed from Q, K and the forward's log-sum-exp.
//  * padding: keys >= kv_len[b] get probability exactly 0 (the reference adds finfo.min and
//    softmaxes: the same zeros in fp32); whole tiles past kv_len are skipped.
// The device code of these kernels is in attn_stream.hpp (one body per kernel, shared with attn_d128.hip) and the host contract
// of every attention entry point in attn_host.hpp; this file holds the d = 64 / 96 kernel entry points, what
// gmlm_attention_fwd / gmlm_attention_bwd check beyond that contract, and their dispatch.
#include "attn_stream.hpp"
#include "attn_host.hpp"
#include "colreduce.hpp"

namespace gmlm {

// entry points: decode the two-dimensional grid (x = tile, y = batch * heads + head), pick the tile sizes
template <typename T, int D, int NW, bool DROP>
__global__ __launch_bounds__(NW * 64) void attn_fwd_kernel(AttnParams p) {
  attn_fwd_body<T, D, NW, DROP, 64, sizeof(T) == 2>(p, blockIdx.x, blockIdx.y / p.h, blockIdx.y % p.h, p.h * D);
}

template <typename T>
__global__ __launch_bounds__(256) void attn_delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                          int64_t rows /* b*lq*h */, int d, int64_t lq, int64_t hn,
                                                          float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, d, lq, hn, delta);
}

template <typename T, int D, int NW, bool DROP>
__global__ __launch_bounds__(NW * 64) void attn_bwd_dq_kernel(AttnParams p) {
  constexpr bool DBUF = sizeof(T) == 2;
  constexpr int KT = DBUF ? (NW == 8 ? 128 : 64) : 32;   // 8-wave blocks own the CU (202 VGPRs): 128-key tiles halve their barriers (-4 %)
  attn_dq_body<T, D, NW, DROP, KT, DBUF>(p, blockIdx.x, blockIdx.y / p.h, blockIdx.y % p.h, p.h * D);
}

// QT = query rows staged per barrier (attn_dkv_body)
template <typename T, int D, int NW, bool DROP, int QT = 32>
__global__ __launch_bounds__(NW * 64) void attn_bwd_dkv_kernel(AttnParams p) {
  attn_dkv_body<T, D, NW, DROP, QT, sizeof(T) == 2 && QT <= 64>(p, blockIdx.x, blockIdx.y / p.h, blockIdx.y % p.h, p.h * D);
}

// the host checks of gmlm_attention_fwd / _bwd up to the empty-problem return, in the order of attn_host.hpp
static int attn_check(const char* who, int64_t b, int64_t h, int64_t lq, int64_t lk, int64_t d, int dtype, const void* out_lo,
                      const int32_t* kv_len, const int32_t* cu_seqlens, int64_t max_len, const int32_t* seq_groups, int64_t num_groups,
                      float dropout_p, float scale) {
  int rc = attn_check_shape(who, b >= 0 && h > 0 && lq >= 0 && lk >= 0, d == 64 || d == 96, d, "64 or 96", dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(!cu_seqlens || (lq == lk && max_len > 0 && !kv_len), "%s: packed mode needs lq == lk = total rows, max_len > 0, kv_len NULL", who);
  GMLM_REQUIRE(!seq_groups || (cu_seqlens && num_groups > 0 && num_groups <= b), "%s: seq_groups needs packed mode and 0 < num_groups <= b", who);
  if ((rc = attn_check_rates(who, dropout_p, nullptr, scale)) != GMLM_OK) return rc;
  GMLM_REQUIRE(b * h <= 65535, "%s: batch*heads %ld > 65535", who, (long)(b * h));   // grid.y of the two-dimensional launches
  return GMLM_OK;
}

}  // namespace gmlm

using namespace gmlm;

#define GMLM_ATTN_DISPATCH2(KERNEL, NWV, DR, grid, st, prm)                                  \
  do {                                                                                       \
    if (dtype == GMLM_BF16) {                                                                \
      if (d == 64) KERNEL<bf16_t, 64, NWV, DR><<<grid, NWV * 64, 0, st>>>(prm);              \
      else KERNEL<bf16_t, 96, NWV, DR><<<grid, NWV * 64, 0, st>>>(prm);                      \
    } else {                                                                                 \
      if (d == 64) KERNEL<float, 64, NWV, DR><<<grid, NWV * 64, 0, st>>>(prm);               \
      else KERNEL<float, 96, NWV, DR><<<grid, NWV * 64, 0, st>>>(prm);                       \
    }                                                                                        \
  } while (0)
#define GMLM_ATTN_DISPATCH(KERNEL, NWV, grid, st, prm)                                       \
  do {                                                                                       \
    if ((prm).drop_thresh) GMLM_ATTN_DISPATCH2(KERNEL, NWV, true, grid, st, prm);            \
    else GMLM_ATTN_DISPATCH2(KERNEL, NWV, false, grid, st, prm);                             \
  } while (0)

// Rows per workgroup.  Every workgroup streams ALL keys of its (batch, head) through LDS, so the K/V bytes read
// per flop fall with the number of query rows that share a tile: 8 waves = 256 rows for long sequences when there
// are enough workgroups to fill the chip twice (measured: forward neutral, backward +4 % at N = 20k); 4 waves
// (128 rows) by default; 2 waves (64 rows) when the grid would under-fill the 256 CUs (+80 % at N = 5k).
namespace gmlm {
int attn_fwd_pipe_launch(const AttnParams& p, int d, int nw, int64_t rows_q, int64_t bh, hipStream_t st);
int attn_short_fwd_launch(const AttnParams& p, int64_t rows, int64_t items, hipStream_t st);
int attn_short_bwd_launch(const AttnParams& p, int64_t rows, int64_t items, float* dbias, hipStream_t st);
int attn_bwd_pipe_launch(const AttnParams& p, int d, int nw, int64_t rows_q, int64_t rows_k, int64_t bh, hipStream_t st);
}

static inline int pick_waves(int64_t rows, int64_t bh) {
  if (rows >= 2048 && cdiv(rows, 256) * bh >= 512) return 8;
  return cdiv(rows, 128) * bh >= 1024 ? 4 : 2;
}

#ifdef GMLM_ATTN_STAMP
static void* g_stamp_buffer = nullptr;     // diagnostic build only: per-wave cycle stamps of the pipelined forward
extern "C" void gmlm_debug_set_stamp_buffer(void* p) { g_stamp_buffer = p; }
#endif

extern "C" int gmlm_attention_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                                  int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                  float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* out, void* out_lo, float* lse,
                                  int dtype, const int32_t* cu_seqlens, int64_t max_len, const int32_t* seq_groups, int64_t num_groups,
                                  gmlm_stream_t stream) {
  static const char* who = "attention_fwd";
  int rc = attn_check(who, b, h, lq, lk, d, dtype, out_lo, kv_len, cu_seqlens, max_len, seq_groups, num_groups, dropout_p, scale);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  AttnParams p{};
  attn_fill(p, q, k, v, kv_len, b, h, lq, lk, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev);
  p.o_w = out; p.o_lo_w = out_lo; p.lse_w = lse; p.cu = cu_seqlens; p.groups = seq_groups;
  if ((rc = attn_check_fwd_operands(who, p, h * d, h * d, dtype)) != GMLM_OK) return rc;
  const int64_t rows_q = cu_seqlens ? max_len : lq;
  hipStream_t st = as_stream(stream);
#ifdef GMLM_ATTN_STAMP
  p.delta = static_cast<float*>(g_stamp_buffer);
#endif
  if (dtype == GMLM_BF16 && d == 64 && rows_q <= 128 && (cu_seqlens ? max_len : lk) <= 128 && b * h >= 512) {
    // short sequences, enough of them to fill the chip: Q / K / V resident in LDS, one barrier (attn_short.hip); with
    // `seq_groups` a workgroup takes a run of sequences (<= 128 rows) instead of one
    const int64_t rk_ = cu_seqlens ? max_len : lk, rmax = rows_q > rk_ ? rows_q : rk_;
    return attn_short_fwd_launch(p, seq_groups ? 128 : rmax, seq_groups ? num_groups : b, st);
  }
  if (dtype == GMLM_BF16 && (d == 96 || rows_q > 128)) {
    // software-pipelined LDS-DMA kernel (attn_fwd_pipe.hip): CrossAttention geometry (d = 96: +40-45 % at N = 5k-20k
    // against attn_fwd_kernel) and BERT geometry beyond 128 tokens (d = 64: +8 % at L = 512, +15 % at L = 2048).
    // Sequences of <= 128 tokens (what the reference's tokeniser produces, main.py:340) go to attn_fwd_short_kernel above
    // when there are enough of them; this kernel measures the same there (171 vs 175 us on the bench's packed mix).
    const int nw = d == 96 ? (pick_waves(rows_q, b * h) == 8 ? 8 : 4) : 4;
    rc = attn_fwd_pipe_launch(p, (int)d, nw, rows_q, b * h, st);
    if (rc != GMLM_OK) return rc;
    GMLM_LAUNCH_CHECK();
    return GMLM_OK;
  }
  if (pick_waves(rows_q, b * h) == 8) {
    dim3 grid((unsigned)cdiv(rows_q, 256), (unsigned)(b * h));
    GMLM_ATTN_DISPATCH(attn_fwd_kernel, 8, grid, st, p);
  } else if (pick_waves(rows_q, b * h) == 4) {
    dim3 grid((unsigned)cdiv(rows_q, 128), (unsigned)(b * h));
    GMLM_ATTN_DISPATCH(attn_fwd_kernel, 4, grid, st, p);
  } else {
    dim3 grid((unsigned)cdiv(rows_q, 64), (unsigned)(b * h));
    GMLM_ATTN_DISPATCH(attn_fwd_kernel, 2, grid, st, p);
  }
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_bwd_workspace_bytes(int64_t b, int64_t h, int64_t lq, int64_t lk, int64_t d) {
  (void)lk; (void)d;
  return attn_delta_bytes(b, h, lq);
}

extern "C" int gmlm_attention_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                                  const float* lse, const int32_t* kv_len, int64_t b, int64_t h, int64_t lq, int64_t lk,
                                  int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                  float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* dq, void* dk, void* dv, int64_t dq_stride,
                                  int64_t dk_stride, int64_t dv_stride, int dtype, const int32_t* cu_seqlens, int64_t max_len,
                                  void* workspace, size_t workspace_bytes, float* dbias_partial, float* dbias,
                                  const void* out_lo, const int32_t* seq_groups, int64_t num_groups, gmlm_stream_t stream) {
  static const char* who = "attention_bwd";
  int rc = attn_check(who, b, h, lq, lk, d, dtype, out_lo, kv_len, cu_seqlens, max_len, seq_groups, num_groups, dropout_p, scale);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE((dbias_partial == nullptr) == (dbias == nullptr), "%s: dbias_partial and dbias come together", who);
  if (b == 0 || (lq == 0 && lk == 0)) return GMLM_OK;
  GMLM_REQUIRE(lq > 0 && lk > 0, "%s: empty query or key set with a non-empty counterpart is not supported", who);
  const int64_t nb = cu_seqlens ? 1 : b;        // delta: packed tensors are one [total_rows, h, d] block
  AttnParams p{};
  attn_fill(p, q, k, v, kv_len, b, h, lq, lk, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev);
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  p.cu = cu_seqlens; p.groups = seq_groups; p.dbias_part = dbias_partial;
  if ((rc = attn_check_bwd_operands(who, p, h * d, h * d, dtype, workspace_bytes, attn_delta_bytes(nb, h, lq))) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t rows_q = cu_seqlens ? max_len : lq, rows_k = cu_seqlens ? max_len : lk;
  if (dtype == GMLM_BF16 && d == 64 && rows_q <= 128 && rows_k <= 128 && b * h >= 512 && !out_lo) {
    // short sequences, enough of them to fill the chip: one fused launch (delta + dQ + dK/dV), no workspace, O is not read.
    // The kernel forms delta = sum_k P dP over ITS OWN keys, which equals rowsum(dO * O) only when `lse` is the log-sum-exp of
    // exactly these keys.  A caller that hands in out_lo asks for delta = rowsum(dO * (out + out_lo)) - a ring block's `lse`
    // and `out` are those of all keys (gmlm_hip.h) - and gets the streaming kernels below at any shape.
    const int64_t rmax = rows_q > rows_k ? rows_q : rows_k;
    return attn_short_bwd_launch(p, seq_groups ? 128 : rmax, seq_groups ? num_groups : b, dbias, st);
  }
  GMLM_REQUIRE(!dbias, "%s: the fused bias-gradient sums exist only on the short-sequence path (bf16, d = 64, <= 128 rows, b*h >= 512, no out_lo)", who);
  const int64_t rows = nb * lq * h;
  const int cpr = (int)d / (dtype == GMLM_BF16 ? 8 : 4);
  GMLM_ATTN_DELTA_LAUNCH(attn_delta_kernel, p, rows, cpr <= 8 ? 8 : (cpr <= 16 ? 16 : 32), st, (int)d, lq, h);
  GMLM_LAUNCH_CHECK();
  if (dtype == GMLM_BF16 && d == 96) {
    // CrossAttention geometry: LDS-DMA staged kernels (attn_bwd_pipe.hip): no staging registers (the register-staged 2- / 4-wave
    // variants spill 44-88 bytes per lane at d = 96), 4-wave workgroups unless the grid fills the chip twice with 8.
    // bf16 below this point is therefore d = 64
    return attn_bwd_pipe_launch(p, (int)d, pick_waves(rows_q, b * h) == 8 ? 8 : 4, rows_q, rows_k, b * h, st);
  }
  if (pick_waves(rows_q, b * h) == 8) {
    dim3 gq((unsigned)cdiv(rows_q, 256), (unsigned)(b * h));
    GMLM_ATTN_DISPATCH(attn_bwd_dq_kernel, 8, gq, st, p);
  } else if (pick_waves(rows_q, b * h) == 4) {
    dim3 gq((unsigned)cdiv(rows_q, 128), (unsigned)(b * h));
    GMLM_ATTN_DISPATCH(attn_bwd_dq_kernel, 4, gq, st, p);
  } else {
    dim3 gq((unsigned)cdiv(rows_q, 64), (unsigned)(b * h));
    GMLM_ATTN_DISPATCH(attn_bwd_dq_kernel, 2, gq, st, p);
  }
  GMLM_LAUNCH_CHECK();
  if (pick_waves(rows_k, b * h) == 8 && !(dtype == GMLM_F32 && d == 96)) {   // f32 d=96 at 512 threads would spill
    dim3 gk((unsigned)cdiv(rows_k, 256), (unsigned)(b * h));
    if (dtype == GMLM_BF16) {   // long sequences: 64 query rows per barrier (two 32-row blocks), double-buffered
      { if (p.drop_thresh) attn_bwd_dkv_kernel<bf16_t, 64, 8, true, 64><<<gk, 512, 0, st>>>(p); else attn_bwd_dkv_kernel<bf16_t, 64, 8, false, 64><<<gk, 512, 0, st>>>(p); }
    } else {
      GMLM_ATTN_DISPATCH(attn_bwd_dkv_kernel, 8, gk, st, p);
    }
  } else if (pick_waves(rows_k, b * h) >= 4) {
    dim3 gk((unsigned)cdiv(rows_k, 128), (unsigned)(b * h));
    if (dtype == GMLM_BF16 && rows_q <= 128) {
      // short sequences (the reference tokenises to <= 128 tokens): all query rows staged behind one barrier
      { if (p.drop_thresh) attn_bwd_dkv_kernel<bf16_t, 64, 4, true, 128><<<gk, 256, 0, st>>>(p); else attn_bwd_dkv_kernel<bf16_t, 64, 4, false, 128><<<gk, 256, 0, st>>>(p); }
    } else if (dtype == GMLM_BF16) {
      // 64 query rows per barrier (two 32-row blocks), double-buffered: -8 % at L = 512 against 32-row tiles
      { if (p.drop_thresh) attn_bwd_dkv_kernel<bf16_t, 64, 4, true, 64><<<gk, 256, 0, st>>>(p); else attn_bwd_dkv_kernel<bf16_t, 64, 4, false, 64><<<gk, 256, 0, st>>>(p); }
    } else {
      GMLM_ATTN_DISPATCH(attn_bwd_dkv_kernel, 4, gk, st, p);
    }
  } else {
    dim3 gk((unsigned)cdiv(rows_k, 64), (unsigned)(b * h));
    if (dtype == GMLM_BF16 && rows_q > 128) {      // 64-row tiles here too: -11 % at N = 5,201
      { if (p.drop_thresh) attn_bwd_dkv_kernel<bf16_t, 64, 2, true, 64><<<gk, 128, 0, st>>>(p); else attn_bwd_dkv_kernel<bf16_t, 64, 2, false, 64><<<gk, 128, 0, st>>>(p); }
    } else {
      GMLM_ATTN_DISPATCH(attn_bwd_dkv_kernel, 2, gk, st, p);
    }
  }
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
