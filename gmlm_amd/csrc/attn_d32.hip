// Attention at head dim 32, forward + backward, gfx950 MFMA (gmlm_attention_d32_*; C ABI in include/gmlm_hip_d32.h).
// Shape: the self-attention of the 384-wide BERT-family sentence encoders (12 heads x 32: MiniLM-L6/L12, bge-small, e5-small,
// gte-small), padded [b, l, h*32] with an optional per-sequence key length, or packed [total_rows, h*32] with cu_seqlens.
// Every kernel IS a streaming kernel of attn_stream.hpp instantiated at D = 32 (S^T = K Q^T with the query on the lane, online
// softmax in the log2 domain, P fed straight from the accumulators into O^T += V^T P^T, bf16 folding of lse / delta / the key
// mask into one extra contraction step, exact fp32 delta through out_lo, the replayable 2 x 2 dropout hash of attn_common.hpp
// with the same slab and row offsets: the mask of a (sequence, head) does not depend on the head dim).  This file fixes:
//  * 1-D grids of (tile, (batch or sequence, head)) work items: no 65,535 bound on batch * heads (12 heads reach it at
//    5,462 sequences);
//  * bf16: 64-row K / V (forward, dQ) and Q / dO (dK/dV) tiles, double-buffered in LDS (<= 20 KiB per workgroup); fp32 (the
//    1e-4 parity path, v_mfma_f32_32x32x2_f32): 32-row tiles, one buffer.  No kernel spills;
//  * dK/dV without atomics: a workgroup owns its keys and walks all query tiles in order (deterministic);
//  * the workgroup height.  A sequence occupies whole work items, and every work item stages all keys of its sequence, so the
//    height follows the LONGEST sequence of the call, rows = max(lq, lk) when padded and max_len when packed:
//        rows <= 32  ->  32 rows, 1 wave   (a 20-token sequence fills most of its only wave)
//        rows <= 128 ->  64 rows, 2 waves  (the encoder's 16-128 token texts: at most two work items per (sequence, head))
//        else        -> 128 rows, 4 waves  (long sequences: four waves share each staged K / V tile)
//    One rule for the forward, dQ and dK/dV launches of a call; all three heights of every kernel are reachable.
// The argument checks and the AttnParams filling shared with the other attention entry points are in attn_host.hpp.
#include "attn_stream.hpp"
#include "attn_host.hpp"
#include "../../include/gmlm_hip_d32.h"

namespace gmlm {
namespace d32 {

constexpr int D = 32;

template <typename T> struct Cfg;
template <> struct Cfg<bf16_t> { static constexpr int KT = 64, QT = 64; static constexpr bool DBUF = true; };
template <> struct Cfg<float> { static constexpr int KT = 32, QT = 32; static constexpr bool DBUF = false; };

// forward: workgroup = NW * 32 query rows of one (sequence, head), loop over key tiles
template <typename T, int NW, bool DROP>
__global__ __launch_bounds__(NW * 64) void fwd_kernel(AttnParams p) {
  const Item it = decode(p);
  attn_fwd_body<T, D, NW, DROP, Cfg<T>::KT, Cfg<T>::DBUF>(p, it.tile, it.b, it.hd, p.h * D);
}

// backward: delta = rowsum(dO * O) over rows of [b * lq, h, 32] (O = out + out_lo when the forward stored the residual)
template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                    int64_t rows /* b * lq * h */, int64_t lq, int64_t hn, float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);     // 8 lanes per row (4 of them loading in bf16)
}

// backward: dQ.  workgroup = NW * 32 queries of one (sequence, head), loop over key tiles
template <typename T, int NW, bool DROP>
__global__ __launch_bounds__(NW * 64) void dq_kernel(AttnParams p) {
  const Item it = decode(p);
  attn_dq_body<T, D, NW, DROP, Cfg<T>::KT, Cfg<T>::DBUF>(p, it.tile, it.b, it.hd, p.h * D);
}

// backward: dK, dV.  workgroup = NW * 32 keys of one (sequence, head), loop over query tiles in order
template <typename T, int NW, bool DROP>
__global__ __launch_bounds__(NW * 64) void dkv_kernel(AttnParams p) {
  const Item it = decode(p);
  attn_dkv_body<T, D, NW, DROP, Cfg<T>::QT, Cfg<T>::DBUF>(p, it.tile, it.b, it.hd, p.h * D);
}

// waves per workgroup from the longest sequence of the call (the rule of the header)
static inline int pick_waves(int64_t rows) { return rows <= 32 ? 1 : (rows <= 128 ? 2 : 4); }

// the checks of attn_host.hpp up to the empty-problem return, with this family's head dim, packed mode and work-item bound;
// fills the launch parameters and the workgroup height
static int setup(const char* who, AttnParams& p, int& nw, const void* q, const void* k, const void* v, const int32_t* kv_len,
                 int64_t b, int64_t h, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                 float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, const void* out_lo, int dtype,
                 const int32_t* cu_seqlens, int64_t max_len) {
  int rc = attn_check_shape(who, b >= 0 && h > 0 && lq >= 0 && lk >= 0, d == 32, d, "this entry point takes 32", dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(!cu_seqlens || (lq == lk && max_len > 0 && !kv_len), "%s: packed mode needs lq == lk = total rows, max_len > 0, kv_len NULL", who);
  if ((rc = attn_check_rates(who, dropout_p, nullptr, scale)) != GMLM_OK) return rc;
  const int64_t rows = cu_seqlens ? max_len : (lq > lk ? lq : lk);
  nw = pick_waves(rows);
  // each factor and each partial product is bounded before the next multiply: no int64 overflow on the way to the answer
  const int64_t tiles = cdiv(rows, (int64_t)nw * 32), lim = (int64_t)1 << 31;
  GMLM_REQUIRE(b < lim && h < lim && tiles < lim && b * h < lim && tiles * (b * h) < lim, "%s: too many work items", who);
  p = AttnParams{};
  attn_fill(p, q, k, v, kv_len, b, h, lq, lk, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev);
  p.cu = cu_seqlens;
  return GMLM_OK;
}

}  // namespace d32
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::d32;

#define GMLM_D32_LAUNCH_T(KERNEL, T, NWV, grid, st, prm)                                                    \
  do {                                                                                                      \
    if ((prm).drop_thresh) KERNEL<T, NWV, true><<<grid, NWV * 64, 0, st>>>(prm);                            \
    else KERNEL<T, NWV, false><<<grid, NWV * 64, 0, st>>>(prm);                                             \
  } while (0)
#define GMLM_D32_LAUNCH_W(KERNEL, NWV, grid, st, prm)                                                       \
  do {                                                                                                      \
    if (dtype == GMLM_BF16) GMLM_D32_LAUNCH_T(KERNEL, bf16_t, NWV, grid, st, prm);                          \
    else GMLM_D32_LAUNCH_T(KERNEL, float, NWV, grid, st, prm);                                              \
  } while (0)
// rows_: the longest query (forward, dQ) or key (dK/dV) sequence; the height nw is the call's
#define GMLM_D32_LAUNCH(KERNEL, nw, rows_, pairs, st, prm)                                                  \
  do {                                                                                                      \
    const dim3 grid_((unsigned)(cdiv((int64_t)(rows_), (int64_t)(nw) * 32) * (pairs)));                     \
    if ((nw) == 1) GMLM_D32_LAUNCH_W(KERNEL, 1, grid_, st, prm);                                            \
    else if ((nw) == 2) GMLM_D32_LAUNCH_W(KERNEL, 2, grid_, st, prm);                                       \
    else GMLM_D32_LAUNCH_W(KERNEL, 4, grid_, st, prm);                                                      \
  } while (0)

extern "C" int gmlm_attention_d32_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                                      int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                      float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* out, void* out_lo,
                                      float* lse, int dtype, const int32_t* cu_seqlens, int64_t max_len, gmlm_stream_t stream) {
  static const char* who = "attention_d32_fwd";
  AttnParams p;
  int nw = 0;
  int rc = setup(who, p, nw, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev, out_lo,
                 dtype, cu_seqlens, max_len);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  p.o_w = out; p.o_lo_w = out_lo; p.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, p, h * D, h * D, dtype)) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  GMLM_D32_LAUNCH(fwd_kernel, nw, cu_seqlens ? max_len : lq, b * h, st, p);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_d32_bwd_workspace_bytes(int64_t b, int64_t h, int64_t lq) {
  return attn_delta_bytes(b, h, lq);
}

extern "C" int gmlm_attention_d32_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                                      const float* lse, const int32_t* kv_len, int64_t b, int64_t h, int64_t lq, int64_t lk,
                                      int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                                      uint64_t seed, const uint64_t* seed_dev, void* dq, void* dk, void* dv, int64_t dq_stride,
                                      int64_t dk_stride, int64_t dv_stride, int dtype, const int32_t* cu_seqlens, int64_t max_len,
                                      void* workspace, size_t workspace_bytes, const void* out_lo, gmlm_stream_t stream) {
  static const char* who = "attention_d32_bwd";
  AttnParams p;
  int nw = 0;
  int rc = setup(who, p, nw, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev, out_lo,
                 dtype, cu_seqlens, max_len);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || (lq == 0 && lk == 0)) return GMLM_OK;
  GMLM_REQUIRE(lq > 0 && lk > 0, "%s: empty query or key set with a non-empty counterpart is not supported", who);
  const int64_t nb = cu_seqlens ? 1 : b;        // delta: packed tensors are one [total_rows, h, 32] block, delta is [h, total_rows]
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, p, h * D, h * D, dtype, workspace_bytes, attn_delta_bytes(nb, h, lq))) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t rows = nb * lq * h;
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, rows, 8, st, lq, h);
  GMLM_LAUNCH_CHECK();
  GMLM_D32_LAUNCH(dq_kernel, nw, cu_seqlens ? max_len : lq, b * h, st, p);
  GMLM_LAUNCH_CHECK();
  GMLM_D32_LAUNCH(dkv_kernel, nw, cu_seqlens ? max_len : lk, b * h, st, p);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
