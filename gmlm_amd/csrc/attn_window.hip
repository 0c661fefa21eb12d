// Band-limited (sliding-window) self-attention at head dim 64, forward + backward, gfx950 MFMA (gmlm_attention_window_*; C ABI
// in include/gmlm_hip_modernbert.h): the "sliding_attention" layers of a ModernBERT encoder, where query i sees the keys j of
// its own sequence with |i - j| <= window that lie below the sequence's key count.  Padded layout [b, l, h*64] with row strides
// (a fused [q | k | v] buffer is read, and its gradient written, without copies) or packed [total_rows, h*64] with cu_seqlens.
// Every kernel IS a streaming body of attn_stream.hpp instantiated with its WINDOW template flag (default false: the existing
// kernels' instantiations are unchanged) at D = 64, 4 waves = 128 rows per workgroup; bf16: 64-row K / V tiles and 32-row
// Q / dO tiles, double-buffered in LDS; fp32: 32-row tiles, one buffer.  What the flag changes:
//  * the key loop (forward, dQ) covers [q_tile0 - w, q_tile_end + w] and the query loop (dK/dV) [k_tile0 - w, k_tile_end + w],
//    cut to the sequence: block-uniform bounds, so the work per workgroup is O(128 + 2 w) rows instead of O(l);
//  * a wave skips the arithmetic, never a barrier, of tiles outside the band of its 32 rows; tiles wholly inside it and below
//    the key count keep the compare-free path; only tiles that the band edge crosses compare |i - j| <= w per element;
//  * a row can meet computed tiles in which it sees no key: the forward guards both exponentials of the online softmax against
//    -inf - -inf; the backward selects P = 0 at band-edge blocks (a select, not a product) and treats lse = -inf as
//    "probability 0 everywhere", so a query with no visible key has output 0, lse = -inf, dQ = 0 and adds nothing to dK / dV.
// 1-D grids of (tile, (batch or sequence, head)) work items: no 65,535 bound on batch * heads.  dK/dV without atomics: a
// workgroup owns its keys and walks its query tiles in order (deterministic).  There is no dropout and no LDS-resident
// short-sequence form.  The argument checks and the AttnParams filling shared with the other attention entry points are in
// attn_host.hpp.
#include "attn_stream.hpp"
#include "attn_host.hpp"
#include "../../include/gmlm_hip_modernbert.h"

namespace gmlm {
namespace mbert {

constexpr int D = 64, NW = 4, NT = NW * 64, BQ = NW * 32;

struct WinParams {
  AttnParams a;
  int64_t window;
};

// Cfg<T> (tile sizes) is attn_stream.hpp's, decode() (1-D grid -> tile, sequence, head) attn_common.hpp's

// forward: workgroup = 128 query rows of one (sequence, head), key tiles of the band
template <typename T>
__global__ __launch_bounds__(NT) void window_fwd_kernel(WinParams x) {
  const Item it = decode(x.a);
  attn_fwd_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, false, false, true>(x.a, it.tile, it.b, it.hd, x.a.h * D, 0, x.window);
}

// backward: delta = rowsum(dO * O) over rows of [b * l, h, 64] (O = out + out_lo when the forward stored the residual)
template <typename T>
__global__ __launch_bounds__(256) void window_delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo,
                                                           const T* __restrict__ dout, int64_t rows /* b * l * h */, int64_t lq,
                                                           int64_t hn, float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);
}

// backward: dQ.  workgroup = 128 queries of one (sequence, head), key tiles of the band
template <typename T>
__global__ __launch_bounds__(NT) void window_dq_kernel(WinParams x) {
  const Item it = decode(x.a);
  attn_dq_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, false, false, true>(x.a, it.tile, it.b, it.hd, x.a.h * D, 0, x.window);
}

// backward: dK, dV.  workgroup = 128 keys of one (sequence, head), query tiles of the band in order
template <typename T>
__global__ __launch_bounds__(NT) void window_dkv_kernel(WinParams x) {
  const Item it = decode(x.a);
  attn_dkv_body<T, D, NW, false, Cfg<T>::QT, Cfg<T>::DBUF, true>(x.a, it.tile, it.b, it.hd, x.a.h * D, x.window);
}

// the checks of attn_host.hpp up to the empty-problem return, with this family's head dim, layout rules and work-item bound;
// fills the launch parameters
static int setup(const char* who, WinParams& x, const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b,
                 int64_t h, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                 float dropout_p, int64_t window, const void* out_lo, int dtype, const int32_t* cu_seqlens, int64_t max_len) {
  int rc = attn_check_shape(who, b >= 0 && h > 0 && lq >= 0 && lk >= 0, d == 64, d, "this entry point takes 64", dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(lq == lk, "%s: band-limited self-attention needs lq == lk (got %ld and %ld)", who, (long)lq, (long)lk);
  GMLM_REQUIRE(!cu_seqlens || (max_len > 0 && !kv_len), "%s: packed mode needs lq == lk = total rows, max_len > 0, kv_len NULL", who);
  GMLM_REQUIRE(window >= 0 && window < ((int64_t)1 << 30), "%s: window %ld must be in [0, 2^30)", who, (long)window);
  GMLM_REQUIRE(dropout_p == 0.f, "%s: attention-probability dropout is not implemented for the band-limited kernels (dropout_p must be 0)", who);
  GMLM_REQUIRE(scale > 0.f, "%s: scale must be positive", who);
  const int64_t rows = cu_seqlens ? max_len : lq;
  // each factor and each partial product is bounded before the next multiply: no int64 overflow on the way to the answer
  const int64_t tiles = cdiv(rows, (int64_t)BQ), lim = (int64_t)1 << 31;
  GMLM_REQUIRE(lq < ((int64_t)1 << 30) && rows < ((int64_t)1 << 30) && b < lim && h < lim && b * h < lim && tiles * (b * h) < lim,
               "%s: too many work items", who);
  x = WinParams{};
  attn_fill(x.a, q, k, v, kv_len, b, h, lq, lk, q_stride, k_stride, v_stride, scale, 0.f, 0, nullptr);
  x.a.cu = cu_seqlens;
  x.window = window;
  return GMLM_OK;
}

}  // namespace mbert
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::mbert;

#define GMLM_WINDOW_LAUNCH(KERNEL, grid, st, prm)                         \
  do {                                                                    \
    if (dtype == GMLM_BF16) KERNEL<bf16_t><<<grid, NT, 0, st>>>(prm);     \
    else KERNEL<float><<<grid, NT, 0, st>>>(prm);                         \
  } while (0)

extern "C" int gmlm_attention_window_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                                         int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                         float scale, float dropout_p, int64_t window, void* out, void* out_lo, float* lse,
                                         int dtype, const int32_t* cu_seqlens, int64_t max_len, gmlm_stream_t stream) {
  static const char* who = "attention_window_fwd";
  WinParams x;
  int rc = setup(who, x, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, window, out_lo, dtype,
                 cu_seqlens, max_len);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, h * D, h * D, dtype)) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(cdiv(cu_seqlens ? max_len : lq, (int64_t)BQ) * b * h));
  GMLM_WINDOW_LAUNCH(window_fwd_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_window_workspace_bytes(int64_t b, int64_t h, int64_t lq) { return attn_delta_bytes(b, h, lq); }

extern "C" int gmlm_attention_window_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                         const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t h,
                                         int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                         float scale, float dropout_p, int64_t window, void* dq, void* dk, void* dv,
                                         int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                         const int32_t* cu_seqlens, int64_t max_len, void* workspace, size_t workspace_bytes,
                                         gmlm_stream_t stream) {
  static const char* who = "attention_window_bwd";
  WinParams x;
  int rc = setup(who, x, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, window, out_lo, dtype,
                 cu_seqlens, max_len);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  AttnParams& p = x.a;
  const int64_t nb = cu_seqlens ? 1 : b;        // delta: packed tensors are one [total_rows, h, 64] block, delta is [h, total_rows]
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, p, h * D, h * D, dtype, workspace_bytes, attn_delta_bytes(nb, h, lq))) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t rows = nb * lq * h;
  GMLM_ATTN_DELTA_LAUNCH(window_delta_kernel, p, rows, dtype == GMLM_BF16 ? 8 : 16, st, lq, h);   // attn_delta_body: 64 / V lanes per row
  GMLM_LAUNCH_CHECK();
  const dim3 grid((unsigned)(cdiv(cu_seqlens ? max_len : lq, (int64_t)BQ) * b * h));
  GMLM_WINDOW_LAUNCH(window_dq_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  GMLM_WINDOW_LAUNCH(window_dkv_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
