// Band-limited (sliding-window) self-attention with grouped KV heads at head dim 256, causal or bidirectional, padded or packed,
// forward + backward, gfx950 MFMA (gmlm_attention_gqa_d256_band_*; C ABI in include/gmlm_hip_gqa_band.h), all in namespace
// gmlm::gqab: the "sliding_attention" layers of a Gemma3 text encoder whose sequences reach past the window.  Query i sees key j
// of its own sequence iff j < kv_len and 0 <= i - j < window (causal) or |i - j| < window: HF's exclusive window.
// Every kernel IS a body of attn_wide.hpp at GROUPED = true, D = 256 with its BAND flag (what the flag changes is said there);
// the launch parameters are grouped::Params plus the window, in a struct of this file, so the gqaw:: kernels of
// attn_gqa_wide.hip keep their arguments.  The argument checks are grouped::setup with that family's words and the window check
// added after the scale check.  Here: the kernels under their names, the dynamic-LDS attributes (81.3 KiB in fp32), the launches
// and the exports.  No atomics and no scratch: a repeated call gives identical bytes.
#include "attn_wide.hpp"
#include "../../include/gmlm_hip_gqa_band.h"

namespace gmlm {
namespace gqab {

using grouped::Params, grouped::Seqs, widehead::NT, widehead::R;

constexpr int D = 256;
template <typename T> using Lds = widehead::Lds<T, D>;

struct BandParams {
  Params g;
  int64_t window;          // >= 1: key j is visible to query i iff |i - j| < window (causal: and j <= i)
};

template <typename T, bool CAUSAL>
__global__ __launch_bounds__(NT) void fwd_kernel(BandParams x) {
  const Item it = decode(x.g.a);
  widehead::fwd_body<T, D, false, CAUSAL, true, true>(x.g, it, x.window);
}

// delta = rowsum(dO * O) over rows of [seqs * lq, hq, 256]
template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                    int64_t rows /* seqs * lq * hn */, int64_t lq, int64_t hn, float* __restrict__ delta) {
  widehead::delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);
}

template <typename T, bool CAUSAL>
__global__ __launch_bounds__(NT) void dq_kernel(BandParams x) {
  const Item it = decode(x.g.a);
  widehead::dq_body<T, D, false, CAUSAL, true, true>(x.g, it, x.window);
}

template <typename T, bool CAUSAL>
__global__ __launch_bounds__(NT) void dkv_kernel(BandParams x) {
  const CausalKeyTile it = causal_key_tile(x.g.a, x.g.group);       // key tile, sequence, KV head, first row, rows
  widehead::dkv_body<T, D, false, CAUSAL, true, true>(x.g, it, x.window);
}

// the words and grids of gmlm_attention_gqa_d256_*
static const grouped::Contract kContract = {"this entry point takes 256", "self-attention", "grouped", R};

template <typename T, bool CAUSAL> static int set_attrs() {
  constexpr int kLds = Lds<T>::BYTES;
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fwd_kernel<T, CAUSAL>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dq_kernel<T, CAUSAL>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dkv_kernel<T, CAUSAL>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  return GMLM_OK;
}
static int prepare() {
  static PerDeviceOnce once;
  return once([]() -> int {
    int rc;
    if ((rc = set_attrs<bf16_t, false>()) != GMLM_OK) return rc;
    if ((rc = set_attrs<bf16_t, true>()) != GMLM_OK) return rc;
    if ((rc = set_attrs<float, false>()) != GMLM_OK) return rc;
    return set_attrs<float, true>();
  });
}

#define GMLM_GQAB_LAUNCH(KERNEL, GRID)                                                              \
  do {                                                                                              \
    const dim3 grid_((unsigned)(GRID));                                                             \
    if (dtype == GMLM_BF16) {                                                                       \
      if (causal) KERNEL<bf16_t, true><<<grid_, NT, Lds<bf16_t>::BYTES, st>>>(x);                   \
      else KERNEL<bf16_t, false><<<grid_, NT, Lds<bf16_t>::BYTES, st>>>(x);                         \
    } else {                                                                                        \
      if (causal) KERNEL<float, true><<<grid_, NT, Lds<float>::BYTES, st>>>(x);                     \
      else KERNEL<float, false><<<grid_, NT, Lds<float>::BYTES, st>>>(x);                           \
    }                                                                                               \
    GMLM_LAUNCH_CHECK();                                                                            \
  } while (0)

// ---- the entry points: a padded export passes grouped::padded(...), its varlen twin grouped::packed(...) -----------------------
static int fwd(const char* who, const Seqs& s, const void* q, const void* k, const void* v, int64_t hq, int64_t hkv, int64_t d,
               int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p, int causal, int64_t window, void* out,
               void* out_lo, float* lse, int dtype, gmlm_stream_t stream) {
  BandParams x;
  int rc = grouped::setup(kContract, d == D, who, x.g, s, q, k, v, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype,
                          window);
  if (rc != GMLM_OK) return rc;
  if (s.empty()) return GMLM_OK;
  x.window = window;
  x.g.a.o_w = out; x.g.a.o_lo_w = out_lo; x.g.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.g.a, hq * d, hkv * d, dtype)) != GMLM_OK) return rc;
  if ((rc = prepare()) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  GMLM_GQAB_LAUNCH(fwd_kernel, cdiv(s.len, R) * s.n * hq);
  return GMLM_OK;
}

static int bwd(const char* who, const Seqs& s, const void* q, const void* k, const void* v, const void* out, const void* out_lo,
               const void* dout, const float* lse, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride, int64_t k_stride,
               int64_t v_stride, float scale, float dropout_p, int causal, int64_t window, void* dq, void* dk, void* dv, int64_t dq_stride,
               int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  BandParams x;
  int rc = grouped::setup(kContract, d == D, who, x.g, s, q, k, v, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype,
                          window);
  if (rc != GMLM_OK) return rc;
  if (s.empty()) return GMLM_OK;
  x.window = window;
  AttnParams& p = x.g.a;
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, p, hq * d, hkv * d, dtype, workspace_bytes, attn_delta_bytes(s.lse_seqs(), hq, s.rows))) != GMLM_OK)
    return rc;
  if ((rc = prepare()) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t drows = s.lse_seqs() * s.rows * hq;
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, drows, 64, st, s.rows, hq);       // one wave per row
  GMLM_LAUNCH_CHECK();
  GMLM_GQAB_LAUNCH(dq_kernel, cdiv(s.len, R) * s.n * hq);
  GMLM_GQAB_LAUNCH(dkv_kernel, cdiv(s.len, R) * s.n * hkv);
  return GMLM_OK;
}

}  // namespace gqab
}  // namespace gmlm

using namespace gmlm;

extern "C" int gmlm_attention_gqa_d256_band_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                                int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                                int64_t v_stride, float scale, float dropout_p, int causal, int64_t window, void* out,
                                                void* out_lo, float* lse, int dtype, gmlm_stream_t stream) {
  return gqab::fwd("attention_gqa_d256_band_fwd", grouped::padded(kv_len, b, lq, lk), q, k, v, hq, hkv, d, q_stride, k_stride, v_stride,
                   scale, dropout_p, causal, window, out, out_lo, lse, dtype, stream);
}

extern "C" size_t gmlm_attention_gqa_d256_band_bwd_workspace_bytes(int64_t b, int64_t hq, int64_t lq) { return attn_delta_bytes(b, hq, lq); }

extern "C" int gmlm_attention_gqa_d256_band_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                                const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq,
                                                int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                                int64_t v_stride, float scale, float dropout_p, int causal, int64_t window, void* dq,
                                                void* dk, void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                                void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  return gqab::bwd("attention_gqa_d256_band_bwd", grouped::padded(kv_len, b, lq, lk), q, k, v, out, out_lo, dout, lse, hq, hkv, d, q_stride,
                   k_stride, v_stride, scale, dropout_p, causal, window, dq, dk, dv, dq_stride, dk_stride, dv_stride, dtype, workspace,
                   workspace_bytes, stream);
}

extern "C" int gmlm_attention_gqa_d256_band_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                                       int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv,
                                                       int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                                       float dropout_p, int causal, int64_t window, void* out, void* out_lo, float* lse,
                                                       int dtype, gmlm_stream_t stream) {
  return gqab::fwd("attention_gqa_d256_band_varlen_fwd", grouped::packed(cu_seqlens, num_seqs, max_len, total_rows), q, k, v, hq, hkv, d,
                   q_stride, k_stride, v_stride, scale, dropout_p, causal, window, out, out_lo, lse, dtype, stream);
}

extern "C" size_t gmlm_attention_gqa_d256_band_varlen_bwd_workspace_bytes(int64_t total_rows, int64_t hq) {
  return attn_delta_bytes(1, hq, total_rows);   // delta [hq, total_rows]
}

extern "C" int gmlm_attention_gqa_d256_band_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                                       const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                                       int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d,
                                                       int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                                                       int causal, int64_t window, void* dq, void* dk, void* dv, int64_t dq_stride,
                                                       int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                                       size_t workspace_bytes, gmlm_stream_t stream) {
  return gqab::bwd("attention_gqa_d256_band_varlen_bwd", grouped::packed(cu_seqlens, num_seqs, max_len, total_rows), q, k, v, out, out_lo,
                   dout, lse, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, causal, window, dq, dk, dv, dq_stride, dk_stride,
                   dv_stride, dtype, workspace, workspace_bytes, stream);
}
