// Attention at head dims 256 / 384 / 512, forward + backward, gfx950 MFMA (gmlm_attention_wide_*; C ABI in
// include/gmlm_hip_wide.h), all in namespace gmlm::wide.
// Shape: padded [b, l, h*D] with an optional per-sequence key length, lq != lk and in-kernel probability dropout: the CrossAttention
// (8 heads) of a text encoder 2,048 to 4,096 wide (Qwen3-Embedding-4B: 8 x 320 zero-padded to 384; -8B: 8 x 512).
// The kernel plan (the head dim split over four waves, the exchange of partial score tiles through LDS) and the loop bodies are
// in attn_wide.hpp, shared with the grouped family of attn_gqa_wide.hip; this family is its DROP flag at three head dims, with
// CAUSAL = GROUPED = false.  Here: the kernels under their names, the argument checks (attn_host.hpp) with this family's head
// dims and work-item bound, the dynamic-LDS attributes, the launches and the exports.
#include "attn_wide.hpp"
#include "../../include/gmlm_hip_wide.h"

namespace gmlm {
namespace wide {

using widehead::Params, widehead::Lds, widehead::NT, widehead::R;

template <typename T, int D, bool DROP>
__global__ __launch_bounds__(NT) void fwd_kernel(Params x) {
  const Item it = decode(x.a);
  widehead::fwd_body<T, D, DROP, false, false>(x, it);
}

// delta = rowsum(dO * O) over rows of [b * lq, h, d]
template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                    int64_t rows /* b * lq * h */, int d, int64_t lq, int64_t hn, float* __restrict__ delta) {
  widehead::delta_body<T>(o, o_lo, dout, rows, d, lq, hn, delta);
}

template <typename T, int D, bool DROP>
__global__ __launch_bounds__(NT) void dq_kernel(Params x) {
  const Item it = decode(x.a);
  widehead::dq_body<T, D, DROP, false, false>(x, it);
}

template <typename T, int D, bool DROP>
__global__ __launch_bounds__(NT) void dkv_kernel(Params x) {
  const Item it = decode(x.a);
  widehead::dkv_body<T, D, DROP, false, false>(x, it);
}

// the checks of attn_host.hpp up to the empty-problem return, with this family's head dims and work-item bound; fills the
// launch parameters
static int setup(const char* who, Params& x, const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                 int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                 uint64_t seed, const uint64_t* seed_dev, const void* out_lo, int dtype) {
  int rc = attn_check_shape(who, b >= 0 && h > 0 && lq >= 0 && lk >= 0, d == 256 || d == 384 || d == 512, d,
                            "this entry point takes 256, 384 and 512", dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  if ((rc = attn_check_rates(who, dropout_p, nullptr, scale)) != GMLM_OK) return rc;
  const int64_t rows = lq > lk ? lq : lk;
  GMLM_REQUIRE(b < ((int64_t)1 << 31) && h < ((int64_t)1 << 31) && rows < ((int64_t)1 << 31) &&
                   (double)cdiv(rows, R) * (double)b * (double)h < 2147483648.0 &&
                   (double)lq * (double)b * (double)h < 4.0 * 2147483648.0,      // the delta launch: one wave per (b, q, h) row
               "%s: too many work items", who);
  x = Params{};
  attn_fill(x.a, q, k, v, kv_len, b, h, lq, lk, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev);
  x.dout_stride = h * d;
  return GMLM_OK;
}

// > 64 KiB of dynamic LDS needs the attribute once per instantiation and device
template <typename T, int D> static int set_attrs() {
  constexpr int kLds = Lds<T, D>::BYTES;
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fwd_kernel<T, D, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fwd_kernel<T, D, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dq_kernel<T, D, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dq_kernel<T, D, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dkv_kernel<T, D, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dkv_kernel<T, D, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  return GMLM_OK;
}
static int prepare() {
  static PerDeviceOnce once;
  return once([]() -> int {
    int rc;
    if ((rc = set_attrs<bf16_t, 256>()) != GMLM_OK) return rc;
    if ((rc = set_attrs<bf16_t, 384>()) != GMLM_OK) return rc;
    if ((rc = set_attrs<bf16_t, 512>()) != GMLM_OK) return rc;
    if ((rc = set_attrs<float, 256>()) != GMLM_OK) return rc;
    if ((rc = set_attrs<float, 384>()) != GMLM_OK) return rc;
    return set_attrs<float, 512>();
  });
}

}  // namespace wide
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::wide;

#define GMLM_WIDE_K(KERNEL, T, DD, DR) KERNEL<T, DD, DR><<<grid, NT, Lds<T, DD>::BYTES, st>>>(x)
#define GMLM_WIDE_D(KERNEL, T, DR)                         \
  do {                                                     \
    if (d == 256) GMLM_WIDE_K(KERNEL, T, 256, DR);         \
    else if (d == 384) GMLM_WIDE_K(KERNEL, T, 384, DR);    \
    else GMLM_WIDE_K(KERNEL, T, 512, DR);                  \
  } while (0)
#define GMLM_WIDE_LAUNCH(KERNEL)                           \
  do {                                                     \
    const bool dr_ = x.a.drop_thresh != 0;                 \
    if (dtype == GMLM_BF16) {                              \
      if (dr_) GMLM_WIDE_D(KERNEL, bf16_t, true);          \
      else GMLM_WIDE_D(KERNEL, bf16_t, false);             \
    } else {                                               \
      if (dr_) GMLM_WIDE_D(KERNEL, float, true);           \
      else GMLM_WIDE_D(KERNEL, float, false);              \
    }                                                      \
  } while (0)

extern "C" int gmlm_attention_wide_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                                       int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                       float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* out,
                                       void* out_lo, float* lse, int dtype, gmlm_stream_t stream) {
  static const char* who = "attention_wide_fwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, h * d, h * d, dtype)) != GMLM_OK) return rc;
  if ((rc = prepare()) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(cdiv(lq, R) * b * h));
  GMLM_WIDE_LAUNCH(fwd_kernel);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_wide_bwd_workspace_bytes(int64_t b, int64_t h, int64_t lq) {
  return attn_delta_bytes(b, h, lq);
}

extern "C" int gmlm_attention_wide_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                       const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t h,
                                       int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                       float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* dq, void* dk,
                                       void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                       void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "attention_wide_bwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, h, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, seed, seed_dev, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || (lq == 0 && lk == 0)) return GMLM_OK;
  GMLM_REQUIRE(lq > 0 && lk > 0, "%s: empty query or key set with a non-empty counterpart is not supported", who);
  AttnParams& p = x.a;
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, p, h * d, h * d, dtype, workspace_bytes, attn_delta_bytes(b, h, lq))) != GMLM_OK) return rc;
  if ((rc = prepare()) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t rows = b * lq * h;
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, rows, 64, st, (int)d, lq, h);     // one wave per row
  GMLM_LAUNCH_CHECK();
  {
    const dim3 grid((unsigned)(cdiv(lq, R) * b * h));
    GMLM_WIDE_LAUNCH(dq_kernel);
    GMLM_LAUNCH_CHECK();
  }
  {
    const dim3 grid((unsigned)(cdiv(lk, R) * b * h));
    GMLM_WIDE_LAUNCH(dkv_kernel);
    GMLM_LAUNCH_CHECK();
  }
  return GMLM_OK;
}
