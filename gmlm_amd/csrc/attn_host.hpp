// Host contract of the attention entry points (gmlm_attention_*, _d128_*, _d32_*, _wide_*, _causal_d128_*, _causal_d128_varlen_*):
// the argument checks every family makes, in ONE order, and the launch parameters every family fills the same way.  No device
// code here.  An entry point validates in this order (include/gmlm_hip.h), the first failure deciding code and message:
//   1 sizes  2 head dim  3 dtype  4 out_lo         attn_check_shape
//   5 layout (packed mode, seq_groups, lq == lk, GQA divisibility)   the family's own GMLM_REQUIRE lines
//   6 dropout  7 scale                              attn_check_rates
//   8 the family's work-item bound                  its own GMLM_REQUIRE line
// then the empty-problem return, then attn_check_fwd_operands / attn_check_bwd_operands (operands, outputs, workspace last).
// What differs between families is passed in as data; every message keeps the entry point's name (`who`) as its prefix.
#pragma once
#include "attn_common.hpp"

namespace gmlm {

// 8-bit dropout threshold: P(drop) = th / 256 (|error| <= 2e-3: 0.1 -> 0.1016, 0.3 -> 0.3008), keep scale uses the quantised rate
inline uint32_t drop8(float p) { long t = lroundf(p * 256.f); return (uint32_t)(t < 0 ? 0 : (t > 255 ? 255 : t)); }

// checks 1-4.  sizes_ok: the family's size test (h > 0, or hq > 0 && hkv > 0); d_ok / dims: the head dims it takes and how its
// message names them
inline int attn_check_shape(const char* who, bool sizes_ok, bool d_ok, int64_t d, const char* dims, int dtype, const void* out_lo) {
  GMLM_REQUIRE(sizes_ok, "%s: bad sizes", who);
  GMLM_REQUIRE(d_ok, "%s: head dim %ld not supported (%s)", who, (long)d, dims);
  GMLM_REQUIRE(dtype == GMLM_F32 || dtype == GMLM_BF16, "%s: unsupported dtype", who);
  GMLM_REQUIRE(!out_lo || (dtype == GMLM_BF16 && aligned16(out_lo)), "%s: out_lo is the bf16 residual of a bf16 output (16-byte aligned)", who);
  return GMLM_OK;
}

// checks 6-7.  no_dropout: NULL for a family with dropout; else how the refusal names its kernels ("causal", "grouped"), which
// take dropout_p = 0 only
inline int attn_check_rates(const char* who, float dropout_p, const char* no_dropout, float scale) {
  if (!no_dropout) GMLM_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, "%s: dropout_p must be in [0,1)", who);
  else GMLM_REQUIRE(dropout_p == 0.f, "%s: attention-probability dropout is not implemented for the %s kernels (dropout_p must be 0)", who, no_dropout);
  GMLM_REQUIRE(scale > 0.f, "%s: scale must be positive", who);
  return GMLM_OK;
}

// operand `what` of entry point `who`: 16-byte aligned rows of at least min_stride elements
inline int attn_stride_check(const char* who, const char* what, const void* ptr, int64_t stride, int64_t min_stride, int dtype) {
  const int v = dtype == GMLM_F32 ? 4 : 8;
  GMLM_REQUIRE(ptr && aligned16(ptr), "%s(%s): null or not 16-byte aligned pointer", who, what);
  GMLM_REQUIRE(stride >= min_stride && stride % v == 0 && stride < (1 << 24),
               "%s(%s): row stride %ld must be >= %ld, < 2^24 and a multiple of %d", who, what, (long)stride, (long)min_stride, v);
  return GMLM_OK;
}

// the fields every entry point sets the same way (the packed-mode fields are the caller's)
inline void attn_fill(AttnParams& p, const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                      int64_t lq, int64_t lk, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                      uint64_t seed, const uint64_t* seed_dev) {
  p.q = q; p.k = k; p.v = v; p.kv_len = kv_len;
  p.b = b; p.h = h; p.lq = lq; p.lk = lk; p.q_stride = q_stride; p.k_stride = k_stride; p.v_stride = v_stride;
  p.scale = scale; p.seed = seed; p.seed_dev = seed_dev;
  p.drop_thresh = drop8(dropout_p); p.keep_scale = 256.f / (256.f - (float)p.drop_thresh);
}
// the backward half; delta is the whole workspace
inline void attn_fill_bwd(AttnParams& p, const void* out, const void* out_lo, const void* dout, const float* lse, void* dq, void* dk,
                          void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, void* workspace) {
  p.out = out; p.out_lo = out_lo; p.dout = dout; p.lse = lse;
  p.delta = static_cast<float*>(workspace);
  p.dq = dq; p.dk = dk; p.dv = dv;
  p.dq_stride = dq_stride; p.dk_stride = dk_stride; p.dv_stride = dv_stride;
}

// operands of a filled forward call: q; k / v when there are keys; out.  wq / wkv: the least row width on the query side and on
// the KV side (h * d; hq * d and hkv * d with grouped KV heads)
inline int attn_check_fwd_operands(const char* who, const AttnParams& p, int64_t wq, int64_t wkv, int dtype) {
  int rc;
  if ((rc = attn_stride_check(who, "q", p.q, p.q_stride, wq, dtype)) != GMLM_OK) return rc;
  if (p.lk > 0) {
    if ((rc = attn_stride_check(who, "k", p.k, p.k_stride, wkv, dtype)) != GMLM_OK) return rc;
    if ((rc = attn_stride_check(who, "v", p.v, p.v_stride, wkv, dtype)) != GMLM_OK) return rc;
  }
  GMLM_REQUIRE(p.o_w && aligned16(p.o_w), "%s: null or misaligned out", who);
  return GMLM_OK;
}

// the six strided tensors of a filled backward call: q, k, v, then dq, dk, dv
inline int attn_check_bwd_strides(const char* who, const AttnParams& p, int64_t wq, int64_t wkv, int dtype) {
  int rc;
  if ((rc = attn_stride_check(who, "q", p.q, p.q_stride, wq, dtype)) != GMLM_OK) return rc;
  if ((rc = attn_stride_check(who, "k", p.k, p.k_stride, wkv, dtype)) != GMLM_OK) return rc;
  if ((rc = attn_stride_check(who, "v", p.v, p.v_stride, wkv, dtype)) != GMLM_OK) return rc;
  if ((rc = attn_stride_check(who, "dq", p.dq, p.dq_stride, wq, dtype)) != GMLM_OK) return rc;
  if ((rc = attn_stride_check(who, "dk", p.dk, p.dk_stride, wkv, dtype)) != GMLM_OK) return rc;
  return attn_stride_check(who, "dv", p.dv, p.dv_stride, wkv, dtype);
}

// operands of a filled backward call, then its outputs, then the workspace (p.delta; `need` = the family's *_workspace_bytes)
inline int attn_check_bwd_operands(const char* who, const AttnParams& p, int64_t wq, int64_t wkv, int dtype, size_t workspace_bytes,
                                   size_t need) {
  const int rc = attn_check_bwd_strides(who, p, wq, wkv, dtype);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(p.out && p.dout && p.lse && aligned16(p.out) && aligned16(p.dout), "%s: null or misaligned out/dout/lse", who);
  GMLM_REQUIRE_WS(p.delta && workspace_bytes >= need, "%s: workspace too small", who);
  return GMLM_OK;
}

// the same for the one-launch short-sequence backwards (gqa_short, d32_short), which read neither out nor a workspace
inline int attn_check_short_bwd_operands(const char* who, const AttnParams& p, int64_t wq, int64_t wkv, int dtype) {
  const int rc = attn_check_bwd_strides(who, p, wq, wkv, dtype);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(p.dout && p.lse && aligned16(p.dout), "%s: null or misaligned dout/lse", who);
  return GMLM_OK;
}

// bytes of delta [b, h, lq] fp32 (packed: [h, total_rows], b = 1), the workspace of every backward; an empty problem still has a size
inline size_t attn_delta_bytes(int64_t b, int64_t h, int64_t lq) {
  return (size_t)(b > 0 && h > 0 && lq > 0 ? b * h * lq : 1) * sizeof(float);
}

// the delta launch of a streaming backward: KERNEL is the family's delta_kernel wrapper, `lanes` its threads per row, the
// variadic arguments what it takes between `rows` and `delta`.  Only bf16 has an output residual.  Needs `dtype` in scope.
#define GMLM_ATTN_DELTA_LAUNCH(KERNEL, p, rows, lanes, st, ...)                                                                \
  do {                                                                                                                         \
    const unsigned gd_ = (unsigned)cdiv((int64_t)(rows) * (lanes), (int64_t)256);                                              \
    if (dtype == GMLM_BF16)                                                                                                    \
      KERNEL<bf16_t><<<gd_, 256, 0, st>>>((const bf16_t*)(p).out, (const bf16_t*)(p).out_lo, (const bf16_t*)(p).dout, rows,    \
                                          __VA_ARGS__, (p).delta);                                                             \
    else                                                                                                                       \
      KERNEL<float><<<gd_, 256, 0, st>>>((const float*)(p).out, nullptr, (const float*)(p).dout, rows, __VA_ARGS__, (p).delta); \
  } while (0)

}  // namespace gmlm
