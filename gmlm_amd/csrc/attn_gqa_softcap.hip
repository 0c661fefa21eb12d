// Soft-capped self-attention with grouped KV heads at head dim 256, causal or bidirectional, with or without a band, padded or
// packed, forward + backward, gfx950 MFMA (gmlm_attention_gqa_d256_softcap_*; C ABI in include/gmlm_hip_gqa_softcap.h), all in
// namespace gmlm::gqac: the attention of a Gemma2 text encoder (hf:modeling_gemma2.py eager_attention_forward), whose scores enter
// the softmax as z = c tanh(q.k scale / c), capped BEFORE the mask.  Every kernel IS a body of attn_wide.hpp at GROUPED = true,
// D = 256 with its SOFTCAP flag, with and without BAND (what the flags change is said there); the launch parameters are
// grouped::Params plus the window and the cap, in a struct of this file.  The argument checks are grouped::setup with the words of
// gmlm_attention_gqa_d256_*, the window check (0 = no band) after the scale check and the cap check after setup.  Here: the kernels
// under their names, the dynamic-LDS attributes (81.3 KiB in fp32), the launches and the exports.  No atomics and no scratch: a
// repeated call gives identical bytes.
// Also here: gmlm_rope_heads_d256_*, the rotary embedding on head rows without a head norm (at the end of the file).
#include <cmath>
#include "attn_wide.hpp"
#include "row_kernels.hpp"
#include "../../include/gmlm_hip_gqa_softcap.h"

namespace gmlm {
namespace gqac {

using grouped::Params, grouped::Seqs, widehead::NT, widehead::R;

constexpr int D = 256;
template <typename T> using Lds = widehead::Lds<T, D>;

struct CapParams {
  Params g;
  int64_t window;          // 0: no band; >= 1: key j is visible to query i iff |i - j| < window (causal: and j <= i)
  float softcap;           // c > 0: the scores enter the softmax as c tanh(score * scale / c)
};

template <typename T, bool CAUSAL, bool BAND>
__global__ __launch_bounds__(NT) void fwd_kernel(CapParams x) {
  const Item it = decode(x.g.a);
  widehead::fwd_body<T, D, false, CAUSAL, true, BAND, true>(x.g, it, x.window, x.softcap);
}

// delta = rowsum(dO * O) over rows of [seqs * lq, hq, 256]
template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                    int64_t rows /* seqs * lq * hn */, int64_t lq, int64_t hn, float* __restrict__ delta) {
  widehead::delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);
}

template <typename T, bool CAUSAL, bool BAND>
__global__ __launch_bounds__(NT) void dq_kernel(CapParams x) {
  const Item it = decode(x.g.a);
  widehead::dq_body<T, D, false, CAUSAL, true, BAND, true>(x.g, it, x.window, x.softcap);
}

template <typename T, bool CAUSAL, bool BAND>
__global__ __launch_bounds__(NT) void dkv_kernel(CapParams x) {
  const CausalKeyTile it = causal_key_tile(x.g.a, x.g.group);       // key tile, sequence, KV head, first row, rows
  widehead::dkv_body<T, D, false, CAUSAL, true, BAND, true>(x.g, it, x.window, x.softcap);
}

// the words and grids of gmlm_attention_gqa_d256_*
static const grouped::Contract kContract = {"this entry point takes 256", "self-attention", "grouped", R};

template <typename T, bool CAUSAL, bool BAND> static int set_attrs_one() {
  constexpr int kLds = Lds<T>::BYTES;
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&fwd_kernel<T, CAUSAL, BAND>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dq_kernel<T, CAUSAL, BAND>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&dkv_kernel<T, CAUSAL, BAND>), hipFuncAttributeMaxDynamicSharedMemorySize, kLds));
  return GMLM_OK;
}
template <typename T, bool CAUSAL> static int set_attrs() {
  const int rc = set_attrs_one<T, CAUSAL, false>();
  return rc != GMLM_OK ? rc : set_attrs_one<T, CAUSAL, true>();
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

#define GMLM_GQAC_PICK(KERNEL, T)                                                                   \
  do {                                                                                              \
    if (causal) {                                                                                   \
      if (x.window) KERNEL<T, true, true><<<grid_, NT, Lds<T>::BYTES, st>>>(x);                     \
      else KERNEL<T, true, false><<<grid_, NT, Lds<T>::BYTES, st>>>(x);                             \
    } else {                                                                                        \
      if (x.window) KERNEL<T, false, true><<<grid_, NT, Lds<T>::BYTES, st>>>(x);                    \
      else KERNEL<T, false, false><<<grid_, NT, Lds<T>::BYTES, st>>>(x);                            \
    }                                                                                               \
  } while (0)
#define GMLM_GQAC_LAUNCH(KERNEL, GRID)                                                              \
  do {                                                                                              \
    const dim3 grid_((unsigned)(GRID));                                                             \
    if (dtype == GMLM_BF16) GMLM_GQAC_PICK(KERNEL, bf16_t);                                         \
    else GMLM_GQAC_PICK(KERNEL, float);                                                             \
    GMLM_LAUNCH_CHECK();                                                                            \
  } while (0)

// window 0 = no band: grouped::setup checks a window only when it is given one, so every other value goes through its check
static std::optional<int64_t> band_arg(int64_t window) { return window == 0 ? std::nullopt : std::optional<int64_t>(window); }
#define GMLM_GQAC_SOFTCAP_CHECK() \
  GMLM_REQUIRE(std::isfinite(softcap) && softcap > 0.f, "%s: softcap %g must be finite and > 0", who, (double)softcap)

// ---- the entry points: a padded export passes grouped::padded(...), its varlen twin grouped::packed(...) -----------------------
static int fwd(const char* who, const Seqs& s, const void* q, const void* k, const void* v, int64_t hq, int64_t hkv, int64_t d,
               int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p, int causal, int64_t window, float softcap,
               void* out, void* out_lo, float* lse, int dtype, gmlm_stream_t stream) {
  CapParams x;
  int rc = grouped::setup(kContract, d == D, who, x.g, s, q, k, v, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype,
                          band_arg(window));
  if (rc != GMLM_OK) return rc;
  GMLM_GQAC_SOFTCAP_CHECK();
  if (s.empty()) return GMLM_OK;
  x.window = window;
  x.softcap = softcap;
  x.g.a.o_w = out; x.g.a.o_lo_w = out_lo; x.g.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.g.a, hq * d, hkv * d, dtype)) != GMLM_OK) return rc;
  if ((rc = prepare()) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  GMLM_GQAC_LAUNCH(fwd_kernel, cdiv(s.len, R) * s.n * hq);
  return GMLM_OK;
}

static int bwd(const char* who, const Seqs& s, const void* q, const void* k, const void* v, const void* out, const void* out_lo,
               const void* dout, const float* lse, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride, int64_t k_stride,
               int64_t v_stride, float scale, float dropout_p, int causal, int64_t window, float softcap, void* dq, void* dk, void* dv, int64_t dq_stride,
               int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  CapParams x;
  int rc = grouped::setup(kContract, d == D, who, x.g, s, q, k, v, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype,
                          band_arg(window));
  if (rc != GMLM_OK) return rc;
  GMLM_GQAC_SOFTCAP_CHECK();
  if (s.empty()) return GMLM_OK;
  x.window = window;
  x.softcap = softcap;
  AttnParams& p = x.g.a;
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, p, hq * d, hkv * d, dtype, workspace_bytes, attn_delta_bytes(s.lse_seqs(), hq, s.rows))) != GMLM_OK)
    return rc;
  if ((rc = prepare()) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t drows = s.lse_seqs() * s.rows * hq;
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, drows, 64, st, s.rows, hq);       // one wave per row
  GMLM_LAUNCH_CHECK();
  GMLM_GQAC_LAUNCH(dq_kernel, cdiv(s.len, R) * s.n * hq);
  GMLM_GQAC_LAUNCH(dkv_kernel, cdiv(s.len, R) * s.n * hkv);
  return GMLM_OK;
}

}  // namespace gqac
}  // namespace gmlm

using namespace gmlm;

extern "C" int gmlm_attention_gqa_d256_softcap_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                                int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                                int64_t v_stride, float scale, float dropout_p, int causal, int64_t window, float softcap, void* out,
                                                void* out_lo, float* lse, int dtype, gmlm_stream_t stream) {
  return gqac::fwd("attention_gqa_d256_softcap_fwd", grouped::padded(kv_len, b, lq, lk), q, k, v, hq, hkv, d, q_stride, k_stride, v_stride,
                   scale, dropout_p, causal, window, softcap, out, out_lo, lse, dtype, stream);
}

extern "C" size_t gmlm_attention_gqa_d256_softcap_bwd_workspace_bytes(int64_t b, int64_t hq, int64_t lq) { return attn_delta_bytes(b, hq, lq); }

extern "C" int gmlm_attention_gqa_d256_softcap_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                                const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq,
                                                int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                                int64_t v_stride, float scale, float dropout_p, int causal, int64_t window, float softcap, void* dq,
                                                void* dk, void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                                void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  return gqac::bwd("attention_gqa_d256_softcap_bwd", grouped::padded(kv_len, b, lq, lk), q, k, v, out, out_lo, dout, lse, hq, hkv, d, q_stride,
                   k_stride, v_stride, scale, dropout_p, causal, window, softcap, dq, dk, dv, dq_stride, dk_stride, dv_stride, dtype, workspace,
                   workspace_bytes, stream);
}

extern "C" int gmlm_attention_gqa_d256_softcap_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                                       int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv,
                                                       int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                                       float dropout_p, int causal, int64_t window, float softcap, void* out, void* out_lo, float* lse,
                                                       int dtype, gmlm_stream_t stream) {
  return gqac::fwd("attention_gqa_d256_softcap_varlen_fwd", grouped::packed(cu_seqlens, num_seqs, max_len, total_rows), q, k, v, hq, hkv, d,
                   q_stride, k_stride, v_stride, scale, dropout_p, causal, window, softcap, out, out_lo, lse, dtype, stream);
}

extern "C" size_t gmlm_attention_gqa_d256_softcap_varlen_bwd_workspace_bytes(int64_t total_rows, int64_t hq) {
  return attn_delta_bytes(1, hq, total_rows);   // delta [hq, total_rows]
}

extern "C" int gmlm_attention_gqa_d256_softcap_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                                       const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                                       int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d,
                                                       int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                                                       int causal, int64_t window, float softcap, void* dq, void* dk, void* dv, int64_t dq_stride,
                                                       int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                                       size_t workspace_bytes, gmlm_stream_t stream) {
  return gqac::bwd("attention_gqa_d256_softcap_varlen_bwd", grouped::packed(cu_seqlens, num_seqs, max_len, total_rows), q, k, v, out, out_lo,
                   dout, lse, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, causal, window, softcap, dq, dk, dv, dq_stride, dk_stride,
                   dv_stride, dtype, workspace, workspace_bytes, stream);
}

// ---- rotary embedding on head rows at d = 256 ---------------------------------------------------------------------------------
// gqa::rope_heads_kernel of attn_gqa.hip written out at D = 256 with the rotary pieces of row_kernels.hpp: a head row = LPR lanes
// x 16 bytes, 32 lanes in bf16 and 64 in fp32, where the partner lane (lane ^ 32) is in the other half of the wave, which the
// exchange of rotate_half over 64 lanes reaches (gmlm_qknorm_rope_d256_* runs it at the same width).  Every lane reads its 16
// bytes and writes the same 16 bytes back: in place without a hazard.  fp32 arithmetic, one rounding on store.
namespace gmlm {
namespace gqac {

constexpr int kRopeMaxBlocks = 2048;

template <typename T, bool INV>
__global__ __launch_bounds__(256) void rope_heads_d256_kernel(T* __restrict__ qkv, int64_t stride, const float* __restrict__ cs,
                                                              int64_t tokens, int64_t seq_len, int nh /* hq + hkv head rows per token */,
                                                              const int32_t* __restrict__ pos_ids, int64_t max_len) {
  constexpr int V = Store<T>::kVec, LPR = D / V, GPB = 256 / LPR;
  static_assert(LPR <= 64 && 256 % LPR == 0, "a head row must lie inside one wave");
  const int lr = threadIdx.x % LPR, grp = threadIdx.x / LPR;
  const int col = (lr * V) & (D / 2 - 1);
  const bool upper = lr >= LPR / 2;
  const int64_t items = tokens * nh;
  // the trip count is block-uniform: every lane of a wave reaches the exchange of every trip
  for (int64_t first = (int64_t)blockIdx.x * GPB; first < items; first += (int64_t)gridDim.x * GPB) {
    int64_t t;
    int hd;
    const bool live = head_row(first + grp, items, nh, t, hd);
    const float* csr = rope_row<D>(cs, t, seq_len, pos_ids, max_len);
    T* ptr = qkv + t * stride + (int64_t)hd * D + lr * V;
    float x[V], c[V], sn[V], o[V];
    Store<T>::ldv(ptr, x);
    load_f32<V>(csr + col, c);
    load_f32<V>(csr + D / 2 + col, sn);
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = rotate_half<LPR, INV>(x[v], c[v], sn[v], upper);
    if (live) Store<T>::stv(ptr, o);
  }
}

// the checks of gmlm_rope_heads_* in their order, with 256 as the one head dim
template <bool INV>
static int rope_heads_d256(const char* who, void* qkv, int64_t stride, const float* cos_sin, int64_t max_len, int64_t tokens,
                           int64_t seq_len, const int32_t* pos_ids, int64_t heads, int64_t d, int dtype, gmlm_stream_t stream) {
  GMLM_REQUIRE(dtype == GMLM_F32 || dtype == GMLM_BF16, "%s: unsupported dtype", who);
  GMLM_REQUIRE(d == D, "%s: head dim %ld not supported (this entry point takes 256)", who, (long)d);
  GMLM_REQUIRE(tokens >= 0 && heads > 0 && heads < 4096, "%s: bad sizes", who);
  GMLM_REQUIRE(max_len > 0, "%s: empty cos / sin table", who);
  if (!pos_ids) {
    GMLM_REQUIRE(seq_len >= 0 && seq_len <= max_len, "%s: sequence length %ld exceeds the %ld rows of the cos / sin table", who,
                 (long)seq_len, (long)max_len);
    GMLM_REQUIRE(seq_len > 0 || tokens == 0, "%s: %ld tokens in sequences of length 0", who, (long)tokens);
  }
  const int v = dtype == GMLM_F32 ? 4 : 8;
  GMLM_REQUIRE(stride >= heads * d && stride % v == 0, "%s: qkv row stride %ld must be >= %ld and a multiple of %d", who, (long)stride,
               (long)(heads * d), v);
  GMLM_REQUIRE(tokens * heads < ((int64_t)1 << 34), "%s: too many head rows", who);
  if (tokens == 0) return GMLM_OK;
  GMLM_REQUIRE(qkv && aligned16(qkv), "%s: null or not 16-byte aligned pointer", who);
  GMLM_REQUIRE(cos_sin && aligned16(cos_sin), "%s: null or misaligned cos / sin table", who);
  hipStream_t st = as_stream(stream);
  const int64_t items = tokens * heads, gpb = 256 / (d / v);     // head rows per block
  const int grid = grid_cap(cdiv(items, gpb), kRopeMaxBlocks);
  if (dtype == GMLM_BF16)
    rope_heads_d256_kernel<bf16_t, INV><<<grid, 256, 0, st>>>((bf16_t*)qkv, stride, cos_sin, tokens, seq_len, (int)heads, pos_ids, max_len);
  else
    rope_heads_d256_kernel<float, INV><<<grid, 256, 0, st>>>((float*)qkv, stride, cos_sin, tokens, seq_len, (int)heads, pos_ids, max_len);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

}  // namespace gqac
}  // namespace gmlm

extern "C" int gmlm_rope_heads_d256_fwd(void* qkv, int64_t qkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens,
                                        int64_t seq_len, const int32_t* pos_ids, int64_t heads, int64_t d, int dtype,
                                        gmlm_stream_t stream) {
  return gqac::rope_heads_d256<false>("rope_heads_d256_fwd", qkv, qkv_stride, cos_sin, max_len, tokens, seq_len, pos_ids, heads, d, dtype, stream);
}

extern "C" int gmlm_rope_heads_d256_bwd(void* dqkv, int64_t dqkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens,
                                        int64_t seq_len, const int32_t* pos_ids, int64_t heads, int64_t d, int dtype,
                                        gmlm_stream_t stream) {
  return gqac::rope_heads_d256<true>("rope_heads_d256_bwd", dqkv, dqkv_stride, cos_sin, max_len, tokens, seq_len, pos_ids, heads, d, dtype, stream);
}
