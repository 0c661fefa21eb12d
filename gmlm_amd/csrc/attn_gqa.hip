// Kernels of a Llama-architecture text encoder without the Q / K head norm (Llama, Qwen2, Mistral; C ABI in
// include/gmlm_hip_gqa.h), all in namespace gmlm::gqa:
//  * rope_heads: the rotate-half rotary embedding IN PLACE on the first `heads` = hq + hkv head rows of every token row of a
//    fused [q | k | v] buffer, at head dim 64 or 128 (the rotary pieces of row_kernels.hpp).  V columns are neither read nor
//    written.  A head row = D / V lanes x 16 bytes; every lane reads its 16 bytes, exchanges with the lane holding the other
//    half, and writes the same 16 bytes back: in place without a hazard.  fp32 arithmetic, one rounding on store; the table is
//    built on the host.  1-D grid capped at kRopeMaxBlocks, a block-uniform stride loop over groups of 256 / LPR head rows.
//    INV: the backward = the inverse rotation, so it needs no saved input and no workspace.
//  * causal attention with grouped KV heads at head dim 64 (gmlm_attention_causal_d64_*, padded and packed): one of the three
//    grouped families of attn_grouped.hpp (kernels described there; checks, launches and entry-point bodies held there),
//    CAUSAL = true at D = 64; here the kernels under their names, the family, the exports.
//    At D = 64 the tiles and the accumulators are half as large as at 128, so the register and LDS budget holds with room to
//    spare (DESIGN.md section 4 "Llama, Qwen2 and Mistral encoders").
#include "attn_grouped.hpp"
#include "row_kernels.hpp"
#include "../../include/gmlm_hip_gqa.h"

namespace gmlm {
namespace gqa {

// ---- rotary embedding over head rows ---------------------------------------------------------------
constexpr int kRopeMaxBlocks = 2048;

template <typename T, int D, bool INV>
__global__ __launch_bounds__(256) void rope_heads_kernel(T* __restrict__ qkv, int64_t stride, const float* __restrict__ cs,
                                                         int64_t tokens, int64_t seq_len, int nh /* hq + hkv head rows per token */,
                                                         const int32_t* __restrict__ pos_ids, int64_t max_len) {
  constexpr int V = Store<T>::kVec, LPR = D / V, GPB = 256 / LPR;
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

template <bool INV>
static int rope_heads(const char* who, void* qkv, int64_t stride, const float* cos_sin, int64_t max_len, int64_t tokens,
                      int64_t seq_len, const int32_t* pos_ids, int64_t heads, int64_t d, int dtype, gmlm_stream_t stream) {
  GMLM_REQUIRE(dtype == GMLM_F32 || dtype == GMLM_BF16, "%s: unsupported dtype", who);
  GMLM_REQUIRE(d == 64 || d == 128, "%s: head dim %ld not supported (this entry point takes 64 or 128)", who, (long)d);
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
#define GMLM_ROPE_HEADS_LAUNCH(T, D_)                                                                                          \
  rope_heads_kernel<T, D_, INV><<<grid, 256, 0, st>>>((T*)qkv, stride, cos_sin, tokens, seq_len, (int)heads, pos_ids, max_len)
  if (dtype == GMLM_BF16) { if (d == 64) GMLM_ROPE_HEADS_LAUNCH(bf16_t, 64); else GMLM_ROPE_HEADS_LAUNCH(bf16_t, 128); }
  else { if (d == 64) GMLM_ROPE_HEADS_LAUNCH(float, 64); else GMLM_ROPE_HEADS_LAUNCH(float, 128); }
#undef GMLM_ROPE_HEADS_LAUNCH
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

// ---- causal GQA attention at head dim 64 (attn_grouped.hpp) ------------------------------------------
using grouped::Params, grouped::NW, grouped::NT;
constexpr int D = 64;

template <typename T>
__global__ __launch_bounds__(NT) void causal64_fwd_kernel(Params x) {
  const Item it = decode(x.a);
  attn_fwd_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, true, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

// delta = rowsum(dO * O) over rows of [b * l, hq, 64]
template <typename T>
__global__ __launch_bounds__(256) void causal64_delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo,
                                                             const T* __restrict__ dout, int64_t rows /* b * l * hq */, int64_t lq,
                                                             int64_t hn, float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);
}

template <typename T>
__global__ __launch_bounds__(NT) void causal64_dq_kernel(Params x) {
  const Item it = decode(x.a);
  attn_dq_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, true, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

template <typename T>
__global__ __launch_bounds__(NT) void causal64_dkv_kernel(Params x) {
  const CausalKeyTile it = causal_key_tile(x.a, x.group);
  causal_dkv_body<T, D, NW, Cfg<T>::QT, Cfg<T>::DBUF, true>(x.a, x.dout_stride, x.group, it, clamp_kvlen(x.a, it.b, it.l));
}

static const grouped::Family kFamily = {
    {"this entry point takes 64", "causal self-attention", "causal"},
    {{causal64_fwd_kernel<bf16_t>, causal64_delta_kernel<bf16_t>, causal64_dq_kernel<bf16_t>, causal64_dkv_kernel<bf16_t>}, {}},
    {{causal64_fwd_kernel<float>, causal64_delta_kernel<float>, causal64_dq_kernel<float>, causal64_dkv_kernel<float>}, {}}};

}  // namespace gqa
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::gqa;

extern "C" int gmlm_rope_heads_fwd(void* qkv, int64_t qkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens,
                                   int64_t seq_len, const int32_t* pos_ids, int64_t heads, int64_t d, int dtype, gmlm_stream_t stream) {
  return rope_heads<false>("rope_heads_fwd", qkv, qkv_stride, cos_sin, max_len, tokens, seq_len, pos_ids, heads, d, dtype, stream);
}

extern "C" int gmlm_rope_heads_bwd(void* dqkv, int64_t dqkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens,
                                   int64_t seq_len, const int32_t* pos_ids, int64_t heads, int64_t d, int dtype, gmlm_stream_t stream) {
  return rope_heads<true>("rope_heads_bwd", dqkv, dqkv_stride, cos_sin, max_len, tokens, seq_len, pos_ids, heads, d, dtype, stream);
}

extern "C" int gmlm_attention_causal_d64_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                             int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                             int64_t v_stride, float scale, float dropout_p, void* out, void* out_lo, float* lse,
                                             int dtype, gmlm_stream_t stream) {
  return grouped::fwd(kFamily, "attention_causal_d64_fwd", grouped::padded(kv_len, b, lq, lk), q, k, v, hq, hkv, d, q_stride, k_stride,
                      v_stride, scale, dropout_p, out, out_lo, lse, dtype, stream);
}

extern "C" size_t gmlm_attention_causal_d64_workspace_bytes(int64_t b, int64_t hq, int64_t lq) { return attn_delta_bytes(b, hq, lq); }

extern "C" int gmlm_attention_causal_d64_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                             const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq,
                                             int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                             int64_t v_stride, float scale, float dropout_p, void* dq, void* dk, void* dv,
                                             int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                             size_t workspace_bytes, gmlm_stream_t stream) {
  return grouped::bwd(kFamily, "attention_causal_d64_bwd", grouped::padded(kv_len, b, lq, lk), q, k, v, out, out_lo, dout, lse, hq, hkv,
                      d, q_stride, k_stride, v_stride, scale, dropout_p, dq, dk, dv, dq_stride, dk_stride, dv_stride, dtype, workspace,
                      workspace_bytes, stream);
}

extern "C" int gmlm_attention_causal_d64_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                                    int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv,
                                                    int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                                    float dropout_p, void* out, void* out_lo, float* lse, int dtype,
                                                    gmlm_stream_t stream) {
  return grouped::fwd(kFamily, "attention_causal_d64_varlen_fwd", grouped::packed(cu_seqlens, num_seqs, max_len, total_rows), q, k, v, hq,
                      hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, out, out_lo, lse, dtype, stream);
}

extern "C" size_t gmlm_attention_causal_d64_varlen_workspace_bytes(int64_t total_rows, int64_t hq) {
  return attn_delta_bytes(1, hq, total_rows);   // delta [hq, total_rows]
}

extern "C" int gmlm_attention_causal_d64_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                                    const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                                    int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d,
                                                    int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                                    float dropout_p, void* dq, void* dk, void* dv, int64_t dq_stride,
                                                    int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                                    size_t workspace_bytes, gmlm_stream_t stream) {
  return grouped::bwd(kFamily, "attention_causal_d64_varlen_bwd", grouped::packed(cu_seqlens, num_seqs, max_len, total_rows), q, k, v, out,
                      out_lo, dout, lse, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, dq, dk, dv, dq_stride, dk_stride,
                      dv_stride, dtype, workspace, workspace_bytes, stream);
}
