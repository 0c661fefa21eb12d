// Causal attention with grouped KV heads at head dim 128, forward + backward, gfx950 MFMA (gmlm_attention_causal_d128_*, padded
// and packed): the self-attention of a Qwen3-geometry text encoder (query i sees keys 0..i of its own sequence and, of those,
// the ones below kv_len).  One of the three grouped families of attn_grouped.hpp, which describes the kernels and holds the
// argument checks, the launches and the entry-point bodies: CAUSAL = true at D = 128, at the tiling of attn_d128.hip (DESIGN.md
// section 4 "Qwen3 encoder").  Here: the kernels under their names, the family, the exports.
#include "attn_grouped.hpp"

namespace gmlm {
namespace causal128 {

using grouped::Params, grouped::NW, grouped::NT;
constexpr int D = 128;

template <typename T>
__global__ __launch_bounds__(NT) void fwd_kernel(Params x) {
  const Item it = decode(x.a);
  attn_fwd_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, true, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

// delta = rowsum(dO * O) over rows of [b * l, hq, 128]
template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                    int64_t rows /* b * l * hq */, int64_t lq, int64_t hn, float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);
}

template <typename T>
__global__ __launch_bounds__(NT) void dq_kernel(Params x) {
  const Item it = decode(x.a);
  attn_dq_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, true, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

template <typename T>
__global__ __launch_bounds__(NT) void dkv_kernel(Params x) {
  const CausalKeyTile it = causal_key_tile(x.a, x.group);
  causal_dkv_body<T, D, NW, Cfg<T>::QT, Cfg<T>::DBUF, true>(x.a, x.dout_stride, x.group, it, clamp_kvlen(x.a, it.b, it.l));
}

static const grouped::Family kFamily = {
    {"this entry point takes 128", "causal self-attention", "causal"},
    {{}, {fwd_kernel<bf16_t>, delta_kernel<bf16_t>, dq_kernel<bf16_t>, dkv_kernel<bf16_t>}},
    {{}, {fwd_kernel<float>, delta_kernel<float>, dq_kernel<float>, dkv_kernel<float>}}};

}  // namespace causal128
}  // namespace gmlm

using namespace gmlm;
using gmlm::causal128::kFamily;

extern "C" int gmlm_attention_causal_d128_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b,
                                              int64_t hq, int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride,
                                              int64_t k_stride, int64_t v_stride, float scale, float dropout_p, void* out,
                                              void* out_lo, float* lse, int dtype, gmlm_stream_t stream) {
  return grouped::fwd(kFamily, "attention_causal_d128_fwd", grouped::padded(kv_len, b, lq, lk), q, k, v, hq, hkv, d, q_stride, k_stride,
                      v_stride, scale, dropout_p, out, out_lo, lse, dtype, stream);
}

extern "C" size_t gmlm_attention_causal_d128_workspace_bytes(int64_t b, int64_t hq, int64_t lq) {
  return attn_delta_bytes(b, hq, lq);
}

extern "C" int gmlm_attention_causal_d128_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                              const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq,
                                              int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                              int64_t v_stride, float scale, float dropout_p, void* dq, void* dk, void* dv,
                                              int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                              size_t workspace_bytes, gmlm_stream_t stream) {
  return grouped::bwd(kFamily, "attention_causal_d128_bwd", grouped::padded(kv_len, b, lq, lk), q, k, v, out, out_lo, dout, lse, hq, hkv,
                      d, q_stride, k_stride, v_stride, scale, dropout_p, dq, dk, dv, dq_stride, dk_stride, dv_stride, dtype, workspace,
                      workspace_bytes, stream);
}

extern "C" int gmlm_attention_causal_d128_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                                     int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq,
                                                     int64_t hkv, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                                     float scale, float dropout_p, void* out, void* out_lo, float* lse, int dtype,
                                                     gmlm_stream_t stream) {
  return grouped::fwd(kFamily, "attention_causal_d128_varlen_fwd", grouped::packed(cu_seqlens, num_seqs, max_len, total_rows), q, k, v, hq,
                      hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, out, out_lo, lse, dtype, stream);
}

extern "C" size_t gmlm_attention_causal_d128_varlen_workspace_bytes(int64_t total_rows, int64_t hq) {
  return attn_delta_bytes(1, hq, total_rows);   // delta [hq, total_rows]
}

extern "C" int gmlm_attention_causal_d128_varlen_bwd(const void* q, const void* k, const void* v, const void* out,
                                                     const void* out_lo, const void* dout, const float* lse,
                                                     const int32_t* cu_seqlens, int64_t num_seqs, int64_t max_len,
                                                     int64_t total_rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride,
                                                     int64_t k_stride, int64_t v_stride, float scale, float dropout_p, void* dq,
                                                     void* dk, void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride,
                                                     int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  return grouped::bwd(kFamily, "attention_causal_d128_varlen_bwd", grouped::packed(cu_seqlens, num_seqs, max_len, total_rows), q, k, v, out,
                      out_lo, dout, lse, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, dq, dk, dv, dq_stride, dk_stride,
                      dv_stride, dtype, workspace, workspace_bytes, stream);
}
