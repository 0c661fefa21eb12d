// Bidirectional (non-causal) self-attention with grouped KV heads at head dim 64 and 128, forward + backward, gfx950 MFMA
// (gmlm_attention_bidir_gqa_*, padded and packed; C ABI in include/gmlm_hip_bidir.h), all in namespace gmlm::bidir: the
// attention of a EuroBERT text encoder (the Llama layer without the causal mask).  One of the three grouped families of
// attn_grouped.hpp, which describes the kernels and holds the argument checks, the launches and the entry-point bodies:
// CAUSAL = false, so the key loop runs over all key tiles below the sequence's kv_len, and a dK/dV workgroup walks ALL query
// tiles of the sequence for each query head of its group (DESIGN.md section 4 "EuroBERT and NomicBERT encoders").  Here: the
// kernels under their names, the family, the exports.
#include "attn_grouped.hpp"
#include "../../include/gmlm_hip_bidir.h"

namespace gmlm {
namespace bidir {

using grouped::Params, grouped::NW, grouped::NT;

template <typename T, int D>
__global__ __launch_bounds__(NT) void gqa_fwd_kernel(Params x) {
  const Item it = decode(x.a);
  attn_fwd_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, false, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

// delta = rowsum(dO * O) over rows of [b * l, hq, D]
template <typename T, int D>
__global__ __launch_bounds__(256) void gqa_delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                        int64_t rows /* b * l * hq */, int64_t lq, int64_t hn,
                                                        float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);
}

template <typename T, int D>
__global__ __launch_bounds__(NT) void gqa_dq_kernel(Params x) {
  const Item it = decode(x.a);
  attn_dq_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, false, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

template <typename T, int D>
__global__ __launch_bounds__(NT) void gqa_dkv_kernel(Params x) {
  const CausalKeyTile it = causal_key_tile(x.a, x.group);
  causal_dkv_body<T, D, NW, Cfg<T>::QT, Cfg<T>::DBUF, false>(x.a, x.dout_stride, x.group, it, clamp_kvlen(x.a, it.b, it.l));
}

static const grouped::Family kFamily = {
    {"this entry point takes 64 or 128", "self-attention", "grouped"},
    {{gqa_fwd_kernel<bf16_t, 64>, gqa_delta_kernel<bf16_t, 64>, gqa_dq_kernel<bf16_t, 64>, gqa_dkv_kernel<bf16_t, 64>},
     {gqa_fwd_kernel<bf16_t, 128>, gqa_delta_kernel<bf16_t, 128>, gqa_dq_kernel<bf16_t, 128>, gqa_dkv_kernel<bf16_t, 128>}},
    {{gqa_fwd_kernel<float, 64>, gqa_delta_kernel<float, 64>, gqa_dq_kernel<float, 64>, gqa_dkv_kernel<float, 64>},
     {gqa_fwd_kernel<float, 128>, gqa_delta_kernel<float, 128>, gqa_dq_kernel<float, 128>, gqa_dkv_kernel<float, 128>}}};

}  // namespace bidir
}  // namespace gmlm

using namespace gmlm;
using gmlm::bidir::kFamily;

extern "C" int gmlm_attention_bidir_gqa_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                            int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                            int64_t v_stride, float scale, float dropout_p, void* out, void* out_lo, float* lse,
                                            int dtype, gmlm_stream_t stream) {
  return grouped::fwd(kFamily, "attention_bidir_gqa_fwd", grouped::padded(kv_len, b, lq, lk), q, k, v, hq, hkv, d, q_stride, k_stride,
                      v_stride, scale, dropout_p, out, out_lo, lse, dtype, stream);
}

extern "C" size_t gmlm_attention_bidir_gqa_workspace_bytes(int64_t b, int64_t hq, int64_t lq) { return attn_delta_bytes(b, hq, lq); }

extern "C" int gmlm_attention_bidir_gqa_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                            const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq,
                                            int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                            int64_t v_stride, float scale, float dropout_p, void* dq, void* dk, void* dv,
                                            int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                            size_t workspace_bytes, gmlm_stream_t stream) {
  return grouped::bwd(kFamily, "attention_bidir_gqa_bwd", grouped::padded(kv_len, b, lq, lk), q, k, v, out, out_lo, dout, lse, hq, hkv,
                      d, q_stride, k_stride, v_stride, scale, dropout_p, dq, dk, dv, dq_stride, dk_stride, dv_stride, dtype, workspace,
                      workspace_bytes, stream);
}

extern "C" int gmlm_attention_bidir_gqa_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                                   int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv,
                                                   int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                                   float dropout_p, void* out, void* out_lo, float* lse, int dtype,
                                                   gmlm_stream_t stream) {
  return grouped::fwd(kFamily, "attention_bidir_gqa_varlen_fwd", grouped::packed(cu_seqlens, num_seqs, max_len, total_rows), q, k, v, hq,
                      hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, out, out_lo, lse, dtype, stream);
}

extern "C" size_t gmlm_attention_bidir_gqa_varlen_workspace_bytes(int64_t total_rows, int64_t hq) {
  return attn_delta_bytes(1, hq, total_rows);   // delta [hq, total_rows]
}

extern "C" int gmlm_attention_bidir_gqa_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                                   const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                                   int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d,
                                                   int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                                   float dropout_p, void* dq, void* dk, void* dv, int64_t dq_stride,
                                                   int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                                   size_t workspace_bytes, gmlm_stream_t stream) {
  return grouped::bwd(kFamily, "attention_bidir_gqa_varlen_bwd", grouped::packed(cu_seqlens, num_seqs, max_len, total_rows), q, k, v, out,
                      out_lo, dout, lse, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, dq, dk, dv, dq_stride, dk_stride,
                      dv_stride, dtype, workspace, workspace_bytes, stream);
}
