/* gmlm_hip_gqa.h — ninth header of libgmlm_hip.so's C ABI: Llama-architecture text encoders without the Q / K head norm
 * (Llama, Qwen2 / Qwen2.5, Mistral: hf:modeling_llama.py, modeling_qwen2.py, modeling_mistral.py).
 *
 * Such a layer is the Qwen3 layer of gmlm_hip.h (add + RMSNorm, fused Q|K|V GEMM, rotary embedding, causal attention with
 * grouped KV heads, SwiGLU) without the per-head RMSNorm of Q and K, and mostly at head dim 64.  Two things are added here:
 * the rotate-half rotary embedding in place on the Q and K head rows of a fused [q | k | v] buffer at head dim 64 or 128, and
 * the causal grouped-KV attention of gmlm_attention_causal_d128_* at head dim 64.  Head dim 128 runs gmlm_rope_heads_* and then
 * gmlm_attention_causal_d128_*.
 *
 * Conventions: those of gmlm_hip.h, which this header includes for its types and status codes.  Every pointer is a DEVICE
 * pointer owned by the caller; the library never allocates, frees or synchronises and enqueues only on `stream` (nullable);
 * a call returns 0 or a negative GMLM_E* code with a thread-local gmlm_last_error() message; arguments are validated on the
 * host BEFORE any launch; sizes, strides and dtype are checked before a call with nothing to do returns GMLM_OK, and such a
 * call needs no data pointer; "16-byte aligned" pointers are checked (GMLM_EINVAL); a NULL or short workspace is
 * GMLM_EWORKSPACE; re-entrant, thread-safe, and safe to call twice with the same arguments (identical bytes: no atomics).
 */
#ifndef GMLM_HIP_GQA_H
#define GMLM_HIP_GQA_H

#include "gmlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rotary embedding over head rows, IN PLACE.  qkv: `tokens` rows of qkv_stride elements (16-byte aligned, dtype GMLM_F32 or
 * GMLM_BF16), each beginning with `heads` = hq + hkv head rows of d elements (d = 64 or 128); whatever follows them in the row
 * (the V columns) is neither read nor written.  Head row x of a token at position p becomes, in the rotate-half form,
 *     y[i] = x[i] cos[p, i] - x[i + d/2] sin[p, i],   y[i + d/2] = x[i + d/2] cos[p, i] + x[i] sin[p, i],   0 <= i < d/2,
 * with cos_sin fp32 [max_len, 2, d/2] (cos row, then sin row; 16-byte aligned), built on the host: there is no device
 * trigonometry.  p = t % seq_len for token row t (padded [b, seq_len] layout; seq_len <= max_len), or, when pos_ids (int32
 * [tokens]) is given, pos_ids[t] clamped into [0, max_len) (seq_len is then not used): the contract of gmlm_rope64_fwd.
 * fp32 arithmetic, ONE rounding on store.  _bwd applies the inverse rotation (sin negated) in place on a gradient buffer of
 * the same layout: it needs no saved input and no workspace.
 * Refused (GMLM_EINVAL): a dtype other than the two, d outside {64, 128}, tokens < 0, heads <= 0 or >= 4096, max_len <= 0,
 * seq_len outside [0, max_len] or seq_len == 0 with tokens > 0 (without pos_ids), qkv_stride below heads * d or not a multiple
 * of 8 (bf16) / 4 (fp32) elements, 2^34 or more head rows; then, unless tokens == 0 (GMLM_OK without a launch), a null or
 * misaligned qkv or table. */
int gmlm_rope_heads_fwd(void* qkv, int64_t qkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len,
                        const int32_t* pos_ids, int64_t heads, int64_t d, int dtype, gmlm_stream_t stream);
int gmlm_rope_heads_bwd(void* dqkv, int64_t dqkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len,
                        const int32_t* pos_ids, int64_t heads, int64_t d, int dtype, gmlm_stream_t stream);

/* Causal self-attention with grouped KV heads at head dim 64: layout, semantics, argument order, checks and workspace of
 * gmlm_attention_causal_d128_* (gmlm_hip.h) with d required to be 64.  hq query heads share hkv KV heads (hq % hkv == 0);
 * query i sees the keys <= i of its own sequence that lie below kv_len[b], which is clamped into [0, l]; a sequence with
 * kv_len 0 gives zeros and lse = -inf; out_lo (bf16) is the residual of the output, with which the backward's delta is exact;
 * dropout_p must be 0; lq == lk; row strides >= heads * 64, multiples of 8 (bf16) / 4 (fp32) elements; 1-D grids of
 * ceil(l / 128) * b * hq work items, which must stay below 2^31.  Identical calls give identical bits. */
int gmlm_attention_causal_d64_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                  int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                  int64_t v_stride, float scale, float dropout_p, void* out, void* out_lo, float* lse, int dtype,
                                  gmlm_stream_t stream);
size_t gmlm_attention_causal_d64_workspace_bytes(int64_t b, int64_t hq, int64_t lq);
int gmlm_attention_causal_d64_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo, const void* dout,
                                  const float* lse, const int32_t* kv_len, int64_t b, int64_t hq, int64_t hkv, int64_t lq, int64_t lk,
                                  int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                                  void* dq, void* dk, void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                  void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

/* The packed (varlen) layout of gmlm_attention_causal_d128_varlen_*: sequence i = rows [cu_seqlens[i], cu_seqlens[i + 1]) of
 * total_rows packed rows, none longer than max_len; lse and the workspace (delta) are [hq, total_rows].  A row owned by no
 * sequence is neither read nor written. */
int gmlm_attention_causal_d64_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens, int64_t num_seqs,
                                         int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride,
                                         int64_t k_stride, int64_t v_stride, float scale, float dropout_p, void* out, void* out_lo,
                                         float* lse, int dtype, gmlm_stream_t stream);
size_t gmlm_attention_causal_d64_varlen_workspace_bytes(int64_t total_rows, int64_t hq);
int gmlm_attention_causal_d64_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                         const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                         int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride,
                                         int64_t k_stride, int64_t v_stride, float scale, float dropout_p, void* dq, void* dk,
                                         void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                         void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GMLM_HIP_GQA_H */
