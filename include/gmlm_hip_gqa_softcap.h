/* gmlm_hip_gqa_softcap.h — fifteenth header of libgmlm_hip.so's C ABI: self-attention with grouped KV heads at head dim 256 and
 * attention-logit soft-capping, causal or bidirectional, with or without a sliding window, and the rotary embedding on head rows
 * at head dim 256 without a head norm (csrc/attn_gqa_softcap.hip): the attention of a Gemma2 text encoder (hf:modeling_gemma2.py).
 *
 * Conventions: those of gmlm_hip.h, which this header includes for its types and status codes.  Every pointer is a DEVICE
 * pointer owned by the caller; the library never allocates, frees or synchronises and enqueues only on `stream` (nullable);
 * a call returns 0 or a negative GMLM_E* code with a thread-local gmlm_last_error() message; arguments are validated on the
 * host BEFORE any launch; sizes, strides and dtype are checked before a call with nothing to do returns GMLM_OK, and such a
 * call needs no data pointer; "16-byte aligned" pointers are checked (GMLM_EINVAL); a NULL or short workspace is
 * GMLM_EWORKSPACE; re-entrant, thread-safe, and safe to call twice with the same arguments (identical bytes: no atomics).
 */
#ifndef GMLM_HIP_GQA_SOFTCAP_H
#define GMLM_HIP_GQA_SOFTCAP_H

#include "gmlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gmlm_attention_gqa_d256_band_* (gmlm_hip_gqa_band.h: layout, strides, out_lo, alignment, workspace, the empty call, the mask)
 * with `softcap` after `window`.  With c = softcap the score of query i and key j enters the softmax as
 *     z = c * tanh(q_i . k_j * scale / c)
 * and the cap is applied BEFORE the mask, as HF's eager path has it: a masked key has probability exactly 0 whatever its score
 * (a cap applied after the mask would give it the probability of a score of -c).  lse is the log-sum-exp of the capped scores;
 * _bwd carries the factor 1 - tanh^2 into dq and dk.  A score far past the cap gives exactly z = +-c and a factor of exactly 0;
 * no finite score gives a NaN.  `window` = 0 means no band (the mask of gmlm_attention_gqa_d256_*), window in [1, 2^30) the
 * exclusive window of gmlm_attention_gqa_d256_band_*.
 * Refused (GMLM_EINVAL), in this order: the refusals of gmlm_attention_gqa_d256_band_* up to the scale; a window that is neither 0
 * nor in [1, 2^30); l >= 2^30 or too many work items; a softcap that is not finite and > 0; then, unless b or l is 0 (GMLM_OK
 * without a launch), the operand refusals of that family and last the workspace (GMLM_EWORKSPACE), which holds delta [b, hq, l].
 * dropout_p != 0 is refused.  Identical calls give identical bits. */
int gmlm_attention_gqa_d256_softcap_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                     int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                     int64_t v_stride, float scale, float dropout_p, int causal, int64_t window, float softcap, void* out,
                                     void* out_lo, float* lse, int dtype, gmlm_stream_t stream);
size_t gmlm_attention_gqa_d256_softcap_bwd_workspace_bytes(int64_t b, int64_t hq, int64_t lq);
int gmlm_attention_gqa_d256_softcap_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                     const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq, int64_t hkv,
                                     int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                     float scale, float dropout_p, int causal, int64_t window, float softcap, void* dq, void* dk, void* dv,
                                     int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                     size_t workspace_bytes, gmlm_stream_t stream);

/* The packed (varlen) layout of gmlm_attention_gqa_d256_varlen_*: sequence i = rows [cu_seqlens[i], cu_seqlens[i + 1]) of
 * total_rows packed rows, none longer than max_len (> 0); a sequence of length 0 is legal; lse and the workspace (delta) are
 * [hq, total_rows].  The packed refusals (a null cu_seqlens, max_len <= 0, total_rows < 0 or >= 2^30) come first, as there. */
int gmlm_attention_gqa_d256_softcap_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                            int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv,
                                            int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                            float dropout_p, int causal, int64_t window, float softcap, void* out, void* out_lo, float* lse,
                                            int dtype, gmlm_stream_t stream);
size_t gmlm_attention_gqa_d256_softcap_varlen_bwd_workspace_bytes(int64_t total_rows, int64_t hq);
int gmlm_attention_gqa_d256_softcap_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                            const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                            int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d,
                                            int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                                            int causal, int64_t window, float softcap, void* dq, void* dk, void* dv, int64_t dq_stride,
                                            int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                            size_t workspace_bytes, gmlm_stream_t stream);

/* The rotate-half rotary embedding IN PLACE on the first `heads` = hq + hkv head rows of every token row of a fused
 * [q | k | v] buffer at head dim 256: gmlm_rope_heads_* (gmlm_hip_gqa.h: arguments, table layout fp32 [max_len, 2, d / 2],
 * positions by seq_len or pos_ids, refusals and their order) with d required to be 256.  fp32 arithmetic, one rounding;
 * _bwd is the inverse rotation in place on the gradient.  V columns are neither read nor written. */
int gmlm_rope_heads_d256_fwd(void* qkv, int64_t qkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len,
                             const int32_t* pos_ids, int64_t heads, int64_t d, int dtype, gmlm_stream_t stream);
int gmlm_rope_heads_d256_bwd(void* dqkv, int64_t dqkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len,
                             const int32_t* pos_ids, int64_t heads, int64_t d, int dtype, gmlm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GMLM_HIP_GQA_SOFTCAP_H */
