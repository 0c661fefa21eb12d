/* gmlm_hip_gqa_band.h — fourteenth header of libgmlm_hip.so's C ABI: band-limited (sliding-window) self-attention with grouped
 * KV heads at head dim 256, causal or bidirectional (csrc/attn_gqa_band.hip): the "sliding_attention" layers of a Gemma3 text
 * encoder (hf:modeling_gemma3.py) for sequences that reach past config.sliding_window.
 *
 * Conventions: those of gmlm_hip.h, which this header includes for its types and status codes.  Every pointer is a DEVICE
 * pointer owned by the caller; the library never allocates, frees or synchronises and enqueues only on `stream` (nullable);
 * a call returns 0 or a negative GMLM_E* code with a thread-local gmlm_last_error() message; arguments are validated on the
 * host BEFORE any launch; sizes, strides and dtype are checked before a call with nothing to do returns GMLM_OK, and such a
 * call needs no data pointer; "16-byte aligned" pointers are checked (GMLM_EINVAL); a NULL or short workspace is
 * GMLM_EWORKSPACE; re-entrant, thread-safe, and safe to call twice with the same arguments (identical bytes: no atomics).
 */
#ifndef GMLM_HIP_GQA_BAND_H
#define GMLM_HIP_GQA_BAND_H

#include "gmlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gmlm_attention_gqa_d256_* (gmlm_hip_gqa_wide.h: layout, strides, out_lo, alignment, workspace, the empty call) with `window`
 * after `causal`.  The mask is HF's, with an EXCLUSIVE window: query i of a sequence sees key j of the same sequence iff
 *     j < kv_len  and  (causal != 0 ?  0 <= i - j < window  :  |i - j| < window),      window >= 1
 * where i and j are positions inside the sequence in both layouts (window 1: the query itself; note that ModernBERT's
 * gmlm_attention_window_* count |i - j| <= window).  With window >= l the result is that of gmlm_attention_gqa_d256_*, bit for
 * bit.  Rows at or past kv_len are still computed as queries.  A query with no visible key (padded layout: one at or past
 * kv_len + window - 1; every query when kv_len is 0) gives an output row of zeros and lse = -inf; _bwd gives it dq = 0 and it
 * contributes nothing to dk / dv, and a key at or past kv_len gets dk = dv = 0.  In the packed layout every query sees itself.
 * The work per query tile is O(32 + 2 window) keys (causal: 32 + window) instead of O(l).
 * Refused (GMLM_EINVAL), in this order: negative sizes or hq, hkv <= 0; d != 256; a dtype other than the two; an out_lo that
 * is not the aligned residual of a bf16 output; lq != lk; hq % hkv != 0; dropout_p != 0; scale <= 0; window < 1 or >= 2^30;
 * l >= 2^30 or ceil(l / 32) * b * hq >= 2^31 work items; then, unless b or l is 0 (GMLM_OK without a launch), null or misaligned
 * operands, row strides below heads * 256, >= 2^24 or not multiples of 8 (bf16) / 4 (fp32) elements, and last the workspace
 * (GMLM_EWORKSPACE), which holds delta [b, hq, l].  Identical calls give identical bits. */
int gmlm_attention_gqa_d256_band_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                     int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                     int64_t v_stride, float scale, float dropout_p, int causal, int64_t window, void* out,
                                     void* out_lo, float* lse, int dtype, gmlm_stream_t stream);
size_t gmlm_attention_gqa_d256_band_bwd_workspace_bytes(int64_t b, int64_t hq, int64_t lq);
int gmlm_attention_gqa_d256_band_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                     const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq, int64_t hkv,
                                     int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                     float scale, float dropout_p, int causal, int64_t window, void* dq, void* dk, void* dv,
                                     int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                     size_t workspace_bytes, gmlm_stream_t stream);

/* The packed (varlen) layout of gmlm_attention_gqa_d256_varlen_*: sequence i = rows [cu_seqlens[i], cu_seqlens[i + 1]) of
 * total_rows packed rows, none longer than max_len (> 0); a sequence of length 0 is legal; lse and the workspace (delta) are
 * [hq, total_rows].  The packed refusals (a null cu_seqlens, max_len <= 0, total_rows < 0 or >= 2^30) come first, as there. */
int gmlm_attention_gqa_d256_band_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                            int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv,
                                            int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                            float dropout_p, int causal, int64_t window, void* out, void* out_lo, float* lse,
                                            int dtype, gmlm_stream_t stream);
size_t gmlm_attention_gqa_d256_band_varlen_bwd_workspace_bytes(int64_t total_rows, int64_t hq);
int gmlm_attention_gqa_d256_band_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                            const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                            int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d,
                                            int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                                            int causal, int64_t window, void* dq, void* dk, void* dv, int64_t dq_stride,
                                            int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                            size_t workspace_bytes, gmlm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GMLM_HIP_GQA_BAND_H */
