/* gmlm_hip_bidir.h — tenth header of libgmlm_hip.so's C ABI: bidirectional (non-causal) self-attention with grouped KV heads
 * at head dim 64 or 128, the attention of a EuroBERT text encoder (hf:modeling_eurobert.py: the Llama layer without the
 * causal mask).
 *
 * The rotary embedding of such a layer is gmlm_rope_heads_* of gmlm_hip_gqa.h; this header adds the one attention form that
 * neither the bidirectional entry points (one KV head per query head) nor the grouped ones (causal) cover.
 *
 * Conventions: those of gmlm_hip.h, which this header includes for its types and status codes.  Every pointer is a DEVICE
 * pointer owned by the caller; the library never allocates, frees or synchronises and enqueues only on `stream` (nullable);
 * a call returns 0 or a negative GMLM_E* code with a thread-local gmlm_last_error() message; arguments are validated on the
 * host BEFORE any launch; sizes, strides and dtype are checked before a call with nothing to do returns GMLM_OK, and such a
 * call needs no data pointer; "16-byte aligned" pointers are checked (GMLM_EINVAL); a NULL or short workspace is
 * GMLM_EWORKSPACE; re-entrant, thread-safe, and safe to call twice with the same arguments (identical bytes: no atomics).
 */
#ifndef GMLM_HIP_BIDIR_H
#define GMLM_HIP_BIDIR_H

#include "gmlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bidirectional self-attention with grouped KV heads: layout, argument order, checks and workspace of
 * gmlm_attention_causal_d64_* (gmlm_hip_gqa.h) without the causal clause, and with d = 64 or 128 (dispatched on the host).
 * q [b, l, hq, d], k / v [b, l, hkv, d] with per-operand row strides (slices of one fused [q | k | v] buffer are fine), dtype
 * GMLM_F32 or GMLM_BF16; out [b, l, hq * d] contiguous, lse fp32 [b, hq, l].  hq query heads share hkv KV heads
 * (hq % hkv == 0, query head h reads KV head h / (hq / hkv)); query i of sequence b sees the keys of its own sequence that lie
 * below kv_len[b] (int32 [b] or NULL = l), which is clamped into [0, l]; rows at or past kv_len are still computed as queries;
 * a sequence with kv_len 0 gives zeros and lse = -inf (and zero gradients); out_lo (bf16 only, nullable) receives the residual
 * of the output, with which the backward's delta is exact.  _bwd writes dq [.., hq, d], dk / dv [.., hkv, d] with their own
 * row strides; its workspace holds delta [b, hq, l] (gmlm_attention_bidir_gqa_workspace_bytes).
 * Refused (GMLM_EINVAL), in this order: negative sizes or hq, hkv <= 0; d outside {64, 128}; a dtype other than the two; an
 * out_lo that is not the aligned residual of a bf16 output; lq != lk; hq % hkv != 0; dropout_p != 0 (there is no probability
 * dropout in these kernels); scale <= 0; l >= 2^30 or ceil(l / 128) * b * hq >= 2^31 work items (1-D grids); then, unless b or
 * l is 0 (GMLM_OK without a launch), null or misaligned operands, row strides below heads * d, >= 2^24 or not multiples of 8
 * (bf16) / 4 (fp32) elements, and last the workspace (GMLM_EWORKSPACE).  Identical calls give identical bits. */
int gmlm_attention_bidir_gqa_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                 int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                 int64_t v_stride, float scale, float dropout_p, void* out, void* out_lo, float* lse, int dtype,
                                 gmlm_stream_t stream);
size_t gmlm_attention_bidir_gqa_workspace_bytes(int64_t b, int64_t hq, int64_t lq);
int gmlm_attention_bidir_gqa_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo, const void* dout,
                                 const float* lse, const int32_t* kv_len, int64_t b, int64_t hq, int64_t hkv, int64_t lq, int64_t lk,
                                 int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                                 void* dq, void* dk, void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                 void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

/* The packed (varlen) layout: sequence i = rows [cu_seqlens[i], cu_seqlens[i + 1]) (int32 [num_seqs + 1]) of total_rows packed
 * rows, none longer than max_len (> 0); a sequence of length 0 is legal; a query sees every key of its own sequence; lse and
 * the workspace (delta) are [hq, total_rows].  A row owned by no sequence is neither read nor written.  Further refusals: a
 * null cu_seqlens, max_len <= 0, total_rows < 0 or >= 2^30, ceil(max_len / 128) * num_seqs * hq >= 2^31. */
int gmlm_attention_bidir_gqa_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens, int64_t num_seqs,
                                        int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride,
                                        int64_t k_stride, int64_t v_stride, float scale, float dropout_p, void* out, void* out_lo,
                                        float* lse, int dtype, gmlm_stream_t stream);
size_t gmlm_attention_bidir_gqa_varlen_workspace_bytes(int64_t total_rows, int64_t hq);
int gmlm_attention_bidir_gqa_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                        const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                        int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride,
                                        int64_t k_stride, int64_t v_stride, float scale, float dropout_p, void* dq, void* dk,
                                        void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                        void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GMLM_HIP_BIDIR_H */
