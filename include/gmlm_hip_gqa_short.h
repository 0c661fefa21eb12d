/* gmlm_hip_gqa_short.h — eleventh header of libgmlm_hip.so's C ABI: LDS-resident short-sequence self-attention with grouped KV
 * heads at head dim 64, bidirectional or causal, for packed batches of sequences of at most 128 tokens: the attention of the
 * Llama / Qwen2 / Mistral encoders (gmlm_attention_causal_d64_varlen_* of gmlm_hip_gqa.h) and of EuroBERT
 * (gmlm_attention_bidir_gqa_varlen_* of gmlm_hip_bidir.h) in the form gmlm_attention_fwd / _bwd of gmlm_hip.h take with
 * seq_groups: several consecutive sequences per work item, one launch forward and one backward, no delta pass.
 *
 * Conventions: those of gmlm_hip.h, which this header includes for its types and status codes.  Every pointer is a DEVICE
 * pointer owned by the caller; the library never allocates, frees or synchronises and enqueues only on `stream` (nullable);
 * a call returns 0 or a negative GMLM_E* code with a thread-local gmlm_last_error() message; arguments are validated on the
 * host BEFORE any launch; sizes, strides and dtype are checked before a call with nothing to do returns GMLM_OK, and such a
 * call needs no data pointer; "16-byte aligned" pointers are checked (GMLM_EINVAL); re-entrant, thread-safe, and safe to call
 * twice with the same arguments (identical bytes: no atomics).  These two entry points take no workspace.
 */
#ifndef GMLM_HIP_GQA_SHORT_H
#define GMLM_HIP_GQA_SHORT_H

#include "gmlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Layout of gmlm_attention_bidir_gqa_varlen_*: q [T, hq, d], k / v [T, hkv, d] with per-operand row strides (slices of one
 * fused [q | k | v] buffer are fine), dtype GMLM_BF16; out [T, hq * d] contiguous, lse fp32 [hq, T], T = total_rows.  Sequence
 * i = rows [cu_seqlens[i], cu_seqlens[i + 1]) (int32 [num_seqs + 1]), none longer than max_len; hq query heads share hkv KV
 * heads (query head h reads KV head h / (hq / hkv)).  seq_groups (int32 [num_groups + 1], as in gmlm_hip.h): work item g =
 * sequences [seq_groups[g], seq_groups[g + 1]): at most 13 sequences and at most 128 rows, which the caller guarantees
 * (ops.pack_sequence_groups) and the kernels clamp: rows and sequences past either bound are left out, never indexed.
 * A query sees the keys of its own sequence, or with causal = 1 those at or before its own position.  A sequence of length 0
 * is legal, inside a group and as a whole group; a row owned by no sequence of any group is neither read nor written.
 * _bwd reads q, k, v, dout [T, hq * d] and lse, and writes dq [T, hq, d], dk / dv [T, hkv, d] with their own row strides; it
 * forms delta itself, in fp32 from the probabilities it uses, so it takes neither out, out_lo nor a workspace.  dk / dv are a
 * fixed-order sum over (query head, query row) in registers: no atomics.
 * Identical calls give identical bits.  The same batch grouped differently agrees to rounding, not to bits: the grouping
 * decides which 32-row blocks a row's sums run over and in which order.
 * Refused (GMLM_EINVAL), in this order: num_seqs < 0 or hq, hkv <= 0; d != 64; a dtype other than GMLM_BF16; hq % hkv != 0;
 * dropout_p != 0 (there is no probability dropout in these kernels); scale <= 0; causal outside {0, 1}; a null cu_seqlens; a
 * null seq_groups; num_groups < 0; max_len <= 0 or > 128; total_rows < 0 or >= 2^30; num_groups * hq >= 2^31 work items (1-D
 * grids); then, unless num_groups, num_seqs or total_rows is 0 (GMLM_OK without a launch), null or misaligned operands and row
 * strides below heads * d, >= 2^24 or not multiples of 8 elements; then out and lse (_fwd) or dout and lse (_bwd). */
int gmlm_attention_gqa_short_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens, int64_t num_seqs,
                                 int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride,
                                 int64_t k_stride, int64_t v_stride, float scale, float dropout_p, int causal,
                                 const int32_t* seq_groups, int64_t num_groups, void* out, float* lse, int dtype,
                                 gmlm_stream_t stream);
int gmlm_attention_gqa_short_bwd(const void* q, const void* k, const void* v, const void* dout, const float* lse,
                                 const int32_t* cu_seqlens, int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq,
                                 int64_t hkv, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                 float dropout_p, int causal, const int32_t* seq_groups, int64_t num_groups, void* dq, void* dk,
                                 void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                 gmlm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GMLM_HIP_GQA_SHORT_H */
