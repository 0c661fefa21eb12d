/* gmlm_hip_gqa_wide.h — thirteenth header of libgmlm_hip.so's C ABI: what a Gemma3 text encoder (hf:modeling_gemma3.py,
 * config.model_type "gemma3_text") needs beyond the other decoder-style encoders: self-attention with grouped KV heads at head
 * dim 256, causal or bidirectional (csrc/attn_gqa_wide.hip), and three row kernels (csrc/gemma_kernels.hip): the sandwich
 * RMSNorm pair, the per-head RMSNorm of Q / K with rotary embedding at head dim 256, and the tanh-GELU gated unit.
 *
 * Conventions: those of gmlm_hip.h, which this header includes for its types and status codes.  Every pointer is a DEVICE
 * pointer owned by the caller; the library never allocates, frees or synchronises and enqueues only on `stream` (nullable);
 * a call returns 0 or a negative GMLM_E* code with a thread-local gmlm_last_error() message; arguments are validated on the
 * host BEFORE any launch; sizes, strides and dtype are checked before a call with nothing to do returns GMLM_OK, and such a
 * call needs no data pointer; "16-byte aligned" pointers are checked (GMLM_EINVAL); a NULL or short workspace is
 * GMLM_EWORKSPACE; re-entrant, thread-safe, and safe to call twice with the same arguments (identical bytes: no atomics).
 */
#ifndef GMLM_HIP_GQA_WIDE_H
#define GMLM_HIP_GQA_WIDE_H

#include "gmlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Self-attention with grouped KV heads at head dim 256: layout, argument order, checks and workspace of
 * gmlm_attention_bidir_gqa_* (gmlm_hip_bidir.h) plus `causal` after dropout_p.
 * q [b, l, hq, 256], k / v [b, l, hkv, 256] with per-operand row strides (slices of one fused [q | k | v] buffer are fine), dtype
 * GMLM_F32 or GMLM_BF16; out [b, l, hq * 256] contiguous, lse fp32 [b, hq, l].  hq query heads share hkv KV heads
 * (hq % hkv == 0, query head h reads KV head h / (hq / hkv), any group size); query i of sequence b sees the keys of its own
 * sequence that lie below kv_len[b] (int32 [b] or NULL = l, clamped into [0, l]) and, with causal != 0, at or before i; rows at
 * or past kv_len are still computed as queries; a sequence with kv_len 0 gives zeros and lse = -inf (and zero gradients);
 * `scale` multiplies the scores (Gemma3: query_pre_attn_scalar^-1/2); out_lo (bf16 only, nullable) receives the residual of
 * the output, with which the backward's delta is exact.  _bwd writes dq [.., hq, 256], dk / dv [.., hkv, 256] with their own row
 * strides; its workspace holds delta [b, hq, l] (gmlm_attention_gqa_d256_bwd_workspace_bytes).
 * Refused (GMLM_EINVAL), in this order: negative sizes or hq, hkv <= 0; d != 256; a dtype other than the two; an out_lo that
 * is not the aligned residual of a bf16 output; lq != lk; hq % hkv != 0; dropout_p != 0 (there is no probability dropout in
 * these kernels); scale <= 0; l >= 2^30 or ceil(l / 32) * b * hq >= 2^31 work items (1-D grids); then, unless b or l is 0
 * (GMLM_OK without a launch), null or misaligned operands, row strides below heads * 256, >= 2^24 or not multiples of 8 (bf16)
 * / 4 (fp32) elements, and last the workspace (GMLM_EWORKSPACE).  Identical calls give identical bits. */
int gmlm_attention_gqa_d256_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                int64_t v_stride, float scale, float dropout_p, int causal, void* out, void* out_lo, float* lse,
                                int dtype, gmlm_stream_t stream);
size_t gmlm_attention_gqa_d256_bwd_workspace_bytes(int64_t b, int64_t hq, int64_t lq);
int gmlm_attention_gqa_d256_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo, const void* dout,
                                const float* lse, const int32_t* kv_len, int64_t b, int64_t hq, int64_t hkv, int64_t lq, int64_t lk,
                                int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                                int causal, void* dq, void* dk, void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride,
                                int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

/* The packed (varlen) layout: sequence i = rows [cu_seqlens[i], cu_seqlens[i + 1]) (int32 [num_seqs + 1]) of total_rows packed
 * rows, none longer than max_len (> 0); a sequence of length 0 is legal; a query sees the keys of its own sequence (causal: at
 * or before it); lse and the workspace (delta) are [hq, total_rows].  A row owned by no sequence is neither read nor written.
 * Further refusals: a null cu_seqlens, max_len <= 0, total_rows < 0 or >= 2^30, ceil(max_len / 32) * num_seqs * hq >= 2^31. */
int gmlm_attention_gqa_d256_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens, int64_t num_seqs,
                                       int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride,
                                       int64_t k_stride, int64_t v_stride, float scale, float dropout_p, int causal, void* out,
                                       void* out_lo, float* lse, int dtype, gmlm_stream_t stream);
size_t gmlm_attention_gqa_d256_varlen_bwd_workspace_bytes(int64_t total_rows, int64_t hq);
int gmlm_attention_gqa_d256_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                       const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                       int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride,
                                       int64_t k_stride, int64_t v_stride, float scale, float dropout_p, int causal, void* dq,
                                       void* dk, void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                                       void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

/* Sandwich RMSNorm pair over rows of f elements (f <= 4096, a multiple of 8 (bf16) / 4 (fp32)); s (nullable: no residual), b,
 * s_out, y [rows, f] contiguous in `dtype`, w_post / w_pre fp32 [f], rstd_b / rstd_s fp32 [rows]:
 *   rstd_b = (mean(b^2) + eps)^-1/2;   s_out = s + b * rstd_b * (w_offset + w_post), rounded once to the storage type;
 *   rstd_s = (mean(s_out^2) + eps)^-1/2 of the STORED s_out;   y = s_out * rstd_s * (w_offset + w_pre).
 * All arithmetic in fp32.  _bwd: from dy and ds_in (nullable: the gradient that arrives on s_out from later layers) it writes
 * ds (nullable: the gradient of s, = the whole gradient of s_out), db, and the column sums dw_post | dw_pre, ONE fp32 [2, f]
 * buffer (dw_pre == dw_post + f), summed in a fixed order.  With rows == 0 the backward zero-fills the weight gradients. */
int gmlm_sandwich_rmsnorm_fwd(const void* s, const void* b, const float* w_post, const float* w_pre, int64_t rows, int64_t f,
                              float w_offset, float eps, void* s_out, void* y, float* rstd_b, float* rstd_s, int dtype,
                              gmlm_stream_t stream);
size_t gmlm_sandwich_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t f);
int gmlm_sandwich_rmsnorm_bwd(const void* dy, const void* ds_in, const void* b, const void* s_out, const float* w_post,
                              const float* w_pre, const float* rstd_b, const float* rstd_s, int64_t rows, int64_t f,
                              float w_offset, void* ds, void* db, float* dw_post, float* dw_pre, int dtype, void* workspace,
                              size_t workspace_bytes, gmlm_stream_t stream);

/* gmlm_qknorm_rope_* (gmlm_hip.h) at head dim 256 with the weight offset of Gemma3's RMSNorm: the first hq + hkv head rows of
 * every fused [q | k | v] row are normalised, n = x * (mean(x^2) + eps)^-1/2 * (w_offset + w), and rotated (rotate-half: element
 * i pairs with i + 128) by the cos / sin row of the token's position; cos_sin fp32 [max_len, 2, 128]; rstd fp32 [tokens,
 * hq + hkv].  `out` may be `qkv` itself (out_stride = qkv_stride): the kernel then works in place and the V columns are never
 * written.  The position is row % seq_len, or pos_ids[row] (int32 [tokens], clamped into [0, max_len)) in the _pos_ forms.
 * _bwd runs IN PLACE on the leading (hq + hkv) * 256 columns of dqkv and needs the UN-normalised qkv the forward read;
 * dq_weight | dk_weight are ONE fp32 [2, 256] buffer (dk_weight == dq_weight + 256), block partials summed in a fixed order. */
int gmlm_qknorm_rope_d256_fwd(const void* qkv, int64_t qkv_stride, const float* q_weight, const float* k_weight,
                              const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len, int64_t hq, int64_t hkv,
                              int64_t d, float w_offset, float eps, void* out, int64_t out_stride, float* rstd, int dtype,
                              gmlm_stream_t stream);
int gmlm_qknorm_rope_d256_pos_fwd(const void* qkv, int64_t qkv_stride, const float* q_weight, const float* k_weight,
                                  const float* cos_sin, int64_t max_len, int64_t tokens, const int32_t* pos_ids, int64_t hq,
                                  int64_t hkv, int64_t d, float w_offset, float eps, void* out, int64_t out_stride, float* rstd,
                                  int dtype, gmlm_stream_t stream);
size_t gmlm_qknorm_rope_d256_bwd_workspace_bytes(int64_t tokens, int64_t hq, int64_t hkv, int dtype);
int gmlm_qknorm_rope_d256_bwd(void* dqkv, int64_t dqkv_stride, const void* qkv, int64_t qkv_stride, const float* q_weight,
                              const float* k_weight, const float* cos_sin, int64_t max_len, const float* rstd, int64_t tokens,
                              int64_t seq_len, int64_t hq, int64_t hkv, int64_t d, float w_offset, float* dq_weight,
                              float* dk_weight, int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream);
int gmlm_qknorm_rope_d256_pos_bwd(void* dqkv, int64_t dqkv_stride, const void* qkv, int64_t qkv_stride, const float* q_weight,
                                  const float* k_weight, const float* cos_sin, int64_t max_len, const float* rstd, int64_t tokens,
                                  const int32_t* pos_ids, int64_t hq, int64_t hkv, int64_t d, float w_offset, float* dq_weight,
                                  float* dk_weight, int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

/* Gated unit with the tanh form of GELU (torch "gelu_pytorch_tanh"): gate_up [rows, 2 * inter] = [gate | up] ->
 * y [rows, inter] = gelu_tanh(gate) * up, gelu_tanh(g) = 0.5 g (1 + tanh(sqrt(2 / pi) (g + 0.044715 g^3))); the argument lists
 * of gmlm_swiglu_*.  tanh is formed from exp(-2 |u|) in (0, 1], so a saturated gate gives exactly 0 or g and never a NaN. */
int gmlm_geglu_tanh_fwd(const void* gate_up, int64_t rows, int64_t inter, void* y, int dtype, gmlm_stream_t stream);
int gmlm_geglu_tanh_bwd(const void* dy, const void* gate_up, int64_t rows, int64_t inter, void* dgate_up, int dtype,
                        gmlm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GMLM_HIP_GQA_WIDE_H */
