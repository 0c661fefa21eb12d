/* gmlm_hip_modernbert.h — sixth header of libgmlm_hip.so's C ABI: the kernels of a ModernBERT text encoder.
 *
 * ModernBERT (hf:modeling_modernbert.py) is a pre-norm encoder: LayerNorm without bias before each branch, a fused Wqkv
 * projection at head dim 64 with the rotate-half rotary embedding and no Q / K norm, GeGLU with the erf GELU, and attention
 * that is bidirectional everywhere but limited to the band |i - j| <= sliding_window in its "sliding_attention" layers.  The
 * entry points below are what the rest of the library lacks for it: residual add + LayerNorm, rotary embedding at d = 64 in
 * place, GeGLU, and band-limited attention at d = 64.  A full-attention layer runs gmlm_attention_fwd / _bwd (gmlm_hip.h).
 *
 * Conventions: those of the decoder section of gmlm_hip.h, which this header includes for its types and status codes.  bf16 or
 * fp32 storage (`dtype`), fp32 arithmetic, ONE rounding on store, 16-byte accesses.  Every pointer is a DEVICE pointer owned
 * by the caller; the library never allocates, frees or synchronises and enqueues only on `stream` (nullable); a call returns 0
 * or a negative GMLM_E* code with a thread-local gmlm_last_error() message; arguments are validated on the host BEFORE any
 * launch, sizes, strides and dtype first: a call with nothing to do then returns GMLM_OK and needs no data pointer; "16-byte
 * aligned" pointers are checked (GMLM_EINVAL); a NULL or short workspace is GMLM_EWORKSPACE.  Every sum across rows runs in
 * a fixed order with no atomics: identical calls give identical bits.
 */
#ifndef GMLM_HIP_MODERNBERT_H
#define GMLM_HIP_MODERNBERT_H

#include "gmlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Residual add + LayerNorm, the LayerNorm sibling of gmlm_add_rmsnorm_*.  a, b, s, y, dy, dres, ds: [rows, f] in `dtype`.
 *   sum = a + b, stored to s (b and s are given together or both NULL: then sum = a and nothing is stored);
 *   y = (sum - mean) * rstd * gamma (+ beta; beta nullable), mean / rstd over the STORED sum (the rounded residual stream is
 *   what every later kernel reads), rstd = 1 / sqrt(var + eps) with the biased variance; mean, rstd: fp32 [rows] outputs.
 * gamma, beta, dgamma, dbeta: fp32 [f].  f is a multiple of 8 (bf16) / 4 (fp32) and at most 4096 (GMLM_ADD_LAYERNORM_MAX_F).
 * rows == 0: GMLM_OK without a launch (the backward still zeroes dgamma / dbeta). */
#define GMLM_ADD_LAYERNORM_MAX_F 4096
int gmlm_add_layernorm_fwd(const void* a, const void* b, const float* gamma, const float* beta, int64_t rows, int64_t f,
                           float eps, void* s, void* y, float* mean, float* rstd, int dtype, gmlm_stream_t stream);
/* ds = dres (nullable: the gradient arriving on the residual stream) + d(sum): the gradient of a AND of b.
 * dgamma[c] = sum_r dy * xhat, dbeta[c] = sum_r dy.  dbeta is nullable; when given, dgamma | dbeta are ONE fp32 [2, f] buffer
 * (dbeta == dgamma + f).  workspace: gmlm_add_layernorm_bwd_workspace_bytes(rows, f). */
size_t gmlm_add_layernorm_bwd_workspace_bytes(int64_t rows, int64_t f);
int gmlm_add_layernorm_bwd(const void* dy, const void* dres, const void* s, const float* gamma, const float* mean,
                           const float* rstd, int64_t rows, int64_t f, void* ds, float* dgamma, float* dbeta, int dtype,
                           void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

/* Rotary embedding at head dim 64, IN PLACE on the first 2 * h * 64 columns (the Q heads, then the K heads) of fused
 * [tokens, >= 3 * h * 64] rows with row stride qkv_stride (elements); the V columns are not touched.  Rotate-half form:
 *   out[i] = x[i] cos[i] - x[i + 32] sin[i],  out[i + 32] = x[i + 32] cos[i] + x[i] sin[i],  i < 32.
 * cos_sin: fp32 [max_len, 2, 32] (cos row, then sin row), built by the caller; there is no device trigonometry.  The position
 * of row t is t % seq_len (pos_ids NULL; padded [b, seq_len] layout, seq_len <= max_len), or pos_ids[t] (int32 [tokens],
 * clamped into [0, max_len); seq_len is not used then).  d must be 64.  gmlm_rope64_bwd applies the inverse rotation in place
 * to the same columns of dqkv: it needs no saved input and no workspace.  tokens == 0: GMLM_OK without a launch. */
int gmlm_rope64_fwd(void* qkv, int64_t qkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len,
                    const int32_t* pos_ids, int64_t h, int64_t d, int dtype, gmlm_stream_t stream);
int gmlm_rope64_bwd(void* dqkv, int64_t dqkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len,
                    const int32_t* pos_ids, int64_t h, int64_t d, int dtype, gmlm_stream_t stream);

/* GeGLU: u = [gate | up] rows of 2 * inter -> y = gelu(gate) * up [rows, inter], gelu = the erf form.  The backward returns
 * the fused [rows, 2 * inter] gradient.  inter is a multiple of 8 (bf16) / 4 (fp32). */
int gmlm_geglu_fwd(const void* u, int64_t rows, int64_t inter, void* y, int dtype, gmlm_stream_t stream);
int gmlm_geglu_bwd(const void* dy, const void* u, int64_t rows, int64_t inter, void* du, int dtype, gmlm_stream_t stream);

/* Band-limited (sliding-window) self-attention at head dim 64: key j is visible to query i of the same sequence iff
 * |i - j| <= window and j lies below the sequence's key count.  Layout as gmlm_attention_fwd / _bwd:
 * padded mode: q, k, v [b, l, h, 64] with row strides (elements) and h * 64 contiguous inside a position (a fused
 *   [.., 3 * h * 64] buffer works without a copy); out / out_lo / dout dense [b, l, h * 64]; lse [b, h, l] fp32 (nullable in
 *   the forward, required by the backward); kv_len int32 [b] (NULL = all l keys; values above l count as l).
 * packed mode: cu_seqlens int32 [b + 1] != NULL, sequence i = rows [cu[i], cu[i + 1]) of [total_rows, h * 64] blocks with
 *   indices local to the sequence; lq = lk = total_rows, max_len > 0 = longest sequence, kv_len NULL, lse [h, total_rows].
 * lq == lk, d == 64, 0 <= window < 2^30, scale > 0; there is no probability dropout: dropout_p must be 0.
 * A query with no visible key (at or past its key count + window, or with a key count of 0) has output 0, lse = -inf and
 * dQ = 0, and adds nothing to dK or dV.  out_lo (bf16 only, optional) as in gmlm_attention_fwd: the forward also stores
 * bf16(O - bf16(O)), and the backward forms delta from out + out_lo.
 * 1-D grids of ceil(rows / 128) * b * h work items (rows = l padded, max_len packed), which must stay below 2^31: no bound
 * on b * h.  The backward is three launches (delta, dQ, dK/dV) with fixed summation orders; its workspace is delta, fp32
 * [b, h, lq] (packed: pass b = 1, lq = total_rows).  b == 0 or lq == 0: GMLM_OK without a launch. */
int gmlm_attention_window_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                              int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                              float scale, float dropout_p, int64_t window, void* out, void* out_lo, float* lse, int dtype,
                              const int32_t* cu_seqlens, int64_t max_len, gmlm_stream_t stream);
size_t gmlm_attention_window_workspace_bytes(int64_t b, int64_t h, int64_t lq);
int gmlm_attention_window_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                              const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t h, int64_t lq,
                              int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                              float dropout_p, int64_t window, void* dq, void* dk, void* dv, int64_t dq_stride,
                              int64_t dk_stride, int64_t dv_stride, int dtype, const int32_t* cu_seqlens, int64_t max_len,
                              void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GMLM_HIP_MODERNBERT_H */
