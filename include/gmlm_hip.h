/* gmlm_hip.h — C ABI of libgmlm_hip.so: the MI355X (gfx950) kernels behind the GraphTextLM hot path.
 *
 * The reference (chungimungi/GMLM, main.py) has no FFI layer: its hot path is the Python
 * nn.Module surface GraphTextLM.forward / get_graph_embeddings (main.py:250, 322) calling into
 * PyTorch-Geometric and HuggingFace operators.  This header is the boundary a drop-in for that
 * path binds to (ctypes stub: INTEGRATION.md).  Each entry cites the reference interface it
 * replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch tensors); the library never
 *    allocates or frees device memory, never synchronises the device, and enqueues only on `stream`
 *    (a hipStream_t passed as void*; NULL = the null stream);
 *  - every call returns 0 on success or a negative GMLM_E* code; gmlm_last_error() then returns a
 *    thread-local message; arguments are validated on the host BEFORE any launch;
 *  - a pointer may be NULL only where its entry says so ("nullable", "optional", "NULL = ...", or required under a stated
 *    condition); `stream` and every `seed_dev` are nullable everywhere.  Sizes, strides and dtype are checked before a call
 *    with nothing to do returns GMLM_OK, and such a call needs no data pointer, except an output that it has to fill with
 *    zeros (deg, rel_count, rowptr, s1 / s2, gs, dtoken, dgamma / dbeta / dbias, dw, dq_weight) and the cu_seqlens of the
 *    causal varlen entries;
 *  - workspaces: an entry point with a `workspace` has a `*_workspace_bytes` companion that takes the same sizes.  A NULL
 *    workspace or fewer bytes than the companion returns is GMLM_EWORKSPACE, every other refusal is GMLM_EINVAL; the
 *    companion of an empty problem still returns a positive size (gmlm_wgrad_bf16 has no empty problem: below t = 32 its
 *    companion returns 0 and the call is refused).  No workspace needs initialising;
 *  - alignment: "16-byte aligned" pointers are checked (GMLM_EINVAL); a pointer without that remark is read and written
 *    with scalar accesses and needs only the alignment of its element type;
 *  - tensors are row-major and dense unless a stride argument says otherwise (strides in elements);
 *  - dtype: GMLM_F32 or GMLM_BF16 selects the storage type of activations; accumulation and all
 *    statistics are fp32; index arrays are int32 unless the reference hands over int64 (edge_index);
 *  - re-entrant and thread-safe: the only state kept is a write-once "kernel attributes set on device d" bit per
 *    kernel family, taken under a lock (one process may drive several GPUs / call from several host threads);
 *    safe to call twice with the same arguments (torch.utils.checkpoint recompute, main.py:278-314).
 */
#ifndef GMLM_HIP_H
#define GMLM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMLM_ABI_VERSION 1

enum gmlm_dtype { GMLM_F32 = 0, GMLM_BF16 = 1 };
enum gmlm_status {
  GMLM_OK = 0,
  GMLM_EINVAL = -1,    /* bad argument (null pointer, size, alignment, unsupported shape) */
  GMLM_EWORKSPACE = -2,/* workspace too small */
  GMLM_ELAUNCH = -3,   /* hip launch / runtime error */
  GMLM_EDEVICE = -4    /* not a gfx950 device */
};

typedef void* gmlm_stream_t;

int gmlm_version(void);
const char* gmlm_last_error(void);
/* Fills CU count / wavefront size / arch name of the current device; GMLM_EDEVICE unless gfx950. */
int gmlm_device_check(int* cu_count, int* wave_size, char* arch, int arch_len);

/* ---------------------------------------------------------------------------------------------
 * K1  graph preprocessing (integer, bit-exact)
 * replaces: torch_geometric.utils.degree (main.py:65, 256), the per-edge Python bucketing loop
 *           (main.py:257-267) and RGCNConv's per-relation masked_edge_index compaction
 *           (PyG RGCNConv.forward, call sites main.py:272-308).
 * ------------------------------------------------------------------------------------------- */
/* deg[v] = #{e : index[e] == v}; deg is zeroed by the call.  index values must be in [0, n).
 * K1 pointers are required whenever the array they name has an element (index when e > 0, deg when n > 0, ...); all
 * accesses are scalar. */
int gmlm_degree_i32(const int64_t* index, int64_t e, int64_t n, int32_t* deg, gmlm_stream_t stream);
/* PyG `degree` drop-in: float32 counts. */
int gmlm_degree_f32(const int64_t* index, int64_t e, int64_t n, float* deg, gmlm_stream_t stream);
/* edge_type[e] = 0 if deg[src[e]] <= 2, 1 if <= 5, 2 if <= 10, else 3   (main.py:260-267).  deg has n entries; a
 * source id outside [0, n) is typed 0 here (no out-of-bounds read) and rejected by gmlm_segment_sort's checks. */
int gmlm_edge_bucket(const int64_t* src, const int32_t* deg, int64_t e, int64_t n, int64_t* edge_type,
                     gmlm_stream_t stream);
/* rel_count[r] = #{e : edge_type[e] == r}, r < num_relations in [1, 64] (zeroed by the call, also when e = 0). */
int gmlm_relation_histogram(const int64_t* edge_type, int64_t e, int num_relations, int32_t* rel_count,
                            gmlm_stream_t stream);

/* Stable segment sort.  key[e] = node[e] * r_active + (rel ? rel_remap[rel[e]] : 0).
 * rel is nullable (then rel_remap is unused; given, it requires rel_remap).  node and perm are required when e > 0; rowptr
 * and bad_flag (zeroed by the call) always: e = 0 still fills rowptr with zeros.
 * Outputs: keys[e] (unsorted int32 keys, nullable), perm[t] = original id of the t-th edge in
 * (key, original id) order, rowptr[s] = first t with sorted key >= s, s in [0, num_segments].
 * Edges whose relation maps to a negative remap entry are an error (GMLM_EINVAL is reported by
 * the caller-side check; the kernel clamps them to segment 0 and sets *bad_flag != 0). */
size_t gmlm_segment_sort_workspace_bytes(int64_t e);
int gmlm_segment_sort(const int64_t* node, const int64_t* rel, const int32_t* rel_remap, int r_active, int64_t e,
                      int64_t num_segments, int32_t* keys, int32_t* perm, int32_t* rowptr, int32_t* bad_flag,
                      void* workspace, size_t workspace_bytes, gmlm_stream_t stream);
/* out[t] = (int32) src[perm[t]] (int64 source) / out[t] = src[perm[t]] (int32 source) */
int gmlm_gather_i64_to_i32(const int64_t* src, const int32_t* perm, int64_t e, int32_t* out, gmlm_stream_t stream);
int gmlm_gather_i32(const int32_t* src, const int32_t* perm, int64_t e, int32_t* out, gmlm_stream_t stream);
/* inv_cnt[s] = 1 / max(rowptr[s+1] - rowptr[s], 1) */
int gmlm_segment_inv_count(const int32_t* rowptr, int64_t num_segments, float* inv_cnt, gmlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K2/K3  relation-segmented CSR mean aggregation (the "SpMM") and its transpose
 * replaces: RGCNConv.propagate(aggr='mean') = gather x[src] + scatter-mean to dst per relation
 *           (PyG; call sites main.py:272, 285, 298, 308) and its autograd backward.
 *
 * out[s, :] = scale_s * sum_{t in [rowptr[s], rowptr[s+1])} w_t * src[idx[t], :]
 *   forward : src = x [n, f],           idx = col (source node of each sorted edge),
 *             scale_s = 1/len(s) (mean != 0), w_t = 1 (edge_w == NULL); out = H viewed [n*r_active, f]
 *   backward: src = dH viewed [n*r_active, f], idx = tseg (segment of each source-sorted edge),
 *             scale_s = 1, w_t = edge_w[idx[t]] = inv_cnt[segment];      out = dX [n, f]
 * Rows of src/out are `*_stride` elements apart.  Deterministic: fixed summation order, no atomics.
 * f % (16 / sizeof(dtype)) == 0 with 16-byte aligned rows takes the vector path; anything else
 * the scalar path.
 *
 * Skewed (power-law) graphs: segments longer than `long_threshold` edges are cut into chunks of that
 * many edges, each chunk is reduced by its own lane group into `partial` (fp32 [n_chunks, f]) and a third
 * kernel adds the partials of a segment in chunk order (still deterministic).  The plan arrays
 * (`long_seg` [n_long], `chunk_ptr` [n_long+1], `chunk_owner` [n_chunks]) are index data built once per
 * graph by the caller (or on the device: gmlm_split_plan_build, entries of -1 = unused slot); pass long_threshold = 0 /
 * n_long = 0 for no splitting.
 * src is required when src_rows > 0, idx when a segment has an edge (the caller's rowptr decides; not checkable on the
 * host), edge_w is nullable (w_t = 1), the four plan arrays are required exactly when long_threshold > 0 and n_long > 0.
 * ------------------------------------------------------------------------------------------- */
/* Split plan built on the device, for segment sets that change every step (the embedding-gradient segment sums: token /
 * position ids of the step's batch; replaces the scatter-add of hf BertEmbeddings' backward).  Arrays have CAPACITY size -
 * long_seg [cap_long], chunk_ptr [cap_long + 1], chunk_owner [cap_chunks], partial [cap_chunks, f] - from
 * gmlm_split_plan_capacity(num_items = rowptr[num_segments], long_threshold); unused slots hold -1 and are skipped by
 * gmlm_rgcn_mean_spmm, which is then called with n_long = cap_long, n_chunks = cap_chunks.  One launch, no host round trip,
 * deterministic. */
int gmlm_split_plan_capacity(int64_t num_items, int64_t long_threshold, int64_t* cap_long, int64_t* cap_chunks);
int gmlm_split_plan_build(const int32_t* rowptr, int64_t num_segments, int64_t num_items, int64_t long_threshold,
                          int32_t* long_seg, int32_t* chunk_ptr, int32_t* chunk_owner, gmlm_stream_t stream);

int gmlm_rgcn_mean_spmm(const void* src, int64_t src_rows, int64_t src_stride, const int32_t* rowptr,
                        const int32_t* idx, const float* edge_w, int mean, int64_t num_segments, int64_t f,
                        void* out, int64_t out_stride, int dtype, int64_t long_threshold, const int32_t* long_seg,
                        const int32_t* chunk_ptr, const int32_t* chunk_owner, int64_t n_long, int64_t n_chunks,
                        float* partial, gmlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K10  RGCN basis composition and its backward (PyG RGCNConv with num_bases; ctor sites main.py:189-203)
 *   W[r, :] = sum_b comp[r, b] * weight[b, :]     comp [r_active, num_bases] (rows of the relations that occur),
 *   weight [num_bases, cols = in*out], W [r_active, cols]; all fp32 (master parameters).
 *   backward (one pass): dweight[b, :] = sum_r comp[r, b] * dW[r, :],  dcomp[r, b] = <dW[r, :], weight[b, :]>.
 * r_active <= 5, num_bases <= 32, cols % 4 == 0.  Deterministic (fixed-order reductions).
 * weight, w, dw and dweight are 16-byte aligned (vector accesses); comp and dcomp are scalar.  No pointer is nullable.
 * ------------------------------------------------------------------------------------------- */
int gmlm_basis_compose_fwd(const float* comp, const float* weight, int r_active, int num_bases, int64_t cols,
                           float* w, gmlm_stream_t stream);
size_t gmlm_basis_compose_bwd_workspace_bytes(int r_active, int num_bases, int64_t cols);
int gmlm_basis_compose_bwd(const float* comp, const float* weight, const float* dw, int r_active, int num_bases,
                           int64_t cols, float* dweight, float* dcomp, void* workspace, size_t workspace_bytes,
                           gmlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K4  GraphNorm (+ exact-erf GELU + dropout) forward / backward, single graph (batch = all rows)
 * replaces: torch_geometric.nn.GraphNorm.forward -> F.gelu -> nn.Dropout (main.py:273-275 ...)
 * ------------------------------------------------------------------------------------------- */
/* Column statistics of x [n, f] (`dtype`): s1[c] = sum_i (x[i,c] - shift[c]), s2[c] = sum_i (x[i,c]-shift[c])^2
 * (fp32).  shift may be NULL (= 0).  workspace: gmlm_colstats_workspace_bytes(n, f).  s1 and s2 are the two rows of ONE
 * [2, f] buffer (s2 == s1 + f); n = 0 fills them with zeros.  All K4 accesses are scalar: no alignment rule.
 * In all K4 entries x, y, g and dx share ONE storage dtype (the GEMM output feeds the norm directly). */
size_t gmlm_colstats_workspace_bytes(int64_t n, int64_t f);
int gmlm_colstats(const void* x, int dtype, const float* shift, int64_t n, int64_t f, float* s1, float* s2,
                  void* workspace, size_t workspace_bytes, gmlm_stream_t stream);
/* mean[c], rstd[c] from (s1, s2, shift) over n_total rows:  mu = shift + s1/n; o = x - mu*ms;
 * var = E[o^2]; rstd = 1/sqrt(var + eps).  shift is nullable (= 0), as in gmlm_colstats. */
int gmlm_graphnorm_finalize(const float* s1, const float* s2, const float* shift, const float* mean_scale,
                            int64_t n_total, int64_t f, float eps, float* mean, float* rstd, gmlm_stream_t stream);
/* y = dropout(gelu(weight * (x - mean*ms) * rstd + bias)); y stored as `dtype`; act != 0 applies GELU.
 * dropout: keep-probability scaling 1/(1-p), mask = hash(seed, element index) (replayable); dropout_p in [0, 1), checked
 * alike by the forward and both backward passes, which must draw the same mask.
 * Every entry with a `seed` also takes `seed_dev`: NULL, or a device pointer to one uint64 that the kernel ADDS to `seed`
 * when it runs.  A captured hipGraph replays its arguments unchanged; pointing seed_dev at a counter that the graph itself
 * increments gives every replay fresh masks while forward / recompute / backward of one replay still agree. */
int gmlm_graphnorm_apply(const void* x, const float* mean, const float* rstd, const float* weight,
                         const float* bias, const float* mean_scale, int64_t n, int64_t f, int act,
                         float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* y, int dtype, gmlm_stream_t stream);
/* backward, pass 1: column sums needed by the closed form.  g = dL/dy (dtype), x = saved pre-norm input.
 * gs[0,c] = sum_i gz[i,c], gs[1,c] = sum_i gz[i,c] * ohat[i,c]   (gz = g through dropout and GELU)
 * workspace: gmlm_colstats_workspace_bytes(n, f) (the same two-row column reduction); n = 0 fills gs with zeros. */
int gmlm_graphnorm_bwd_stats(const void* g, int dtype, const void* x, const float* mean, const float* rstd,
                             const float* weight, const float* bias, const float* mean_scale, int64_t n, int64_t f,
                             int act, float dropout_p, uint64_t seed, const uint64_t* seed_dev, float* gs /* [2, f] */,
                             void* workspace, size_t workspace_bytes, gmlm_stream_t stream);
/* backward, pass 2: dx (`dtype`) and parameter grads from the (all-reduced) column sums over n_total rows.
 * dweight, dbias and dmean_scale (fp32 [f]) are each nullable: a NULL one is not written.  They are written even when
 * n = 0 (a rank without rows still holds the all-reduced sums), so the parameters and gs are required then too. */
int gmlm_graphnorm_bwd_apply(const void* g, int dtype, const void* x, const float* mean, const float* rstd,
                             const float* weight, const float* bias, const float* mean_scale, const float* gs,
                             int64_t n, int64_t n_total, int64_t f, int act, float dropout_p, uint64_t seed, const uint64_t* seed_dev,
                             void* dx, float* dweight, float* dbias, float* dmean_scale, gmlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K6  fused bias + dropout + residual + LayerNorm (+ GELU) forward / backward (row-wise)
 * replaces: BertSelfOutput / BertOutput dense-epilogue (hf:modeling_bert.py:289-293, 347-351),
 *           BertEmbeddings LayerNorm (hf:...:105), MultiScaleFusion.layer_norm (main.py:180),
 *           fusion_network LayerNorm+GELU (main.py:238-239).
 * z = dropout(x + bias) + residual;  y = act(LN(z) * gamma + beta)
 * f: a multiple of 8 (bf16) / 4 (fp32), at most 1024.  x, y, dy, dx, residual, dresidual (`dtype`) and bias, gamma, beta
 * (fp32 [f]) are 16-byte aligned: all are read and written 16 bytes at a time.  bias and residual are nullable (absent
 * term), in the backward dresidual too (not written).  mean / rstd (fp32 [rows]) are nullable outputs of the forward (not
 * stored) and required inputs of the backward.
 * ------------------------------------------------------------------------------------------- */
int gmlm_bias_res_layernorm_fwd(const void* x, const float* bias, const void* residual, const float* gamma,
                                const float* beta, int64_t rows, int64_t f, float eps, int act, float dropout_p,
                                uint64_t seed, const uint64_t* seed_dev, void* y, float* mean, float* rstd, int dtype, gmlm_stream_t stream);
/* dz (written to dx; the residual branch receives the same dz; dbias = column sum of dx through dropout)
 * partial parameter grads are reduced inside: dgamma/dbeta/dbias [f] fp32, each nullable (a NULL one is not written);
 * rows = 0 fills the given ones with zeros.  workspace: gmlm_layernorm_bwd_workspace_bytes(rows, f). */
size_t gmlm_layernorm_bwd_workspace_bytes(int64_t rows, int64_t f);
int gmlm_bias_res_layernorm_bwd(const void* dy, const void* x, const float* bias, const void* residual,
                                const float* gamma, const float* beta, const float* mean, const float* rstd,
                                int64_t rows, int64_t f, int act, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* dx,
                                void* dresidual, float* dgamma, float* dbeta, float* dbias, int dtype,
                                void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K5/K7  multi-head attention core, streaming softmax (flash style), forward / backward
 * replaces: K5 BertSelfAttention's attention_interface call softmax(QK^T*scale + padmask)V
 *           (hf:modeling_bert.py:188-201, eager form 111-136) with a per-sequence key length;
 *           K7 CrossAttention.forward's dense [1,8,N,N] softmax (main.py:159-163), no mask.
 * Layout: q [b, lq, h, d], k/v [b, lk, h, d] with row strides (elements) *_stride between
 * consecutive positions and h*d contiguous inside a position (so a fused [.., 3*h*d] QKV buffer
 * works without a copy); out [b, lq, h, d] dense; lse [b, h, lq] fp32 (log-sum-exp of scaled scores; nullable in the
 * forward = not stored, every forward kernel skips the store; required by the backward).
 * q, k, v, out, out_lo, dout, dq, dk, dv are 16-byte aligned and every row stride is a multiple of 8 (bf16) / 4 (fp32)
 * elements, at least h*d and below 2^24.  b*h <= 65535, scale > 0, dropout_p in [0, 1) (forward and backward alike).
 * k and v are required when lk > 0.
 * Order of the checks, here and in every other attention entry point (d128, d32, wide, causal): sizes, head dim, dtype, out_lo,
 * layout (packed mode, seq_groups, lq == lk, GQA divisibility), dropout_p, scale, the work-item bound; then a call with nothing
 * to do returns GMLM_OK; then the operands, the outputs and last the workspace.  The first failed check decides code and message.
 * kv_len: int32 [b] valid key count per sequence (NULL = all lk keys valid); keys >= kv_len[b]
 * are masked out exactly like the additive -inf padding mask of create_bidirectional_mask.
 * d in {64, 96}.  MFMA: bf16 32x32x16 for GMLM_BF16, f32 32x32x2 for GMLM_F32.
 * Packed (variable-length) mode: cu_seqlens int32 [b+1] != NULL.  q, k, v, out are then [total_rows, h*d]
 * row blocks with sequence i owning rows [cu[i], cu[i+1]) of ALL of them (self-attention), lq = lk =
 * total_rows, max_len = longest sequence, kv_len = NULL, lse is [h, total_rows].  No padded token is ever
 * computed: this is how the text encoder runs (one packed batch of all active nodes).
 * dropout_p > 0 drops attention probabilities (after normalisation, scaled by 1/(1-p)) exactly like
 * nn.Dropout on `attn` in main.py:161 / hf eager attention; the mask is hash(seed, (b,h,q,key)) and
 * is regenerated, not stored, by the backward pass when given the same seed.
 * Short sequences: bf16, d = 64, every sequence <= 128 rows (lq, lk <= 128, or max_len <= 128 in packed mode) and
 * b*h >= 512 runs with Q / K / V (/ dO) of a work item resident in LDS; the backward - selected only when out_lo is NULL -
 * is ONE launch (delta + dQ + dK/dV) that forms delta = sum_k P dP from its own fp32 P, dP (it does not read `out`);
 * everything else runs the streaming forward and three backward launches (delta = rowsum(dO * O), dQ, dK/dV).
 * Foreign lse / out (ring blocks, ops.AttentionBlock): on every backward path that forms delta from `out`, lse and out need
 * not be this call's own forward's.  lse may be any value >= the log-sum-exp of the keys given and out (+ out_lo) the output
 * of ALL keys, of which k / v are a part: P = exp(S - lse) is then the global softmax restricted to these keys, and dq / dk /
 * dv are their share of the gradients.  The short-sequence backward sums delta over its own keys and therefore ASSUMES its own
 * lse; with another it returns finite, wrong dq / dk.  A caller with a foreign lse passes out_lo (bf16), which keeps the call
 * on the streaming kernels at any shape; in fp32 no short-sequence path exists.
 * seq_groups (packed mode, optional; int32 [num_groups + 1], device): work item g of the short-sequence kernels is the run
 * of sequences [seq_groups[g], seq_groups[g+1]) - at most 13 sequences and 128 rows in total (the caller guarantees both;
 * rows past 128 would be ignored) - attended block-diagonally.  Ignored by the streaming kernels.  With dropout, a work
 * item draws ONE mask for its whole row range: slab h_index * total_rows + cu[seq_groups[g]] and query / key indices counted
 * from the group's first row, where the ungrouped packed mode uses cu[seq] and indices local to each sequence.  Forward and
 * backward agree as long as both get the same groups; the same batch grouped differently draws a different (equally
 * distributed) mask.  This is intended: the group is the kernels' unit of work.
 * kv_len[b] = 0: zero output, lse = -inf, zero dQ / dK / dV for that sequence; kv_len[b] > lk counts as lk.
 * A sequence with ONE valid key has exact dK = 0; in bf16 the forward rounds P to bf16 but normalises by the unrounded sum,
 * so O = V (1 +- 2^-9) and dK of that key is rounding noise of that size (summed over the queries), not exactly 0.
 * out_lo (bf16 only, optional): the forward also stores lo = bf16(O - bf16(O)); handed to the backward, delta is formed
 * from out + out_lo, i.e. with fp32-like accuracy.  With `out` alone delta carries the 2^-9 rounding of the stored
 * output, which does NOT cancel in dS = P (dP - delta) and dominates the query / key gradients whenever those are small
 * against |dO||O| (deep encoder layers).  The short-sequence kernels neither write nor need it; handing it
 * to the backward at a short-sequence shape selects the streaming kernels (above), so dbias is then refused.
 * ------------------------------------------------------------------------------------------- */
int gmlm_attention_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                       int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                       float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* out, void* out_lo, float* lse,
                       int dtype, const int32_t* cu_seqlens, int64_t max_len, const int32_t* seq_groups, int64_t num_groups,
                       gmlm_stream_t stream);
/* packed mode: pass b = 1 (delta is [h, total_rows]).  The workspace is required on every path. */
size_t gmlm_attention_bwd_workspace_bytes(int64_t b, int64_t h, int64_t lq, int64_t lk, int64_t d);
int gmlm_attention_bwd(const void* q, const void* k, const void* v, const void* out, const void* dout,
                       const float* lse, const int32_t* kv_len, int64_t b, int64_t h, int64_t lq, int64_t lk,
                       int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                       float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* dq, void* dk, void* dv, int64_t dq_stride,
                       int64_t dk_stride, int64_t dv_stride, int dtype, const int32_t* cu_seqlens, int64_t max_len,
                       void* workspace, size_t workspace_bytes,
                       float* dbias_partial /* [b or num_groups, 3*h*d] scratch */, float* dbias /* [3*h*d]: column sums of dq | dk | dv over all rows */,
                       const void* out_lo, const int32_t* seq_groups, int64_t num_groups, gmlm_stream_t stream);
/* dbias (optional, both pointers or neither; short-sequence path only, EINVAL otherwise): the bias gradient of a fused
 * QKV projection, sum over rows of [dq | dk | dv], formed inside the backward kernel from tiles it already holds
 * (three matrix-vector products on the MFMA pipe) instead of a separate pass over dqkv. */

/* ---------------------------------------------------------------------------------------------
 * Attention at head dim 128 (d must be 128; gmlm_attention_fwd / _bwd keep taking 64 and 96 only).
 * Same layout and semantics as the padded mode of gmlm_attention_fwd / _bwd: q [b, lq, h, 128], k / v [b, lk, h, 128] at
 * row strides *_stride, out / out_lo / dout [b, lq, h, 128] dense, dq / dk / dv at their row strides, lse / delta
 * [b, h, lq] fp32, kv_len int32 [b] or NULL, probability dropout with the same replayable hash and row offsets,
 * out_lo (bf16 only, optional) the residual of the output for an exact delta.  The dK/dV sums run in a fixed order
 * (no atomics): identical calls give identical bits.  Backward workspace: gmlm_attention_d128_workspace_bytes(b, h, lq).
 * ------------------------------------------------------------------------------------------- */
int gmlm_attention_d128_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t h,
                            int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                            float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* out,
                            void* out_lo, float* lse, int dtype, gmlm_stream_t stream);
size_t gmlm_attention_d128_workspace_bytes(int64_t b, int64_t h, int64_t lq);
int gmlm_attention_d128_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                            const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t h,
                            int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                            float scale, float dropout_p, uint64_t seed, const uint64_t* seed_dev, void* dq, void* dk,
                            void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype,
                            void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

/* BERT embedding sum (hf:modeling_bert.py:53-108 ahead of the LayerNorm): out[t] = word[tok[t]] + type0 + pos[pos_ids[t]],
 * fp32 tables, stored as `dtype` [rows, p]; replaces two gathers, two adds and a cast.  Its backward is a segment sum of the
 * output gradient by token id / position id (gmlm_segment_sort + gmlm_rgcn_mean_spmm with mean = 0).
 * F.embedding raises on an id outside its table; here an id outside [0, vocab) / [0, npos) is never read out of bounds (it is
 * clamped) and sets *bad_flag = 1 (device int32, nullable, NOT cleared by the call): the caller checks it when it next
 * synchronises, or validates its (static) id tensors once up front, as the Python host does.
 * p % 4 == 0; word, pos, type0 and out are 16-byte aligned. */
int gmlm_embed_sum_fwd(const float* word, const float* pos, const float* type0, const int64_t* tok, const int64_t* pos_ids,
                       int64_t rows, int64_t p, int64_t vocab, int64_t npos, void* out, int dtype, int32_t* bad_flag,
                       gmlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K8  attention-mask-weighted mean pooling + row scatter          (main.py:351-358)
 * out[node_idx[b], :] = sum_t hs[b,t,:] * [t < len[b]] / max(len[b], 1e-9)     (out fp32 [n, p])
 * -------------------------------------------------------------------------------------------
 * cu_seqlens != NULL: hs is packed [total_rows, p], sequence b = rows [cu[b], cu[b+1]) (len / l unused).
 * One of len / cu_seqlens is required, the other nullable.  b <= 65535.  Scalar accesses: no alignment rule.
 * hs is required when l > 0; in packed mode (l is passed as 0) whenever a sequence has a row, which the caller's
 * cu_seqlens decides and the host cannot check.  node_idx, out / dout and dhs are required.  b = 0 returns at once, the
 * padded backward with l = 0 too.
 */
int gmlm_meanpool_scatter_fwd(const void* hs, const int32_t* len, const int64_t* node_idx, int64_t b, int64_t l,
                              int64_t p, float* out, int dtype, const int32_t* cu_seqlens, gmlm_stream_t stream);
int gmlm_meanpool_scatter_bwd(const float* dout, const int32_t* len, const int64_t* node_idx, int64_t b, int64_t l,
                              int64_t p, void* dhs, int dtype, const int32_t* cu_seqlens, gmlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * K9  soft-mask row blend                                           (main.py:92-99)
 * out[i,:] = mask[i] ? (1-beta)*x[i,:] + beta*token : x[i,:]     (out row stride out_stride, dtype out)
 * bwd: dtoken[c] = beta * sum_{i: mask[i]} dout[i,c]     (n = 0 fills dtoken with zeros)
 * Scalar accesses: no alignment rule, any out_stride / dout_stride >= f.  No pointer is nullable.
 * bwd workspace: gmlm_softmask_blend_bwd_workspace_bytes(n, f).
 * ------------------------------------------------------------------------------------------- */
int gmlm_softmask_blend_fwd(const float* x, const uint8_t* mask, const float* token, float beta, int64_t n,
                            int64_t f, void* out, int64_t out_stride, int dtype, gmlm_stream_t stream);
size_t gmlm_softmask_blend_bwd_workspace_bytes(int64_t n, int64_t f);
int gmlm_softmask_blend_bwd(const float* dout, int64_t dout_stride, const uint8_t* mask, float beta, int64_t n,
                            int64_t f, float* dtoken, void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

/* GELU (exact erf) + dropout elementwise with optional bias, used for BertIntermediate
 * (hf:modeling_bert.py:333-336) and classifier.1 (main.py:245): y = dropout(gelu(x + bias)).
 * f: a multiple of 8 (bf16) / 4 (fp32); x, y, dy, dx 16-byte aligned; bias (fp32 [f], scalar loads) is nullable. */
int gmlm_bias_gelu_fwd(const void* x, const float* bias, int64_t rows, int64_t f, float dropout_p, uint64_t seed, const uint64_t* seed_dev,
                       void* y, int dtype, gmlm_stream_t stream);
/* dx = dy * dropout_mask * gelu'(x + bias); dbias (nullable) [f] = column sums of dx, accumulated in fp32
 * inside the same pass (workspace: gmlm_bias_gelu_bwd_workspace_bytes; required with dbias, unused and nullable
 * without it).  rows = 0 fills dbias with zeros. */
size_t gmlm_bias_gelu_bwd_workspace_bytes(int64_t rows, int64_t f, int dtype);
int gmlm_bias_gelu_bwd(const void* dy, const void* x, const float* bias, int64_t rows, int64_t f, float dropout_p,
                       uint64_t seed, const uint64_t* seed_dev, void* dx, float* dbias, int dtype, void* workspace, size_t workspace_bytes,
                       gmlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Split-K weight gradient of the dense layers (bf16 operands, fp32 result)
 * out[n, k] (row stride ld_out) = sum_{t < T} dy[t, n] * x[t, k], dy [T, N] (row stride ld_dy) and x [T, K] (ld_x) bf16.
 * N and K multiples of 256, T >= 32, row strides multiples of 8 elements (4 for out), pointers 16-byte aligned.
 * T is cut into `splits` contiguous slices (0 = the default plan: about 256 workgroups); each slice of each 256 x 256
 * tile goes to a fp32 partial in the workspace, which a second launch adds in slice order: deterministic.
 * flags: GMLM_WGRAD_NO_REMAP = plain workgroup order (no XCD grouping of the slices); GMLM_WGRAD_ONE_PHASE = the one-barrier
 * main loop (all waves read, then multiply, in lock-step) instead of the default two wave groups a phase apart; same bits.
 * workspace: gmlm_wgrad_workspace_bytes(T, N, K, splits), no initialisation needed.
 * ------------------------------------------------------------------------------------------- */
#define GMLM_WGRAD_NO_REMAP 1
#define GMLM_WGRAD_ONE_PHASE 2
size_t gmlm_wgrad_workspace_bytes(int64_t t, int64_t n, int64_t k, int splits);
int gmlm_wgrad_bf16(const void* dy, int64_t ld_dy, const void* x, int64_t ld_x, int64_t t, int64_t n, int64_t k, int splits,
                    float* out, int64_t ld_out, int flags, void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Row kernels of the pre-norm decoder-style text encoders (Qwen3 geometry).  bf16 or fp32 storage (`dtype`), fp32
 * arithmetic, one rounding on store; every pointer 16-byte aligned; sums over rows run in a fixed order (no atomics).
 * Order of the checks, here and in the causal attention below: sizes, strides and dtype are validated first; then a call
 * with nothing to do (rows = 0, tokens = 0, l = 0) returns GMLM_OK before any data pointer is required, so the NULL
 * pointers of empty tensors are fine.  Such a call launches nothing, except that a backward with a weight gradient (dw,
 * dq_weight | dk_weight: required even then) fills it with zeros.  gmlm_qknorm_rope_*: seq_len = 0 is accepted only with
 * tokens = 0.
 * ------------------------------------------------------------------------------------------- */
/* Residual add + RMSNorm over rows of width f (a multiple of 8 (bf16) / 4 (fp32), at most 4096):
 *   sum = a + b, stored to s in `dtype` (b and s are given together or both NULL: sum = a, nothing stored);
 *   y = sum * rstd * w with rstd[r] = rsqrt(mean(sum^2) + eps) (fp32 [rows], taken over the STORED sum); w fp32 [f]. */
int gmlm_add_rmsnorm_fwd(const void* a, const void* b, const float* w, int64_t rows, int64_t f, float eps, void* s, void* y,
                         float* rstd, int dtype, gmlm_stream_t stream);
/* s = the sum the forward normalised (its s, or its a when b was NULL); dres (nullable) = the gradient arriving on the
 * residual stream.  ds = dres + d(sum) is the gradient of a and of b; dw fp32 [f].
 * workspace: gmlm_add_rmsnorm_bwd_workspace_bytes(rows, f). */
size_t gmlm_add_rmsnorm_bwd_workspace_bytes(int64_t rows, int64_t f);
int gmlm_add_rmsnorm_bwd(const void* dy, const void* dres, const void* s, const float* w, const float* rstd, int64_t rows,
                         int64_t f, void* ds, float* dw, int dtype, void* workspace, size_t workspace_bytes,
                         gmlm_stream_t stream);
/* Per-head RMSNorm of Q and K + rotary position embedding (d must be 128).  qkv: `tokens` rows [q (hq heads) | k (hkv) |
 * v (hkv)] x 128 at row stride qkv_stride; token t sits at position t % seq_len (padded [b, seq_len] layout).
 * For every Q and K head row x: n = x * rsqrt(mean(x^2) + eps) * weight (q_weight / k_weight, fp32 [128]), then
 * out[i] = n[i] cos[i] - n[i+64] sin[i], out[i+64] = n[i+64] cos[i] + n[i] sin[i]  (i < 64), written to out
 * [tokens, (hq + hkv) * 128] at row stride out_stride; V is not touched.  cos_sin: fp32 [max_len, 2, 64] (the cos row,
 * then the sin row of each position; seq_len <= max_len).  rstd: fp32 [tokens, hq + hkv]. */
int gmlm_qknorm_rope_fwd(const void* qkv, int64_t qkv_stride, const float* q_weight, const float* k_weight,
                         const float* cos_sin, int64_t max_len, int64_t tokens, int64_t seq_len, int64_t hq, int64_t hkv,
                         int64_t d, float eps, void* out, int64_t out_stride, float* rstd, int dtype, gmlm_stream_t stream);
/* IN PLACE on the first (hq + hkv) * 128 columns of dqkv (row stride dqkv_stride): on entry the gradient of the rotated
 * Q | K, on return the gradient of the projection output (inverse rotation, then the RMSNorm backward); the V columns
 * are left alone.  dq_weight / dk_weight: one fp32 [2, 128] buffer (dk_weight == dq_weight + 128).
 * workspace: gmlm_qknorm_rope_bwd_workspace_bytes(tokens, hq, hkv, dtype). */
size_t gmlm_qknorm_rope_bwd_workspace_bytes(int64_t tokens, int64_t hq, int64_t hkv, int dtype);
int gmlm_qknorm_rope_bwd(void* dqkv, int64_t dqkv_stride, const void* qkv, int64_t qkv_stride, const float* q_weight,
                         const float* k_weight, const float* cos_sin, int64_t max_len, const float* rstd, int64_t tokens,
                         int64_t seq_len, int64_t hq, int64_t hkv, int64_t d, float* dq_weight, float* dk_weight, int dtype,
                         void* workspace, size_t workspace_bytes, gmlm_stream_t stream);
/* The same two operations for packed rows: token t sits at position pos_ids[t] (int32 [tokens], required) instead of
 * t % seq_len; an index outside [0, max_len) is clamped into the table, never read past it.  Same kernels, same
 * arithmetic: with pos_ids[t] = t % seq_len the results are bit for bit those of the entry points above.  The backward's
 * workspace is gmlm_qknorm_rope_bwd_workspace_bytes(tokens, hq, hkv, dtype). */
int gmlm_qknorm_rope_pos_fwd(const void* qkv, int64_t qkv_stride, const float* q_weight, const float* k_weight,
                             const float* cos_sin, int64_t max_len, int64_t tokens, const int32_t* pos_ids, int64_t hq,
                             int64_t hkv, int64_t d, float eps, void* out, int64_t out_stride, float* rstd, int dtype,
                             gmlm_stream_t stream);
int gmlm_qknorm_rope_pos_bwd(void* dqkv, int64_t dqkv_stride, const void* qkv, int64_t qkv_stride, const float* q_weight,
                             const float* k_weight, const float* cos_sin, int64_t max_len, const float* rstd, int64_t tokens,
                             const int32_t* pos_ids, int64_t hq, int64_t hkv, int64_t d, float* dq_weight, float* dk_weight,
                             int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream);
/* SwiGLU: gate_up [rows, 2 * inter] = [gate | up] -> y [rows, inter] = silu(gate) * up; the backward returns the fused
 * [rows, 2 * inter] gradient.  inter: a multiple of 8 (bf16) / 4 (fp32). */
int gmlm_swiglu_fwd(const void* gate_up, int64_t rows, int64_t inter, void* y, int dtype, gmlm_stream_t stream);
int gmlm_swiglu_bwd(const void* dy, const void* gate_up, int64_t rows, int64_t inter, void* dgate_up, int dtype,
                    gmlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Causal self-attention with grouped KV heads at head dim 128 (d must be 128, lq == lk, hq % hkv == 0).
 * q / dq [b, l, hq, 128] and k / v / dk / dv [b, l, hkv, 128], each at its own row stride (a fused [q | k | v] row works
 * without copies); out / out_lo / dout [b, l, hq, 128] dense; lse / delta [b, hq, l] fp32.  Query head j reads KV head
 * j / (hq / hkv).  Query i sees the keys <= i that lie below kv_len[b] (int32 [b] or NULL = l); a sequence with
 * kv_len = 0 has zero output, lse = -inf and zero gradients.  dropout_p must be 0 (no probability dropout here).
 * out_lo (bf16 only, optional): residual of the output for an exact delta, as in gmlm_attention_d128_*.
 * dK / dV are summed over the query heads of a group and the query tiles in a fixed order (no atomics, no expanded
 * K / V): identical calls give identical bits.  Backward workspace: gmlm_attention_causal_d128_workspace_bytes(b, hq, lq).
 * ------------------------------------------------------------------------------------------- */
int gmlm_attention_causal_d128_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                   int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                   int64_t v_stride, float scale, float dropout_p, void* out, void* out_lo, float* lse,
                                   int dtype, gmlm_stream_t stream);
size_t gmlm_attention_causal_d128_workspace_bytes(int64_t b, int64_t hq, int64_t lq);
int gmlm_attention_causal_d128_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                   const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq,
                                   int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                   int64_t v_stride, float scale, float dropout_p, void* dq, void* dk, void* dv,
                                   int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                   size_t workspace_bytes, gmlm_stream_t stream);
/* The same attention on a packed (variable-length) batch: q / dq [total_rows, hq, 128], k / v / dk / dv [total_rows, hkv, 128]
 * at their own row strides, out / out_lo / dout [total_rows, hq, 128] dense, lse / delta [hq, total_rows] fp32.  Sequence i
 * owns rows [cu_seqlens[i], cu_seqlens[i + 1]) (int32 [num_seqs + 1], required, non-decreasing, last entry <= total_rows);
 * its length is its row count (there is no kv_len), it may be 0, and none may exceed max_len (> 0), which only sizes the
 * grid.  total_rows < 2^30.  Rows owned by no sequence are neither read nor written.  Same kernels, same summation order
 * as the padded entry points.  Backward workspace: gmlm_attention_causal_d128_varlen_workspace_bytes(total_rows, hq). */
int gmlm_attention_causal_d128_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                          int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv,
                                          int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                          float dropout_p, void* out, void* out_lo, float* lse, int dtype, gmlm_stream_t stream);
size_t gmlm_attention_causal_d128_varlen_workspace_bytes(int64_t total_rows, int64_t hq);
int gmlm_attention_causal_d128_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                          const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                          int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d,
                                          int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                                          void* dq, void* dk, void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride,
                                          int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GMLM_HIP_H */
