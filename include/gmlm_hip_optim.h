/* gmlm_hip_optim.h — third header of libgmlm_hip.so's C ABI: gradient clipping + AdamW as one multi-tensor step.
 *
 * gmlm_amd.FusedAdamW replaces the tail of a training iteration, clip_grad_norm_ + torch.optim.AdamW.step, by three launches on
 * one stream:
 *   gmlm_adamw_sumsq     one fp32 sum of squares and one non-finite flag per CHUNK of the gradients;
 *   gmlm_adamw_finalize  norm, clip coefficient and the skip decision from those, step counters and bias corrections;
 *   gmlm_adamw_update    decoupled AdamW on p, m, v with the clipped gradient, or nothing at all when the step is skipped.
 * No host synchronisation, no atomics, no allocation; the gradient is read twice and never written (clip_grad_norm_ scales
 * .grad in place, this path does not); p, m and v are read once and written once: 32 bytes per parameter.
 * The reference has no counterpart (torch.optim.AdamW behind clip_grad_norm_ and GradScaler, main.py:375-398, 528-563).
 *
 * Conventions: those of gmlm_hip.h, which this header includes for its types and status codes.  Every pointer is a DEVICE
 * pointer owned by the caller; the library never allocates, frees or synchronises and enqueues only on `stream` (nullable); a
 * call returns 0 or a negative GMLM_E* code with a thread-local gmlm_last_error() message; arguments are validated on the host
 * BEFORE any launch; counts are checked before a call with nothing to do returns GMLM_OK, and such a call needs no pointer;
 * re-entrant and thread-safe (no state of its own: everything lives in the caller's tables).
 *
 * Tables (T tensors, G groups, S step slots, N chunks; C = gmlm_adamw_chunk_elems() elements).  Every table and workspace
 * pointer must be 16-byte aligned (checked, GMLM_EINVAL); the TENSORS the address table names need 4-byte alignment only:
 * the kernels move 16 bytes per lane with dword-aligned vector accesses, so a view into a larger buffer at any element offset
 * takes the same path, the same summation order and gives the same bits as an aligned tensor.
 *   addr       uint64  [T][4]  device addresses of (p, g, m, v) of tensor t: parameter, gradient, exp_avg, exp_avg_sq, each
 *                              numel[t] contiguous fp32 values.  No two of the 4 T ranges may overlap.
 *   numel      int64   [T]     element counts, each >= 1.
 *   group      int32   [T]     row of `hyper` that tensor t uses, in [0, G).
 *   slot       int32   [T]     index of tensor t's step counter in `steps`, in [0, S); distinct within one call.  The slot is
 *                              what lets a call cover only the tensors that have a gradient this time.
 *   chunks     int32   [N][2]  (tensor t, chunk c of that tensor): elements [c C, min((c + 1) C, numel[t])) of tensor t.
 *                              Tensor-major: all chunks of tensor 0 in ascending order, then tensor 1, ...; every element of
 *                              every tensor in exactly one chunk, i.e. N = sum over t of ceil(numel[t] / C).
 *   hyper      double  [G][8]  {lr, weight_decay, beta1, beta2, eps, 0, 0, 0} per group.
 *   steps      int32   [S]     optimiser steps taken per slot; caller zero-initialises, gmlm_adamw_finalize advances.
 *   bias_corr  float   [T][2]  workspace, 8 T bytes: {1 - beta1^t, sqrt(1 - beta2^t)} per tensor, evaluated in double.
 *   partial    float   [N]     workspace, 4 N bytes: sum of squares of each chunk's gradient.
 *   nonfinite  int32   [N]     workspace, 4 N bytes: 1 where a chunk's gradient holds an infinity or a NaN, else 0.
 *   status     32 bytes        [0] float norm, [1] float coef, [2] int32 skip, [3] int32 bad_table, [4] int32 skipped steps
 *                              so far (caller zero-initialises once; finalize adds 1 per skipped step), [5..7] unused.
 *
 * The host cannot see into these tables: that every address is valid for numel[t] floats, that the chunk table is the plan
 * above, and that no two tensors overlap is the caller's word.  group[t] and slot[t] are checked ON THE DEVICE by
 * gmlm_adamw_finalize: one of them out of range sets status.bad_table = 1 and skip = 1, so that the update touches nothing.
 */
#ifndef GMLM_HIP_OPTIM_H
#define GMLM_HIP_OPTIM_H

#include "gmlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host only, never launches: C, the number of elements per chunk (a multiple of 4). */
int64_t gmlm_adamw_chunk_elems(void);

/* Launch a.  One workgroup per chunk: partial[n] = sum of g^2 over chunk n in fp32 and in a fixed order (each lane serially
 * over its elements, then across the wave, then across the waves through LDS; the same bits on every call), nonfinite[n] as
 * above.  Reads addr (the g column), numel, chunks.
 * Refused (GMLM_EINVAL): num_chunks < 0 or >= 2^31; with num_chunks > 0, a null or not 16-byte aligned addr / numel / chunks /
 * partial / nonfinite.  num_chunks == 0: GMLM_OK without a launch. */
int gmlm_adamw_sumsq(const void* addr, const int64_t* numel, const int* chunks, int64_t num_chunks, float* partial,
                     int* nonfinite, gmlm_stream_t stream);

/* Launch b.  One workgroup.  sum = partial[0] + partial[1] + ... in index order in double; norm = sqrt(sum);
 * coef = min(1, max_norm / (norm + 1e-6)), clip_grad_norm_'s formula, and coef = 1 (no clipping) when max_norm <= 0, is
 * infinite or is NaN; skip = any nonfinite[n] or norm not finite or bad_table.  Writes status {norm, coef, skip, bad_table}.
 * Not skipped: steps[slot[t]] += 1 for the T tensors of this call and bias_corr[t] = {1 - beta1^s, sqrt(1 - beta2^s)} with
 * s the new count and the betas of hyper[group[t]].  Skipped: status[4] += 1 and nothing else (GradScaler's skip, decided on
 * the device).
 * Refused (GMLM_EINVAL): num_chunks, num_tensors, num_groups or num_slots negative; num_chunks >= 2^31; num_tensors >
 * num_chunks (every tensor has a chunk) or > num_slots; num_groups == 0 with num_tensors > 0; a null or not 16-byte aligned
 * partial / nonfinite / group / slot / hyper / steps / bias_corr / status.  num_chunks == 0 or num_tensors == 0: GMLM_OK
 * without a launch. */
int gmlm_adamw_finalize(const float* partial, const int* nonfinite, int64_t num_chunks, float max_norm, const int* group,
                        const int* slot, int64_t num_tensors, const double* hyper, int64_t num_groups, int* steps,
                        int64_t num_slots, float* bias_corr, void* status, gmlm_stream_t stream);

/* Launch c.  One workgroup per chunk of the same chunk table.  status.skip set: returns without touching memory (p, m, v
 * and the step counters keep their bits).  Otherwise, per element in fp32, torch's decoupled AdamW:
 *   g' = coef g;  p = p (1 - lr wd);  m = m + (g' - m)(1 - beta1);  v = beta2 v + (1 - beta2) g'^2;
 *   p = p - (lr / bc1) m / (sqrt(v) / bc2s + eps)          with {bc1, bc2s} = bias_corr[t].
 * Reads g, p, m, v once and writes p, m, v once; g is not modified.
 * Refused (GMLM_EINVAL): num_chunks < 0 or >= 2^31; num_groups < 0, or == 0 with num_chunks > 0; with num_chunks > 0, a null or
 * not 16-byte aligned addr / numel / group / chunks / hyper / bias_corr / status.  num_chunks == 0: GMLM_OK without a launch. */
int gmlm_adamw_update(const void* addr, const int64_t* numel, const int* group, const int* chunks, int64_t num_chunks,
                      const double* hyper, int64_t num_groups, const float* bias_corr, const void* status,
                      gmlm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GMLM_HIP_OPTIM_H */
