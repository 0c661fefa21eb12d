/* gmlm_hip_split.h — second header of libgmlm_hip.so's C ABI: the bf16x3 operand split.
 *
 * GraphTextLM(gemm_precision="bf16x3") keeps fp32 storage everywhere and runs its dense layers as ONE bf16 GEMM of three times
 * the contraction depth with an fp32 result: every fp32 operand is split into two bf16 terms, x ~ hi + lo, and
 *   [a_hi | a_lo | a_hi] [b_hi | b_hi | b_lo]^T = a_hi b_hi^T + a_lo b_hi^T + a_hi b_lo^T.
 * The reference has no counterpart (its dense layers are torch.nn.Linear under autocast, main.py:348); the entry below feeds
 * the library GEMM that replaces them in that mode.
 *
 * Conventions: those of gmlm_hip.h, which this header includes for its types and status codes.  Every pointer is a DEVICE
 * pointer owned by the caller; the library never allocates, frees or synchronises and enqueues only on `stream` (nullable);
 * a call returns 0 or a negative GMLM_E* code with a thread-local gmlm_last_error() message; arguments are validated on the
 * host BEFORE any launch; sizes and strides (in elements) are checked before a call with nothing to do returns GMLM_OK, and
 * such a call needs no data pointer; "16-byte aligned" pointers are checked (GMLM_EINVAL); re-entrant, thread-safe, and safe
 * to call twice with the same arguments (identical bytes).
 */
#ifndef GMLM_HIP_SPLIT_H
#define GMLM_HIP_SPLIT_H

#include "gmlm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* x: fp32 [rows, cols], row stride ld_x (>= cols, a multiple of 4), 16-byte aligned.
 * out: bf16, 16-byte aligned; three parts p = 0, 1, 2 of [rows, cols_out] each: part p starts at out + p * part_stride, its
 *      row r at + r * ld_out.  cols_out >= cols and a multiple of 8 (the caller rounds cols up); ld_out and part_stride are
 *      multiples of 8.
 * order 0: the parts are (hi, lo, hi); order 1: (hi, hi, lo), where
 *      hi = bf16(x) rounded to nearest even (NaN stays NaN),
 *      lo = bf16(x - float(hi)) (the difference is exact in fp32), and lo = +0 where hi is not finite, so that an infinity
 *      stays an infinity in the three-product sum.
 *      Columns cols .. cols_out-1 of all three parts are written as zeros; nothing at or past column `cols` of x is read.
 *      Sub-normal x or lo values are outside the contract.
 * The parts must not overlap.  Accepted layouts:
 *      side by side along the contraction dimension: part_stride >= cols_out and ld_out >= 2 * part_stride + cols_out
 *                                                    (dense: part_stride = cols_out, ld_out = 3 * cols_out);
 *      stacked: part_stride >= (rows - 1) * ld_out + cols_out and ld_out >= cols_out (dense: part_stride = rows * ld_out).
 * Refused (GMLM_EINVAL): null or misaligned x / out, negative sizes, ld_x < cols or not a multiple of 4, cols_out < cols or
 * not a multiple of 8, ld_out or part_stride not a multiple of 8, order outside {0, 1}, rows * (cols_out / 8) >= 2^31,
 * overlapping parts.  rows == 0 or cols_out == 0: GMLM_OK without a launch. */
int gmlm_split_bf16x3(const float* x, int64_t ld_x, int64_t rows, int64_t cols, int64_t cols_out,
                      void* out, int64_t ld_out, int64_t part_stride, int order, gmlm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* GMLM_HIP_SPLIT_H */
