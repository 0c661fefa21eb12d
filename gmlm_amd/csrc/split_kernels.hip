// bf16x3 operand split (include/gmlm_hip_split.h): an fp32 matrix -> three bf16 parts (hi, lo, hi) or (hi, hi, lo), so that an
// fp32-grade dense layer runs as ONE bf16 MFMA GEMM of three times the contraction depth:
//   [a_hi | a_lo | a_hi] [b_hi | b_hi | b_lo]^T = a_hi b_hi^T + a_lo b_hi^T + a_hi b_lo^T     (fp32 accumulation)
// One streaming pass, 4 bytes in and 6 bytes out per element; no LDS, no atomics, no scratch.
#include "common.hpp"
#include "../../include/gmlm_hip_split.h"

namespace gmlm {
namespace split3 {

// One lane: 8 consecutive fp32 values of a row (two 16-byte loads) -> one 16-byte store into each of the three parts.
// ORDER 0: parts (hi, lo, hi); ORDER 1: parts (hi, hi, lo).  hi = bf16_rne(x) (v_cvt_pk_bf16_f32: ties to even, NaN stays NaN),
// lo = bf16_rne(x - float(hi)) - the difference is exact in fp32 - and lo = +0 where hi is not finite (an infinity stays an
// infinity in the three-product sum instead of inf - inf adding a NaN).  Columns cols .. cols_out-1 are written as zeros; the
// chunk that straddles `cols` reads nothing at or past it.
template <int ORDER>
__global__ __launch_bounds__(256) void split_rows_kernel(const float* __restrict__ x, int64_t ld_x, int64_t rows, int64_t cols,
                                                         int64_t chunks, bf16_t* __restrict__ out, int64_t ld_out,
                                                         int64_t part_stride) {
  // the host keeps rows * chunks below 2^31 and the grid at 2,048 blocks: the work index and its stride fit 32 bits (one
  // 32-bit division per 8 elements instead of a 64-bit one)
  const uint32_t total = (uint32_t)(rows * chunks), nchunk = (uint32_t)chunks;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int64_t r = i / nchunk;
    const int64_t c = (int64_t)(i - (uint32_t)r * nchunk) * 8;
    const float* src = x + r * ld_x + c;
    float v[8];
    if (c + 8 <= cols) {
      const float4 a = *reinterpret_cast<const float4*>(src);
      const float4 b = *reinterpret_cast<const float4*>(src + 4);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
      v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (c + j < cols) ? src[j] : 0.f;
    }
    uint32_t hi[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t h = pack_bf16x2(v[2 * j], v[2 * j + 1]);
      const uint32_t h0 = h << 16, h1 = h & 0xffff0000u;                 // the two hi values as fp32 bit patterns
      const float l0 = (h0 & 0x7f800000u) == 0x7f800000u ? 0.f : v[2 * j] - __uint_as_float(h0);
      const float l1 = (h1 & 0x7f800000u) == 0x7f800000u ? 0.f : v[2 * j + 1] - __uint_as_float(h1);
      hi[j] = h;
      lo[j] = pack_bf16x2(l0, l1);
    }
    const uint4 vh = make_uint4(hi[0], hi[1], hi[2], hi[3]);
    const uint4 vl = make_uint4(lo[0], lo[1], lo[2], lo[3]);
    bf16_t* dst = out + r * ld_out + c;
    *reinterpret_cast<uint4*>(dst) = vh;
    *reinterpret_cast<uint4*>(dst + part_stride) = ORDER == 0 ? vl : vh;
    *reinterpret_cast<uint4*>(dst + 2 * part_stride) = ORDER == 0 ? vh : vl;
  }
}

}  // namespace split3
}  // namespace gmlm

using namespace gmlm;

extern "C" int gmlm_split_bf16x3(const float* x, int64_t ld_x, int64_t rows, int64_t cols, int64_t cols_out, void* out,
                                 int64_t ld_out, int64_t part_stride, int order, gmlm_stream_t stream) {
  static const char* who = "split_bf16x3";
  GMLM_REQUIRE(rows >= 0 && cols >= 0 && cols_out >= 0 && ld_x >= 0 && ld_out >= 0 && part_stride >= 0,
               "%s: negative size (rows %ld, cols %ld, cols_out %ld, ld_x %ld, ld_out %ld, part_stride %ld)", who, (long)rows,
               (long)cols, (long)cols_out, (long)ld_x, (long)ld_out, (long)part_stride);
  GMLM_REQUIRE(order == 0 || order == 1, "%s: order %d must be 0 (hi, lo, hi) or 1 (hi, hi, lo)", who, order);
  GMLM_REQUIRE(ld_x >= cols && ld_x % 4 == 0, "%s: ld_x %ld must be >= cols %ld and a multiple of 4", who, (long)ld_x, (long)cols);
  GMLM_REQUIRE(cols_out >= cols && cols_out % 8 == 0, "%s: cols_out %ld must be >= cols %ld and a multiple of 8", who,
               (long)cols_out, (long)cols);
  GMLM_REQUIRE(ld_out % 8 == 0, "%s: ld_out %ld must be a multiple of 8", who, (long)ld_out);
  GMLM_REQUIRE(part_stride % 8 == 0, "%s: part_stride %ld must be a multiple of 8", who, (long)part_stride);
  const int64_t chunks = cols_out / 8;
  GMLM_REQUIRE((__int128)rows * chunks < ((__int128)1 << 31), "%s: rows * (cols_out / 8) = %ld * %ld must be below 2^31", who,
               (long)rows, (long)chunks);
  if (rows == 0 || cols_out == 0) return GMLM_OK;
  // the three parts must not overlap: side by side inside a row, or stacked one whole matrix after the other
  const __int128 ps = part_stride, ld = ld_out;
  const bool side_by_side = part_stride >= cols_out && ld >= 2 * ps + cols_out;
  const bool stacked = ps >= (__int128)(rows - 1) * ld + cols_out && ld_out >= cols_out;
  GMLM_REQUIRE(side_by_side || stacked,
               "%s: overlapping parts: part_stride %ld / ld_out %ld fit neither the side-by-side layout (part_stride >= cols_out, "
               "ld_out >= 2 part_stride + cols_out) nor the stacked one (part_stride >= (rows - 1) ld_out + cols_out, ld_out >= cols_out)",
               who, (long)part_stride, (long)ld_out);
  GMLM_REQUIRE(x && out, "%s: null pointer (x or out)", who);
  GMLM_REQUIRE(aligned16(x) && aligned16(out), "%s: x and out must be 16-byte aligned", who);
  hipStream_t st = as_stream(stream);
  const int grid = grid_cap(cdiv(rows * chunks, 256));
  if (order == 0)
    split3::split_rows_kernel<0><<<grid, 256, 0, st>>>(x, ld_x, rows, cols, chunks, static_cast<bf16_t*>(out), ld_out, part_stride);
  else
    split3::split_rows_kernel<1><<<grid, 256, 0, st>>>(x, ld_x, rows, cols, chunks, static_cast<bf16_t*>(out), ld_out, part_stride);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
