// Host side shared by the LDS-resident short-sequence attention families (attn_short.hip, attn_gqa_short.hip,
// attn_d32_short.hip): the tile height, the launcher over (flag, R), the packed-and-grouped argument checks and the tail of the
// fused bias sums.  The LDS sizes come from ShortLds (attn_short.hpp), which the kernels carve with.  No device code here.
#pragma once
#include "attn_host.hpp"
#include "attn_short.hpp"
#include "colreduce.hpp"

namespace gmlm {

// no item holds more rows than the call has, nor more than 128: the tile height R, a multiple of 32
inline int short_tile_rows(int64_t rows) { return (int)((rows < 128 ? rows : 128) + 31) / 32 * 32; }

// The eight instantiations of one (family, direction), [flag][R / 32 - 1], with their LDS layout.  K(flag, R) names one.
template <class P>
struct ShortKernels {
  void (*k[2][4])(P);
  ShortLds lds;
  PerDeviceOnce once;
};
#define GMLM_SHORT_KERNELS(K) {{K(false, 32), K(false, 64), K(false, 96), K(false, 128)}, {K(true, 32), K(true, 64), K(true, 96), K(true, 128)}}

// Sets the dynamic-LDS attribute of all eight once per device, then launches the one of (flag, top) with 2 * top threads.
template <class P>
int short_launch(ShortKernels<P>& t, int top, bool flag, unsigned grid, hipStream_t st, const P& prm) {
  int rc = t.once([&]() -> int {
    for (int f = 0; f < 2; ++f)
      for (int i = 0; i < 4; ++i)
        GMLM_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(t.k[f][i]), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)t.lds.bytes(32 * (i + 1))));
    return GMLM_OK;
  });
  if (rc != GMLM_OK) return rc;
  if (top >= 32 && top <= 128 && top % 32 == 0) t.k[flag][top / 32 - 1]<<<grid, 2 * top, t.lds.bytes(top), st>>>(prm);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

// The packed layout with seq_groups, as every grouped short entry point takes it; after it the family's own layout lines, then
// short_check_items
inline int short_check_packed(const char* who, const int32_t* cu, const int32_t* groups, int64_t num_groups, int64_t max_len, int64_t rows) {
  GMLM_REQUIRE(cu, "%s: null cu_seqlens", who);
  GMLM_REQUIRE(groups, "%s: null seq_groups", who);
  GMLM_REQUIRE(num_groups >= 0, "%s: num_groups %ld must be >= 0", who, (long)num_groups);
  GMLM_REQUIRE(max_len > 0 && max_len <= 128, "%s: max_len %ld must be in 1..128", who, (long)max_len);
  GMLM_REQUIRE(rows >= 0 && rows < ((int64_t)1 << 30), "%s: total_rows = %ld packed rows (must be >= 0 and < 2^30)", who, (long)rows);
  return GMLM_OK;
}
// the work-item bound: per_group items for every group (query heads, or pairs of heads counted as heads)
inline int short_check_items(const char* who, int64_t num_groups, int64_t per_group) {
  GMLM_REQUIRE(num_groups <= (((int64_t)1 << 31) - 1) / per_group, "%s: too many work items", who);
  return GMLM_OK;
}

// the tail of the fused bias sums: [items, width] partial column sums -> [width], fixed order
static inline int short_bias_sums(const float* partial, int64_t items, int64_t width, float* dbias, hipStream_t st) {
  rows_sum_kernel<<<(unsigned)cdiv(width, 32), 256, 0, st>>>(partial, (int)items, width, dbias, 1.f);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

}  // namespace gmlm
