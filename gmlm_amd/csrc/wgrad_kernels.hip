// Split-K weight-gradient GEMM of the packed text encoder: dW[N, K] (fp32) = sum_t dy[t, n] * x[t, k], bf16 operands that both
// have the token index t as their SLOW index (row-major [T, N] / [T, K], any row stride).  The reduction runs over ~10^5
// tokens while the output is only 9..36 tiles of 256 x 256, so T is cut into S contiguous slices (S x tiles ~ one round of
// the 256 CUs); each workgroup sums one slice of one tile into a fp32 partial tile, and a second small kernel adds the S
// partials in slice order (plus the < 32 rows of the token tail) into dW: fixed summation order, bitwise reproducible,
// no workgroup ever waits on another one, no zero-initialised state.
//
// Main kernel, one 256 x 256 tile per workgroup, 8 waves as 2 (n) x 4 (k), each wave 128 x 64 = 8 x 4 accumulators of
// v_mfma_f32_16x16x32_bf16.  A stage is 32 token rows of dy[:, n0 .. n0 + 256) and of x[:, k0 .. k0 + 256): two 16 KiB images
// of 512-byte rows, filled by LDS-DMA (global_load_lds_dwordx4, 1 KiB of contiguous LDS per wave-instruction, per-lane
// source address).  A four-deep ring keeps up to three stages in flight across the barriers of a stage (counted
// vmcnt, raw s_barrier; guide "Pipelining across barriers").  Both MFMA operands want 8 consecutive TOKENS per lane, i.e.
// a column of the staged rows: they are read with ds_read_b64_tr_b16 (4 rows x 16 columns per 16-lane group).
//   Swizzle: 16-byte slot s of row r holds chunk s ^ 2 h(r), h(r) = (r & 3) | ((r >> 3) & 1) << 2.  A half-wave's
//   transposed read covers rows {8g + q} and {8g + 8 + q} (q = 0..3) at the same 32 columns: the 8 rows get 8 distinct h,
//   i.e. 8 distinct 32-byte bank windows of the 256-byte bank row -> conflict free.  The XOR keeps 32-byte pairs together
//   (even mask), so a lane's 8 bytes never straddle two slots.  Applied on the DMA SOURCE address (the LDS side of an
//   LDS-DMA is lane-linear) and again on the read.
//
// Schedules (template parameter; both give every accumulator the stages of its slice in order, one MFMA per stage, so
// the partial tiles are bit-identical):
//   ONE_PHASE (flag GMLM_WGRAD_ONE_PHASE): one barrier per stage; all 8 waves wait, read and multiply in lock-step.
//   TWO_PHASE (default): a stage is a READ phase (the 24 transposed reads, closed by lgkmcnt(0)) and an MMA phase (the 32
//   MFMAs), each opened by a workgroup barrier: A_s opens READ(s), B_s opens MMA(s).  Group 0 = waves 0-3, group 1 = waves
//   4-7; the two waves of a SIMD are w and w + 4, one of each group.  Group 1 executes one extra barrier before its loop and
//   group 0 one after, so group 1 runs exactly one phase behind: on every SIMD one wave issues MFMAs while the other
//   reads LDS and waits.  With the barriers of the workgroup numbered #0, #1, ...:
//                  READ(s) is after      MMA(s) is after
//       group 0        #2s                   #2s+1
//       group 1        #2s+1                 #2s+2
//   Rules the loop keeps (correctness is argued from these, not from clean runs):
//   RAW   stage s is first read after #2s (by group 0), so EVERY wave retires its own DMA pieces of stage s with a counted
//         vmcnt before it arrives at #2s: group 0 in front of its A_s (= #2s); group 1 in front of its B_(s-1) (= #2s), or
//         of its extra barrier #0 when s = 0 - one barrier earlier than its own A_s = #2s+1, which would be too late.
//   WAR   stage s+3 lands in the slot of stage s-1.  Group 1 reads stage s-1 in the phase that #2s ends (group 0 one phase
//         earlier), and every READ phase ends with lgkmcnt(0) in front of its barrier: a wave past #2s knows those reads
//         are done.  A wave issues stage s+3 at the start of its own READ(s): after #2s (group 0), after #2s+1 (group 1).
//   vmcnt immediates are 4 x (issued - s - 1) from `issued` at the point of the wait (group 1 waits for s+1 at the end of
//         READ(s), i.e. after the issue of that phase: one more stage issued than group 0 had at its wait for s in the same
//         iteration): 8 in the steady state, 4 / 0 only while the slice drains or is shorter than the ring (ns = 1, 2, 3:
//         the prologue issues ns stages and the short branches are taken).
//   Barrier count: 2 ns + 1 for both groups and every ns >= 1 (#0 .. #2ns; the last one is group 0's extra barrier and
//         group 1's B_(ns-1)).
//   The reads stay in READ and the MFMAs in MMA: sched_barrier(0) on both sides of the MFMA block, and the lgkmcnt(0) asm
//   is a memory clobber (the compiler's own progressive lgkmcnt waits inside the MMA block are then no-ops).
#include "attn_common.hpp"

namespace gmlm {

namespace wg {
constexpr int BT = 32;                       // token rows per stage (= the K of one 16x16x32 MFMA)
constexpr int TILE = 256;                    // output tile edge
constexpr int NW = 8;                        // waves
constexpr int NBUF = 4;                      // stage ring depth
constexpr int IMG = BT * TILE * 2;           // bytes of one operand image (16 KiB)
constexpr int STAGE = 2 * IMG;               // dy image, then x image
constexpr int LDS = NBUF * STAGE;            // 128 KiB
constexpr int PIECES = IMG / 1024 / NW;      // DMA wave-instructions per operand per stage and wave (2)
constexpr int VM_PER_STAGE = 2 * PIECES;     // vmcnt units one stage adds per wave (4)
__device__ __forceinline__ int swz(int r) { return 2 * ((r & 3) | (((r >> 3) & 1) << 2)); }
}  // namespace wg

struct WgradParams {
  const bf16_t* dy;
  const bf16_t* x;
  float* part;                               // [S][N][K] fp32 partial tiles
  int64_t ld_dy, ld_x, n, k;
  int32_t stages, splits, tiles_k, tiles, remap;
};

// this lane's byte offset inside piece 0 of an operand image: piece k of wave w covers rows 2 (w + 8 k) + (lane >> 5);
// rows advance by 16 per piece, which keeps the low four row bits and with them the swizzle: one offset serves both pieces
__device__ __forceinline__ uint32_t wg_src_off(int64_t ld, int w, int lane) {
  const int row = 2 * w + (lane >> 5), slot = lane & 31;
  return 2u * (uint32_t)(row * ld + 8 * (slot ^ wg::swz(row)));
}

__device__ __forceinline__ void wg_dma(const bf16_t* base, uint32_t off, uint32_t lds) {
  const uint32_t dst = __builtin_amdgcn_readfirstlane(lds);
  uint32_t keep;
  // inline asm on purpose (attn_dma.hpp): the builtin makes hipcc wait vmcnt(0) ahead of every later ds_read
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(off), "s"(base), "s"(dst) : "memory");
}

template <bool TWO_PHASE>
__global__ __launch_bounds__(wg::NW * 64, 1) void wgrad_bf16_kernel(WgradParams p) {
  using namespace wg;
  extern __shared__ __attribute__((aligned(1024))) unsigned char smem_dyn[];
  const uint32_t lds0 = (uint32_t)(size_t)(__attribute__((address_space(3))) void*)smem_dyn;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // workgroups are dealt round-robin over the 8 XCDs (id % 8 = XCD): the bijective remap of guide T1 gives each XCD a
  // contiguous range of logical ids, i.e. mostly the tiles of ONE slice, which share their dy / x slabs in that L2
  const uint32_t nwg = gridDim.x, id = blockIdx.x;
  uint32_t lid = id;
  if (p.remap) {
    const uint32_t q = nwg >> 3, r = nwg & 7, xcd = id & 7;
    lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (id >> 3);
  }
  const int slice = (int)(lid / (uint32_t)p.tiles), tile = (int)(lid % (uint32_t)p.tiles);
  const int n0 = (tile / p.tiles_k) * TILE, k0 = (tile % p.tiles_k) * TILE;
  const int st0 = (int)((int64_t)slice * p.stages / p.splits), st1 = (int)((int64_t)(slice + 1) * p.stages / p.splits);
  const int ns = st1 - st0;

  const uint32_t offa = wg_src_off(p.ld_dy, w, lane), offb = wg_src_off(p.ld_x, w, lane);
  const bf16_t* ga = p.dy + (int64_t)st0 * BT * p.ld_dy + n0;
  const bf16_t* gb = p.x + (int64_t)st0 * BT * p.ld_x + k0;
  const int64_t stepa = (int64_t)BT * p.ld_dy, stepb = (int64_t)BT * p.ld_x;
  auto issue = [&](int s) {                  // stage s of this slice into ring slot s % NBUF
    const uint32_t buf = lds0 + (uint32_t)((s % NBUF) * STAGE) + 1024u * (uint32_t)w;
    const bf16_t* a = ga + s * stepa;
    const bf16_t* b = gb + s * stepb;
#pragma unroll
    for (int k = 0; k < PIECES; ++k) {
      wg_dma(a + (int64_t)(16 * k) * p.ld_dy, offa, buf + 1024u * (uint32_t)(NW * k));
      wg_dma(b + (int64_t)(16 * k) * p.ld_x, offb, buf + (uint32_t)IMG + 1024u * (uint32_t)(NW * k));
    }
  };

  // transposed-read addresses: lane 4q + p of 16-lane group g supplies row 8g + q (+4 for the high half of the fragment),
  // columns c0 + 4p .. 4p + 3; rows 8g + q and 8g + 4 + q have the same swizzle (bit 2 is not in h)
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const int wr = w >> 2, wc = w & 3;
  const int row = 8 * g + q, sw = swz(row);
  const uint32_t rbase = (uint32_t)(row * (TILE * 2)) + 8u * (uint32_t)(pp & 1);
  uint32_t aoff[8], boff[4];
#pragma unroll
  for (int m = 0; m < 8; ++m) aoff[m] = rbase + 16u * (uint32_t)((((wr * 128 + 16 * m) >> 3) + (pp >> 1)) ^ sw);
#pragma unroll
  for (int j = 0; j < 4; ++j) boff[j] = (uint32_t)IMG + rbase + 16u * (uint32_t)((((wc * 64 + 16 * j) >> 3) + (pp >> 1)) ^ sw);

  typedef __attribute__((ext_vector_type(4))) float f32x4;
  f32x4 acc[8][4];
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[m][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // stage s has landed once at most (issued - s - 1) younger stages are outstanding (vmcnt counts in issue order)
  auto wait_stage = [&](int s, int issued) {
    const int younger = issued - s - 1;
    if (younger >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    static_assert(VM_PER_STAGE == 4 && NBUF == 4, "vmcnt immediates above assume 4 per stage and 2 younger stages");
  };
  bf16x8 a[8], b[4];
  auto read_stage = [&](int s) {
    const unsigned char* img = smem_dyn + (s % NBUF) * STAGE;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(GMLM_LDS3(bf16x4, img + boff[j]));
      const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(GMLM_LDS3(bf16x4, img + boff[j] + 4 * TILE * 2));
      b[j] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(GMLM_LDS3(bf16x4, img + aoff[m]));
      const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(GMLM_LDS3(bf16x4, img + aoff[m] + 4 * TILE * 2));
      a[m] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
  };
  auto mma_stage = [&] {
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[m], b[j], acc[m][j], 0, 0, 0);
  };

  const int pre = ns < NBUF - 1 ? ns : NBUF - 1;
  for (int s = 0; s < pre; ++s) issue(s);
  int issued = pre;
  if constexpr (!TWO_PHASE) {
    for (int s = 0; s < ns; ++s) {
      wait_stage(s, issued);
      // every wave's DMA of stage s has landed, and every wave has finished computing stage s - 1 (its slot is free)
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (issued < ns) { issue(issued); ++issued; }
      read_stage(s);
      mma_stage();
    }
  } else {
    const int grp = w >> 2;                  // wave-uniform (w is an SGPR): the branches below are scalar
    if (grp == 1) {
      wait_stage(0, issued);                 // RAW for stage 0: in front of #0
      __builtin_amdgcn_s_barrier();          // #0
    }
    for (int s = 0; s < ns; ++s) {
      if (grp == 0) wait_stage(s, issued);   // RAW for stage s: in front of #2s
      __builtin_amdgcn_s_barrier();          // A_s: #2s (group 0), #2s+1 (group 1)
      asm volatile("" ::: "memory");
      if (issued < ns) { issue(issued); ++issued; }   // stage s+3 into the slot of s-1 (WAR: past #2s)
      read_stage(s);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (grp == 1 && s + 1 < ns) wait_stage(s + 1, issued);   // RAW for stage s+1: in front of #2(s+1)
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();          // B_s: #2s+1 (group 0), #2s+2 (group 1)
      __builtin_amdgcn_sched_barrier(0);
      mma_stage();
      __builtin_amdgcn_sched_barrier(0);
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();       // #2ns
  }

  // C/D map of 16x16x32: column (k) = lane & 15, row (n) = 4 (lane >> 4) + register
  float* out = p.part + (int64_t)slice * p.n * p.k + (int64_t)(n0 + wr * 128 + 4 * g) * p.k + k0 + wc * 64 + (lane & 15);
#pragma unroll
  for (int m = 0; m < 8; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(int64_t)(16 * m + r) * p.k + 16 * j] = acc[m][j][r];
}

// dW[n, k] = sum over slices in order of the partial tiles, then the token tail rows [t_main, t) in row order (fp32 FMA;
// products of bf16 values are exact in fp32).  4 consecutive k per thread.
__global__ __launch_bounds__(256) void wgrad_combine_kernel(const float* __restrict__ part, int splits, int64_t n, int64_t k,
                                                            const bf16_t* __restrict__ dy, int64_t ld_dy, const bf16_t* __restrict__ x,
                                                            int64_t ld_x, int64_t t_main, int64_t t, float* __restrict__ out,
                                                            int64_t ld_out) {
  const int64_t k4 = k >> 2, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * k4) return;
  const int64_t r = i / k4, c = 4 * (i - r * k4);
  typedef __attribute__((ext_vector_type(4))) float f32x4;
  const int64_t nk = n * k;
  const float* src = part + r * k + c;
  // scalar adds on purpose: a vector-typed f32x4 += lowers to v_pk_add_f32 (DESIGN.md section 5 b)
  f32x4 s = *reinterpret_cast<const f32x4*>(src);
  for (int j = 1; j < splits; ++j) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(src + j * nk);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = __fadd_rn(s[e], v[e]);
  }
  for (int64_t tt = t_main; tt < t; ++tt) {
    const float a = bf16_to_f32(dy[tt * ld_dy + r]);
    const bf16x4 xb = *reinterpret_cast<const bf16x4*>(x + tt * ld_x + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = fmaf(a, (float)xb[e], s[e]);
  }
  *reinterpret_cast<f32x4*>(out + r * ld_out + c) = s;
}

}  // namespace gmlm

using namespace gmlm;

namespace {
int wgrad_splits(int64_t t, int64_t n, int64_t k, int splits) {
  const int64_t tiles = (n / wg::TILE) * (k / wg::TILE), stages = t / wg::BT;
  int64_t s = splits > 0 ? splits : 256 / tiles;                 // about one round of the 256 CUs: 36 x 7, 27 x 9, 9 x 28
  if (s < 1) s = 1;
  if (s > stages) s = stages;
  return (int)s;
}
}  // namespace

extern "C" size_t gmlm_wgrad_workspace_bytes(int64_t t, int64_t n, int64_t k, int splits) {
  if (t < wg::BT || n <= 0 || k <= 0) return 0;
  return (size_t)wgrad_splits(t, n, k, splits) * (size_t)n * (size_t)k * sizeof(float);
}

extern "C" int gmlm_wgrad_bf16(const void* dy, int64_t ld_dy, const void* x, int64_t ld_x, int64_t t, int64_t n, int64_t k,
                               int splits, float* out, int64_t ld_out, int flags, void* workspace, size_t workspace_bytes,
                               gmlm_stream_t stream) {
  GMLM_REQUIRE(dy && x && out, "wgrad_bf16: null pointer");
  GMLM_REQUIRE(t >= wg::BT && n > 0 && k > 0, "wgrad_bf16: need t >= %d and n, k > 0 (t=%lld n=%lld k=%lld)", wg::BT, (long long)t,
               (long long)n, (long long)k);
  GMLM_REQUIRE(n % wg::TILE == 0 && k % wg::TILE == 0, "wgrad_bf16: n and k must be multiples of %d (n=%lld k=%lld)", wg::TILE,
               (long long)n, (long long)k);
  GMLM_REQUIRE(ld_dy >= n && ld_x >= k && ld_out >= k, "wgrad_bf16: row stride smaller than the row");
  GMLM_REQUIRE(ld_dy % 8 == 0 && ld_x % 8 == 0 && ld_out % 4 == 0, "wgrad_bf16: row strides must keep rows 16-byte aligned");
  GMLM_REQUIRE(((uintptr_t)dy | (uintptr_t)x | (uintptr_t)out | (uintptr_t)workspace) % 16 == 0,
               "wgrad_bf16: pointers must be 16-byte aligned");
  GMLM_REQUIRE(splits >= 0 && (flags & ~(GMLM_WGRAD_NO_REMAP | GMLM_WGRAD_ONE_PHASE)) == 0, "wgrad_bf16: bad splits / flags");
  // the LDS-DMA source offset of a lane is 32-bit: 16 rows of either operand must stay below 4 GiB
  GMLM_REQUIRE(ld_dy < (1ll << 26) && ld_x < (1ll << 26), "wgrad_bf16: row stride too large");
  const int s = wgrad_splits(t, n, k, splits);
  const size_t need = (size_t)s * (size_t)n * (size_t)k * sizeof(float);
  if (!workspace || workspace_bytes < need) {
    set_error("wgrad_bf16: workspace of %zu bytes, need %zu", workspace_bytes, need);
    return GMLM_EWORKSPACE;
  }
  const int64_t tiles_k = k / wg::TILE, tiles = (n / wg::TILE) * tiles_k, stages = t / wg::BT;
  GMLM_REQUIRE(tiles * s < (1ll << 31) && stages < (1ll << 31), "wgrad_bf16: problem too large");
  static std::once_flag once;
  static hipError_t attr = hipSuccess;
  std::call_once(once, [] {
    attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_bf16_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               wg::LDS);
    if (attr == hipSuccess)
      attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&wgrad_bf16_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 wg::LDS);
  });
  GMLM_HIP(attr);
  hipStream_t st = as_stream(stream);
  WgradParams p{(const bf16_t*)dy, (const bf16_t*)x, (float*)workspace, ld_dy, ld_x, n, k, (int32_t)stages, s, (int32_t)tiles_k,
                (int32_t)tiles, (flags & GMLM_WGRAD_NO_REMAP) ? 0 : 1};
  if (flags & GMLM_WGRAD_ONE_PHASE) wgrad_bf16_kernel<false><<<(unsigned)(tiles * s), wg::NW * 64, wg::LDS, st>>>(p);
  else wgrad_bf16_kernel<true><<<(unsigned)(tiles * s), wg::NW * 64, wg::LDS, st>>>(p);
  GMLM_LAUNCH_CHECK();
  const int64_t items = n * (k / 4);
  wgrad_combine_kernel<<<(unsigned)((items + 255) / 256), 256, 0, st>>>((const float*)workspace, s, n, k, (const bf16_t*)dy, ld_dy,
                                                                      (const bf16_t*)x, ld_x, stages * wg::BT, t, out, ld_out);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
