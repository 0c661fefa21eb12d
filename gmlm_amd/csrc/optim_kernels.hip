// Gradient clipping + AdamW as one multi-tensor step (include/gmlm_hip_optim.h): three launches on one stream,
//   sumsq (one fp32 partial and one non-finite flag per chunk) -> finalize (norm, clip coefficient, skip, step counters, bias
//   corrections) -> update (p, m, v), no host synchronisation, no atomics, no allocation.
// 32 bytes per parameter: g read twice, p / m / v read and written once.  The gradient is never written.
#include "common.hpp"
#include "../../include/gmlm_hip_optim.h"

namespace gmlm {
namespace optim {

constexpr int64_t kChunk = 32768;  // elements per chunk = per workgroup: 128 KiB of each array, 32 float4 per lane
constexpr int kThreads = 256;

// 16 bytes per lane with DWORD alignment: global_load_dwordx4 / global_store_dwordx4 need no more than that, so a tensor that
// is a view into a larger buffer (4-byte aligned) takes the same instructions as an aligned one - and, which is the point,
// the same element -> lane assignment: the fixed summation order below does not depend on where the tensor starts.
typedef float f32x4u __attribute__((ext_vector_type(4)));
// The tensors come out of an address table: as integers their address space is unknown to the compiler (flat_load / flat_store);
// said to be global, they are global_load_dwordx4 / global_store_dwordx4.
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4u __attribute__((aligned(4))) gf32x4u;
__device__ __forceinline__ gf32* as_global(uint64_t a) { return reinterpret_cast<gf32*>(a); }
__device__ __forceinline__ f32x4u ld4(const gf32* p) { return *reinterpret_cast<const gf32x4u*>(p); }
__device__ __forceinline__ void st4(gf32* p, f32x4u v) { *reinterpret_cast<gf32x4u*>(p) = v; }

struct Status {  // the 32-byte status block of the header
  float norm, coef;
  int skip, bad_table, skipped_steps, unused[3];
};

struct Chunk {
  int64_t t, off, len;  // tensor, first element, elements (1 .. kChunk)
};
__device__ __forceinline__ Chunk chunk_of(const int* __restrict__ chunks, const int64_t* __restrict__ numel) {
  Chunk c;
  c.t = chunks[2 * (int64_t)blockIdx.x];
  c.off = (int64_t)chunks[2 * (int64_t)blockIdx.x + 1] * kChunk;
  const int64_t left = numel[c.t] - c.off;
  c.len = left < kChunk ? left : kChunk;
  return c;
}

__device__ __forceinline__ void sq_acc(float x, float& acc, uint32_t& mag) {
  acc = fmaf(x, x, acc);
  const uint32_t a = __float_as_uint(x) & 0x7fffffffu;
  mag = a > mag ? a : mag;  // the largest |x| as an integer: >= 0x7f800000 <=> an infinity or a NaN was seen
}

// ---- a. sum of squares per chunk ---------------------------------------------------------------------------------------
// Order of the sum, the same on every call and for every alignment: lane i takes vectors i, i + 256, i + 512, ... of the chunk,
// even rounds into acc0 and odd rounds into acc1 (two 16-byte loads in flight), then acc0 + acc1, then the tail element (len % 4
// of them, one each on lanes 0..2), then the wave butterfly, then the four wave sums in wave order.
__global__ __launch_bounds__(kThreads) void sumsq_kernel(const uint64_t* __restrict__ addr, const int64_t* __restrict__ numel,
                                                         const int* __restrict__ chunks, float* __restrict__ partial,
                                                         int* __restrict__ nonfinite) {
  const Chunk c = chunk_of(chunks, numel);
  const gf32* g = as_global(addr[4 * c.t + 1]) + c.off;
  const int len = (int)c.len, nvec = len >> 2, tid = threadIdx.x;
  float acc0 = 0.f, acc1 = 0.f;
  uint32_t mag = 0;
  int i = tid;
  for (; i + kThreads < nvec; i += 2 * kThreads) {
    const f32x4u a = ld4(g + 4 * i), b = ld4(g + 4 * (i + kThreads));
    sq_acc(a.x, acc0, mag); sq_acc(a.y, acc0, mag); sq_acc(a.z, acc0, mag); sq_acc(a.w, acc0, mag);
    sq_acc(b.x, acc1, mag); sq_acc(b.y, acc1, mag); sq_acc(b.z, acc1, mag); sq_acc(b.w, acc1, mag);
  }
  if (i < nvec) {
    const f32x4u a = ld4(g + 4 * i);
    sq_acc(a.x, acc0, mag); sq_acc(a.y, acc0, mag); sq_acc(a.z, acc0, mag); sq_acc(a.w, acc0, mag);
  }
  float acc = acc0 + acc1;
  if (4 * nvec + tid < len) sq_acc(g[4 * nvec + tid], acc, mag);
  acc = wave_sum(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t other = (uint32_t)__shfl_xor((int)mag, o, 64);
    mag = other > mag ? other : mag;
  }
  __shared__ float s_sum[kThreads / kWave];
  __shared__ uint32_t s_mag[kThreads / kWave];
  if ((tid & (kWave - 1)) == 0) {
    s_sum[tid / kWave] = acc;
    s_mag[tid / kWave] = mag;
  }
  __syncthreads();
  if (tid == 0) {
    float s = s_sum[0];
    uint32_t m = s_mag[0];
#pragma unroll
    for (int w = 1; w < kThreads / kWave; ++w) {
      s += s_sum[w];
      m = s_mag[w] > m ? s_mag[w] : m;
    }
    partial[blockIdx.x] = s;
    nonfinite[blockIdx.x] = m >= 0x7f800000u ? 1 : 0;
  }
}

// ---- b. finalize ---------------------------------------------------------------------------------------------------------
// One workgroup.  Index order in double: lane i adds its contiguous run of partials in ascending order, lane 0 then adds the
// 256 run sums in lane order.
__global__ __launch_bounds__(kThreads) void finalize_kernel(const float* __restrict__ partial, const int* __restrict__ nonfinite,
                                                            int num_chunks, float max_norm, const int* __restrict__ group,
                                                            const int* __restrict__ slot, int num_tensors,
                                                            const double* __restrict__ hyper, int num_groups,
                                                            int* __restrict__ steps, int num_slots, float* __restrict__ bias_corr,
                                                            Status* __restrict__ status) {
  __shared__ double s_run[kThreads];
  __shared__ int s_skip;
  const int tid = threadIdx.x;
  const int64_t per = ((int64_t)num_chunks + kThreads - 1) / kThreads;
  const int64_t lo = tid * per < num_chunks ? tid * per : num_chunks;
  const int64_t hi = lo + per < num_chunks ? lo + per : num_chunks;
  double run = 0.0;
  int bad_grad = 0, bad_table = 0;
  for (int64_t n = lo; n < hi; ++n) {
    run += (double)partial[n];
    bad_grad |= nonfinite[n];
  }
  for (int t = tid; t < num_tensors; t += kThreads)
    bad_table |= (group[t] < 0 || group[t] >= num_groups || slot[t] < 0 || slot[t] >= num_slots) ? 1 : 0;
  s_run[tid] = run;
  bad_grad = __syncthreads_or(bad_grad);    // also the barrier behind the s_run writes
  bad_table = __syncthreads_or(bad_table);
  if (tid == 0) {
    double sum = 0.0;
    for (int i = 0; i < kThreads; ++i) sum += s_run[i];
    const double norm = sqrt(sum);
    const double mx = (double)max_norm;
    double coef = 1.0;
    if (mx > 0.0 && isfinite(mx)) {
      coef = mx / (norm + 1e-6);
      coef = coef < 1.0 ? coef : 1.0;     // NaN (norm not finite) stays out: the step is skipped then
    }
    const int skip = (bad_grad || bad_table || !isfinite(norm)) ? 1 : 0;
    status->norm = (float)norm;
    status->coef = (float)coef;
    status->skip = skip;
    status->bad_table = bad_table;
    if (skip) status->skipped_steps += 1;
    s_skip = skip;
  }
  __syncthreads();
  if (s_skip) return;
  for (int t = tid; t < num_tensors; t += kThreads) {
    const int s = steps[slot[t]] + 1;
    steps[slot[t]] = s;
    const double* h = hyper + 8 * (int64_t)group[t];
    bias_corr[2 * t] = (float)(1.0 - pow(h[2], (double)s));
    bias_corr[2 * t + 1] = (float)sqrt(1.0 - pow(h[3], (double)s));
  }
}

// ---- c. update --------------------------------------------------------------------------------------------------------------
struct Coef {  // per workgroup, from status, the tensor's bias corrections and its group row
  float clip, decay, omb1, beta2, omb2, neg_step, bc2s, eps;
};

// One element of torch's decoupled AdamW in fp32.  Contraction is off: every rounding is the one written here (the two fmaf
// are meant), so the vector body and the tail give the same bits; / and sqrtf are correctly rounded (hipcc's default).
__device__ __forceinline__ void adamw_elem(const Coef& k, float g, float& p, float& m, float& v) {
#pragma clang fp contract(off)
  const float gs = k.clip * g;
  const float pd = p * k.decay;
  m = fmaf(gs - m, k.omb1, m);
  const float v_decayed = k.beta2 * v;
  v = fmaf(k.omb2 * gs, gs, v_decayed);
  const float denom = sqrtf(v) / k.bc2s + k.eps;
  p = fmaf(k.neg_step, m / denom, pd);
}
__device__ __forceinline__ void adamw_vec(const Coef& k, f32x4u g, f32x4u& p, f32x4u& m, f32x4u& v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float pj = p[j], mj = m[j], vj = v[j];
    adamw_elem(k, g[j], pj, mj, vj);
    p[j] = pj; m[j] = mj; v[j] = vj;
  }
}

__global__ __launch_bounds__(kThreads) void update_kernel(const uint64_t* __restrict__ addr, const int64_t* __restrict__ numel,
                                                          const int* __restrict__ group, const int* __restrict__ chunks,
                                                          const double* __restrict__ hyper, const float* __restrict__ bias_corr,
                                                          const Status* __restrict__ status) {
  if (status->skip) return;  // the same word for every workgroup: nothing is touched by a skipped step
  const Chunk c = chunk_of(chunks, numel);
  // p, g, m, v may not overlap (header), but they come out of a table: no __restrict__, every load of a round before its stores
  gf32* p = as_global(addr[4 * c.t]) + c.off;
  const gf32* g = as_global(addr[4 * c.t + 1]) + c.off;
  gf32* m = as_global(addr[4 * c.t + 2]) + c.off;
  gf32* v = as_global(addr[4 * c.t + 3]) + c.off;
  const double* h = hyper + 8 * (int64_t)group[c.t];
  const double lr = h[0], wd = h[1], b1 = h[2], b2 = h[3];
  Coef k;
  k.clip = status->coef;
  k.decay = (float)(1.0 - lr * wd);
  k.omb1 = (float)(1.0 - b1);
  k.beta2 = (float)b2;
  k.omb2 = (float)(1.0 - b2);
  k.neg_step = (float)(-(lr / (double)bias_corr[2 * c.t]));
  k.bc2s = bias_corr[2 * c.t + 1];
  k.eps = (float)h[4];
  const int len = (int)c.len, nvec = len >> 2, tid = threadIdx.x;
  int i = tid;
  for (; i + kThreads < nvec; i += 2 * kThreads) {
    const int j = i + kThreads;
    const f32x4u g0 = ld4(g + 4 * i), g1 = ld4(g + 4 * j);
    f32x4u p0 = ld4(p + 4 * i), p1 = ld4(p + 4 * j);
    f32x4u m0 = ld4(m + 4 * i), m1 = ld4(m + 4 * j);
    f32x4u v0 = ld4(v + 4 * i), v1 = ld4(v + 4 * j);
    adamw_vec(k, g0, p0, m0, v0);
    adamw_vec(k, g1, p1, m1, v1);
    st4(p + 4 * i, p0); st4(m + 4 * i, m0); st4(v + 4 * i, v0);
    st4(p + 4 * j, p1); st4(m + 4 * j, m1); st4(v + 4 * j, v1);
  }
  if (i < nvec) {
    const f32x4u g0 = ld4(g + 4 * i);
    f32x4u p0 = ld4(p + 4 * i), m0 = ld4(m + 4 * i), v0 = ld4(v + 4 * i);
    adamw_vec(k, g0, p0, m0, v0);
    st4(p + 4 * i, p0); st4(m + 4 * i, m0); st4(v + 4 * i, v0);
  }
  const int e = 4 * nvec + tid;
  if (e < len) {
    float pe = p[e], me = m[e], ve = v[e];
    adamw_elem(k, g[e], pe, me, ve);
    p[e] = pe; m[e] = me; v[e] = ve;
  }
}

}  // namespace optim
}  // namespace gmlm

using namespace gmlm;

#define OPTIM_TABLE(ptr)                                                                             \
  GMLM_REQUIRE((ptr) != nullptr, "%s: null pointer (%s)", who, #ptr);                                \
  GMLM_REQUIRE(aligned16(ptr), "%s: %s must be 16-byte aligned", who, #ptr)

#define OPTIM_COUNT(n) GMLM_REQUIRE((n) >= 0, "%s: negative count (%s = %ld)", who, #n, (long)(n))

#define OPTIM_CHUNKS(n)      \
  OPTIM_COUNT(n);            \
  GMLM_REQUIRE((n) < ((int64_t)1 << 31), "%s: num_chunks %ld must be below 2^31", who, (long)(n))

extern "C" int64_t gmlm_adamw_chunk_elems(void) { return optim::kChunk; }

extern "C" int gmlm_adamw_sumsq(const void* addr, const int64_t* numel, const int* chunks, int64_t num_chunks, float* partial,
                                int* nonfinite, gmlm_stream_t stream) {
  static const char* who = "adamw_sumsq";
  OPTIM_CHUNKS(num_chunks);
  if (num_chunks == 0) return GMLM_OK;
  OPTIM_TABLE(addr);
  OPTIM_TABLE(numel);
  OPTIM_TABLE(chunks);
  OPTIM_TABLE(partial);
  OPTIM_TABLE(nonfinite);
  optim::sumsq_kernel<<<(unsigned)num_chunks, optim::kThreads, 0, as_stream(stream)>>>(static_cast<const uint64_t*>(addr), numel,
                                                                                       chunks, partial, nonfinite);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" int gmlm_adamw_finalize(const float* partial, const int* nonfinite, int64_t num_chunks, float max_norm,
                                   const int* group, const int* slot, int64_t num_tensors, const double* hyper,
                                   int64_t num_groups, int* steps, int64_t num_slots, float* bias_corr, void* status,
                                   gmlm_stream_t stream) {
  static const char* who = "adamw_finalize";
  OPTIM_CHUNKS(num_chunks);
  OPTIM_COUNT(num_tensors);
  OPTIM_COUNT(num_groups);
  OPTIM_COUNT(num_slots);
  GMLM_REQUIRE(num_tensors <= num_chunks, "%s: num_tensors %ld exceeds num_chunks %ld (every tensor has a chunk)", who,
               (long)num_tensors, (long)num_chunks);
  GMLM_REQUIRE(num_tensors <= num_slots, "%s: num_tensors %ld exceeds num_slots %ld", who, (long)num_tensors, (long)num_slots);
  GMLM_REQUIRE(num_groups > 0 || num_tensors == 0, "%s: num_groups is 0 with %ld tensors", who, (long)num_tensors);
  GMLM_REQUIRE(num_groups < ((int64_t)1 << 31) && num_slots < ((int64_t)1 << 31), "%s: num_groups %ld / num_slots %ld must be below 2^31",
               who, (long)num_groups, (long)num_slots);
  if (num_chunks == 0 || num_tensors == 0) return GMLM_OK;
  OPTIM_TABLE(partial);
  OPTIM_TABLE(nonfinite);
  OPTIM_TABLE(group);
  OPTIM_TABLE(slot);
  OPTIM_TABLE(hyper);
  OPTIM_TABLE(steps);
  OPTIM_TABLE(bias_corr);
  OPTIM_TABLE(status);
  optim::finalize_kernel<<<1, optim::kThreads, 0, as_stream(stream)>>>(partial, nonfinite, (int)num_chunks, max_norm, group, slot,
                                                                       (int)num_tensors, hyper, (int)num_groups, steps,
                                                                       (int)num_slots, bias_corr, static_cast<optim::Status*>(status));
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" int gmlm_adamw_update(const void* addr, const int64_t* numel, const int* group, const int* chunks, int64_t num_chunks,
                                 const double* hyper, int64_t num_groups, const float* bias_corr, const void* status,
                                 gmlm_stream_t stream) {
  static const char* who = "adamw_update";
  OPTIM_CHUNKS(num_chunks);
  OPTIM_COUNT(num_groups);
  GMLM_REQUIRE(num_groups > 0 || num_chunks == 0, "%s: num_groups is 0 with %ld chunks", who, (long)num_chunks);
  if (num_chunks == 0) return GMLM_OK;
  OPTIM_TABLE(addr);
  OPTIM_TABLE(numel);
  OPTIM_TABLE(group);
  OPTIM_TABLE(chunks);
  OPTIM_TABLE(hyper);
  OPTIM_TABLE(bias_corr);
  OPTIM_TABLE(status);
  optim::update_kernel<<<(unsigned)num_chunks, optim::kThreads, 0, as_stream(stream)>>>(
      static_cast<const uint64_t*>(addr), numel, group, chunks, hyper, bias_corr, static_cast<const optim::Status*>(status));
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
