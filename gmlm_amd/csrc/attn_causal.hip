// Causal attention with grouped KV heads at head dim 128, forward + backward, gfx950 MFMA (gmlm_attention_causal_d128_*):
// the self-attention of a Qwen3-geometry text encoder (hq query heads share hkv KV heads, query i sees keys 0..i of its own
// sequence and, of those, the ones below kv_len).  Padded layout [b, l, heads, 128] with per-operand row strides, so the
// fused [q | k | v] projection output is read (and its gradient written) without copies; or packed layout [T, heads, 128]
// (gmlm_attention_causal_d128_varlen_*): the same kernels with AttnParams::cu set, sequence i = rows [cu[i], cu[i + 1]).
// Forward and dQ ARE the streaming bodies of attn_stream.hpp, instantiated with their CAUSAL and GQA template flags (defaults
// false: the existing kernels' code objects are unchanged, profiles/attn_causal_static.json) at the tiling of attn_d128.hip
// (4 waves, 128 query rows per workgroup, bf16: 64-row K / V tiles double-buffered, fp32: 32-row tiles in one buffer); delta is
// the shared delta body.  dK/dV has a loop nest of its own (an outer loop over the query heads of a KV head, a start tile, a
// barrier between heads), written on the helpers of attn_common.hpp in attn_causal_dkv.hpp (DESIGN.md section 4 "Qwen3 encoder").
//  * tiles wholly below the diagonal take the compare-free path of the non-causal kernels (block- or wave-uniform test);
//    only tiles that touch the diagonal compare key <= query per element (and key < kv_len);
//  * every wave reaches every barrier: a wave whose rows lie above a tile still stages K / V;
//  * key 0 is valid for every query and a wave only computes tiles whose first key is <= its first query, so every row of a
//    computing wave has a valid key in every tile it computes: the running max is finite, -inf - (-inf) never occurs;
//  * bf16 backward: lse, delta and the kv_len mask ride in one extra contraction step as in the non-causal kernels; the
//    causal mask is not rank-1, so diagonal tiles select P = 0 explicitly before dS;
//  * dK/dV: a workgroup owns 128 keys of one KV head, walks the query heads of its group in order and, per head, the query
//    tiles from the diagonal on, accumulating into the same registers.  No atomics, no expanded K / V or dK / dV in HBM.
// The argument checks and the AttnParams filling shared with the other attention entry points are in attn_host.hpp.
#include "attn_stream.hpp"
#include "attn_causal_dkv.hpp"
#include "attn_host.hpp"

namespace gmlm {
namespace causal128 {

constexpr int D = 128, NW = 4, NT = NW * 64, BQ = NW * 32;

struct Params {
  AttnParams a;            // a.h = query heads; lse / delta are [b, hq, l]; a.lq == a.lk
  int64_t dout_stride;     // row stride of dO / O (= hq * 128)
  int32_t group;           // query heads per KV head (hq / hkv)
};

template <typename T> struct Cfg;
template <> struct Cfg<bf16_t> { static constexpr int KT = 64, QT = 32; static constexpr bool DBUF = true; };
template <> struct Cfg<float> { static constexpr int KT = 32, QT = 32; static constexpr bool DBUF = false; };

__device__ __forceinline__ int64_t clamp_kvlen(const AttnParams& p, int64_t b, int64_t lk_) {
  int64_t kvlen = lk_;
  if (p.kv_len) { kvlen = p.kv_len[b]; if (kvlen > lk_) kvlen = lk_; if (kvlen < 0) kvlen = 0; }
  return kvlen;
}

// work item of the 1-D grid -> (tile, batch, query head); tiles are outermost
struct Item { int64_t tile, b, hd; };
__device__ __forceinline__ Item decode(const AttnParams& p) {
  const int64_t pairs = p.b * p.h, item = blockIdx.x;
  const int64_t bh = item % pairs;
  return {item / pairs, bh / p.h, bh % p.h};
}

// forward: workgroup = 128 query rows of one (batch, query head); key tiles 0 .. the tile holding its last query
template <typename T>
__global__ __launch_bounds__(NT) void fwd_kernel(Params x) {
  const Item it = decode(x.a);
  attn_fwd_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, true, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

// backward: delta = rowsum(dO * O) over rows of [b * l, hq, 128]
template <typename T>
__global__ __launch_bounds__(256) void delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                    int64_t rows /* b * l * hq */, int64_t lq, int64_t hn, float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);
}

// backward: dQ.  workgroup = 128 queries of one (batch, query head), key tiles up to the diagonal.  Without dropout the shared
// body keeps its register budget at D = 128 (d128::dq_kernel's own copy exists for the dropout instantiation).
template <typename T>
__global__ __launch_bounds__(NT) void dq_kernel(Params x) {
  const Item it = decode(x.a);
  attn_dq_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, true, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

// backward: dK, dV.  workgroup = 128 keys (32 per wave) of one (batch, KV head); for each query head of the group, in order,
// the query tiles of 32 from the one holding the workgroup's first key to the end of the sequence.  The loop nest is
// causal_dkv_body (attn_causal_dkv.hpp), shared with the d = 64 family of attn_gqa.hip.
template <typename T>
__global__ __launch_bounds__(NT) void dkv_kernel(Params x) {
  const CausalKeyTile it = causal_key_tile(x.a, x.group);
  causal_dkv_body<T, D, NW, Cfg<T>::QT, Cfg<T>::DBUF>(x.a, x.dout_stride, x.group, it, clamp_kvlen(x.a, it.b, it.l));
}

// the checks of attn_host.hpp up to the empty-problem return, with this family's head dim, layout rules and work-item bound;
// fills the launch parameters.  sizes_ok: what the entry point adds to the size test (the varlen entries' own bounds)
static int setup(const char* who, Params& x, const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b,
                 int64_t hq, int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                 float scale, float dropout_p, const void* out_lo, int dtype, bool sizes_ok = true) {
  int rc = attn_check_shape(who, sizes_ok && b >= 0 && hq > 0 && hkv > 0 && lq >= 0 && lk >= 0, d == 128, d, "this entry point takes 128",
                            dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(lq == lk, "%s: causal self-attention needs lq == lk (got %ld and %ld)", who, (long)lq, (long)lk);
  GMLM_REQUIRE(hq % hkv == 0, "%s: %ld query heads are not a multiple of %ld KV heads", who, (long)hq, (long)hkv);
  if ((rc = attn_check_rates(who, dropout_p, false, scale)) != GMLM_OK) return rc;
  GMLM_REQUIRE(lq < ((int64_t)1 << 30) && cdiv(lq, BQ) * b * hq < ((int64_t)1 << 31), "%s: too many work items", who);
  x = Params{};
  attn_fill(x.a, q, k, v, kv_len, b, hq, lq, lk, q_stride, k_stride, v_stride, scale, 0.f, 0, nullptr);
  x.dout_stride = hq * D;
  x.group = (int32_t)(hq / hkv);
  return GMLM_OK;
}

// packed (varlen) layout: `seqs` sequences, sequence i = rows [cu[i], cu[i + 1]) of `rows` packed rows, none longer than
// max_len.  Same kernels with AttnParams::cu set: b = seqs, lq = lk = rows (lse / delta [hq, rows]); a tile past its
// sequence returns block-uniformly.
static int setup_varlen(const char* who, Params& x, const void* q, const void* k, const void* v, const int32_t* cu, int64_t seqs,
                        int64_t max_len, int64_t rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride, int64_t k_stride,
                        int64_t v_stride, float scale, float dropout_p, const void* out_lo, int dtype) {
  GMLM_REQUIRE(cu, "%s: null cu_seqlens", who);
  GMLM_REQUIRE(max_len > 0, "%s: max_len %ld must be positive", who, (long)max_len);
  GMLM_REQUIRE(seqs >= 0 && rows >= 0 && rows < ((int64_t)1 << 30), "%s: %ld packed rows (must be >= 0 and < 2^30)", who, (long)rows);
  int rc = setup(who, x, q, k, v, nullptr, 0, hq, hkv, 0, 0, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype,
                 max_len < ((int64_t)1 << 30) && seqs < ((int64_t)1 << 30));
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(cdiv(max_len, BQ) * seqs * hq < ((int64_t)1 << 31), "%s: too many work items", who);
  x.a.b = seqs; x.a.lq = x.a.lk = rows; x.a.cu = cu;
  return GMLM_OK;
}

}  // namespace causal128
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::causal128;

#define GMLM_CAUSAL_LAUNCH(KERNEL, grid, st, prm)                         \
  do {                                                                    \
    if (dtype == GMLM_BF16) KERNEL<bf16_t><<<grid, NT, 0, st>>>(prm);     \
    else KERNEL<float><<<grid, NT, 0, st>>>(prm);                         \
  } while (0)

extern "C" int gmlm_attention_causal_d128_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b,
                                              int64_t hq, int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride,
                                              int64_t k_stride, int64_t v_stride, float scale, float dropout_p, void* out,
                                              void* out_lo, float* lse, int dtype, gmlm_stream_t stream) {
  static const char* who = "attention_causal_d128_fwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, hq, hkv, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, hq * D, hkv * D, dtype)) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(cdiv(lq, BQ) * b * hq));
  GMLM_CAUSAL_LAUNCH(fwd_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_causal_d128_workspace_bytes(int64_t b, int64_t hq, int64_t lq) {
  return attn_delta_bytes(b, hq, lq);
}

extern "C" int gmlm_attention_causal_d128_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                              const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq,
                                              int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                              int64_t v_stride, float scale, float dropout_p, void* dq, void* dk, void* dv,
                                              int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                              size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "attention_causal_d128_bwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, hq, hkv, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  AttnParams& p = x.a;
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, p, hq * D, hkv * D, dtype, workspace_bytes, attn_delta_bytes(b, hq, lq))) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t rows = b * lq * hq;
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, rows, dtype == GMLM_BF16 ? 16 : 32, st, lq, hq);
  GMLM_LAUNCH_CHECK();
  const dim3 gq((unsigned)(cdiv(lq, BQ) * b * hq));
  GMLM_CAUSAL_LAUNCH(dq_kernel, gq, st, x);
  GMLM_LAUNCH_CHECK();
  const dim3 gk((unsigned)(cdiv(lk, BQ) * b * hkv));
  GMLM_CAUSAL_LAUNCH(dkv_kernel, gk, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" int gmlm_attention_causal_d128_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                                     int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq,
                                                     int64_t hkv, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                                     float scale, float dropout_p, void* out, void* out_lo, float* lse, int dtype,
                                                     gmlm_stream_t stream) {
  static const char* who = "attention_causal_d128_varlen_fwd";
  Params x;
  int rc = setup_varlen(who, x, q, k, v, cu_seqlens, num_seqs, max_len, total_rows, hq, hkv, d, q_stride, k_stride, v_stride, scale,
                        dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (num_seqs == 0 || total_rows == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, hq * D, hkv * D, dtype)) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(cdiv(max_len, BQ) * num_seqs * hq));
  GMLM_CAUSAL_LAUNCH(fwd_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_causal_d128_varlen_workspace_bytes(int64_t total_rows, int64_t hq) {
  return attn_delta_bytes(1, hq, total_rows);   // delta [hq, total_rows]
}

extern "C" int gmlm_attention_causal_d128_varlen_bwd(const void* q, const void* k, const void* v, const void* out,
                                                     const void* out_lo, const void* dout, const float* lse,
                                                     const int32_t* cu_seqlens, int64_t num_seqs, int64_t max_len,
                                                     int64_t total_rows, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride,
                                                     int64_t k_stride, int64_t v_stride, float scale, float dropout_p, void* dq,
                                                     void* dk, void* dv, int64_t dq_stride, int64_t dk_stride, int64_t dv_stride,
                                                     int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "attention_causal_d128_varlen_bwd";
  Params x;
  int rc = setup_varlen(who, x, q, k, v, cu_seqlens, num_seqs, max_len, total_rows, hq, hkv, d, q_stride, k_stride, v_stride, scale,
                        dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (num_seqs == 0 || total_rows == 0) return GMLM_OK;
  AttnParams& p = x.a;
  attn_fill_bwd(p, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, p, hq * D, hkv * D, dtype, workspace_bytes, attn_delta_bytes(1, hq, total_rows))) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const int64_t rows = total_rows * hq;                         // delta as one sequence of total_rows: [hq, total_rows]
  GMLM_ATTN_DELTA_LAUNCH(delta_kernel, p, rows, dtype == GMLM_BF16 ? 16 : 32, st, total_rows, hq);
  GMLM_LAUNCH_CHECK();
  const dim3 gq((unsigned)(cdiv(max_len, BQ) * num_seqs * hq));
  GMLM_CAUSAL_LAUNCH(dq_kernel, gq, st, x);
  GMLM_LAUNCH_CHECK();
  const dim3 gk((unsigned)(cdiv(max_len, BQ) * num_seqs * hkv));
  GMLM_CAUSAL_LAUNCH(dkv_kernel, gk, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}
