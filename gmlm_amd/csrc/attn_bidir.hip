// Bidirectional (non-causal) self-attention with grouped KV heads at head dim 64 and 128, forward + backward, gfx950 MFMA
// (gmlm_attention_bidir_gqa_*, C ABI in include/gmlm_hip_bidir.h), all in namespace gmlm::bidir: the attention of a EuroBERT
// text encoder (the Llama layer without the causal mask).  Padded layout [b, l, heads, d] with per-operand row strides, so the
// fused [q | k | v] projection output is read (and its gradient written) without copies; or packed layout [T, heads, d]: the
// same kernels with AttnParams::cu set, sequence i = rows [cu[i], cu[i + 1]).
// Forward and dQ ARE the streaming bodies of attn_stream.hpp with CAUSAL = false, GQA = true: the key loop runs over all key
// tiles below the sequence's kv_len.  delta is the shared delta body.  dK/dV is causal_dkv_body (attn_causal_dkv.hpp) with
// CAUSAL = false: a workgroup owns 128 keys of one (sequence, KV head) and, for each query head of the group in order, walks
// ALL query tiles of the sequence, accumulating into the same registers.  No atomics, no expanded K / V or dK / dV in HBM.
// Tiling of causal128:: / gqa::causal64_* (4 waves, 128 query rows; bf16: 64-key tiles double-buffered, fp32: 32-key tiles in
// one buffer; 1-D grids), for both head dims (DESIGN.md section 4 "EuroBERT and NomicBERT encoders").
#include "attn_stream.hpp"
#include "attn_causal_dkv.hpp"
#include "attn_host.hpp"
#include "../../include/gmlm_hip_bidir.h"

namespace gmlm {
namespace bidir {

constexpr int NW = 4, NT = NW * 64, BQ = NW * 32;

struct Params {
  AttnParams a;            // a.h = query heads; lse / delta are [b, hq, l]; a.lq == a.lk
  int64_t dout_stride;     // row stride of dO / O (= hq * d)
  int32_t group;           // query heads per KV head (hq / hkv)
};

template <typename T> struct Cfg;
template <> struct Cfg<bf16_t> { static constexpr int KT = 64, QT = 32; static constexpr bool DBUF = true; };
template <> struct Cfg<float> { static constexpr int KT = 32, QT = 32; static constexpr bool DBUF = false; };

// work item of the 1-D grid -> (tile, batch, query head); tiles are outermost
struct Item { int64_t tile, b, hd; };
__device__ __forceinline__ Item decode(const AttnParams& p) {
  const int64_t pairs = p.b * p.h, item = blockIdx.x;
  const int64_t bh = item % pairs;
  return {item / pairs, bh / p.h, bh % p.h};
}

template <typename T, int D>
__global__ __launch_bounds__(NT) void gqa_fwd_kernel(Params x) {
  const Item it = decode(x.a);
  attn_fwd_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, false, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

// delta = rowsum(dO * O) over rows of [b * l, hq, D]
template <typename T, int D>
__global__ __launch_bounds__(256) void gqa_delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo, const T* __restrict__ dout,
                                                        int64_t rows /* b * l * hq */, int64_t lq, int64_t hn,
                                                        float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);
}

template <typename T, int D>
__global__ __launch_bounds__(NT) void gqa_dq_kernel(Params x) {
  const Item it = decode(x.a);
  attn_dq_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, false, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

template <typename T, int D>
__global__ __launch_bounds__(NT) void gqa_dkv_kernel(Params x) {
  const CausalKeyTile it = causal_key_tile(x.a, x.group);
  int64_t kvlen = it.l;                                      // kv_len clamped into [0, l], as the streaming bodies do
  if (x.a.kv_len) { kvlen = x.a.kv_len[it.b]; if (kvlen > it.l) kvlen = it.l; if (kvlen < 0) kvlen = 0; }
  causal_dkv_body<T, D, NW, Cfg<T>::QT, Cfg<T>::DBUF, false>(x.a, x.dout_stride, x.group, it, kvlen);
}

// the checks of attn_host.hpp up to the empty-problem return, in the order of the causal families; fills the launch parameters
static int setup(const char* who, Params& x, const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b,
                 int64_t hq, int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                 float scale, float dropout_p, const void* out_lo, int dtype, bool sizes_ok = true) {
  int rc = attn_check_shape(who, sizes_ok && b >= 0 && hq > 0 && hkv > 0 && lq >= 0 && lk >= 0, d == 64 || d == 128, d,
                            "this entry point takes 64 or 128", dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(lq == lk, "%s: self-attention needs lq == lk (got %ld and %ld)", who, (long)lq, (long)lk);
  GMLM_REQUIRE(hq % hkv == 0, "%s: %ld query heads are not a multiple of %ld KV heads", who, (long)hq, (long)hkv);
  GMLM_REQUIRE(dropout_p == 0.f, "%s: attention-probability dropout is not implemented for the grouped kernels (dropout_p must be 0)", who);
  GMLM_REQUIRE(scale > 0.f, "%s: scale must be positive", who);
  GMLM_REQUIRE(lq < ((int64_t)1 << 30) && cdiv(lq, BQ) * b * hq < ((int64_t)1 << 31), "%s: too many work items", who);
  x = Params{};
  attn_fill(x.a, q, k, v, kv_len, b, hq, lq, lk, q_stride, k_stride, v_stride, scale, 0.f, 0, nullptr);
  x.dout_stride = hq * d;
  x.group = (int32_t)(hq / hkv);
  return GMLM_OK;
}

// packed layout: the same kernels with AttnParams::cu set: b = seqs, lq = lk = rows (lse / delta [hq, rows])
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

// dispatch on (dtype, d), both validated by setup(): LAUNCH(T, D) is one launch statement
#define GMLM_BIDIR_DISPATCH(LAUNCH)                                                     \
  do {                                                                                  \
    if (dtype == GMLM_BF16) { if (d == 64) LAUNCH(bf16_t, 64); else LAUNCH(bf16_t, 128); } \
    else { if (d == 64) LAUNCH(float, 64); else LAUNCH(float, 128); }                   \
  } while (0)

static int launch_fwd(const Params& x, int64_t tiles, int64_t seqs, int64_t hq, int64_t d, int dtype, hipStream_t st) {
  const dim3 grid((unsigned)(tiles * seqs * hq));
#define GMLM_BIDIR_FWD(T, D_) gqa_fwd_kernel<T, D_><<<grid, NT, 0, st>>>(x)
  GMLM_BIDIR_DISPATCH(GMLM_BIDIR_FWD);
#undef GMLM_BIDIR_FWD
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

// the three backward launches; tiles = query (= key) tiles of 128 per sequence, seqs = sequences, drows / dlq = the delta view
static int launch_bwd(const Params& x, int64_t tiles, int64_t seqs, int64_t hq, int64_t hkv, int64_t d, int64_t drows, int64_t dlq,
                      int dtype, hipStream_t st) {
  const AttnParams& p = x.a;
  // attn_delta_body: d / V lanes per row, rounded up to 8, 16 or 32
  const int64_t lanes = d / (dtype == GMLM_BF16 ? 8 : 4);
  const unsigned gd = (unsigned)cdiv(drows * lanes, (int64_t)256);
  const void* lo = dtype == GMLM_BF16 ? p.out_lo : nullptr;     // only bf16 has an output residual
#define GMLM_BIDIR_DELTA(T, D_) \
  gqa_delta_kernel<T, D_><<<gd, 256, 0, st>>>((const T*)p.out, (const T*)lo, (const T*)p.dout, drows, dlq, hq, p.delta)
  GMLM_BIDIR_DISPATCH(GMLM_BIDIR_DELTA);
#undef GMLM_BIDIR_DELTA
  GMLM_LAUNCH_CHECK();
  const dim3 gq((unsigned)(tiles * seqs * hq));
#define GMLM_BIDIR_DQ(T, D_) gqa_dq_kernel<T, D_><<<gq, NT, 0, st>>>(x)
  GMLM_BIDIR_DISPATCH(GMLM_BIDIR_DQ);
#undef GMLM_BIDIR_DQ
  GMLM_LAUNCH_CHECK();
  const dim3 gk((unsigned)(tiles * seqs * hkv));
#define GMLM_BIDIR_DKV(T, D_) gqa_dkv_kernel<T, D_><<<gk, NT, 0, st>>>(x)
  GMLM_BIDIR_DISPATCH(GMLM_BIDIR_DKV);
#undef GMLM_BIDIR_DKV
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

}  // namespace bidir
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::bidir;

extern "C" int gmlm_attention_bidir_gqa_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                            int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                            int64_t v_stride, float scale, float dropout_p, void* out, void* out_lo, float* lse,
                                            int dtype, gmlm_stream_t stream) {
  static const char* who = "attention_bidir_gqa_fwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, hq, hkv, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, hq * d, hkv * d, dtype)) != GMLM_OK) return rc;
  return launch_fwd(x, cdiv(lq, BQ), b, hq, d, dtype, as_stream(stream));
}

extern "C" size_t gmlm_attention_bidir_gqa_workspace_bytes(int64_t b, int64_t hq, int64_t lq) { return attn_delta_bytes(b, hq, lq); }

extern "C" int gmlm_attention_bidir_gqa_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                            const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq,
                                            int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                            int64_t v_stride, float scale, float dropout_p, void* dq, void* dk, void* dv,
                                            int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                            size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "attention_bidir_gqa_bwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, hq, hkv, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  attn_fill_bwd(x.a, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, x.a, hq * d, hkv * d, dtype, workspace_bytes, attn_delta_bytes(b, hq, lq))) != GMLM_OK) return rc;
  return launch_bwd(x, cdiv(lq, BQ), b, hq, hkv, d, b * lq * hq, lq, dtype, as_stream(stream));
}

extern "C" int gmlm_attention_bidir_gqa_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                                   int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv,
                                                   int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                                   float dropout_p, void* out, void* out_lo, float* lse, int dtype,
                                                   gmlm_stream_t stream) {
  static const char* who = "attention_bidir_gqa_varlen_fwd";
  Params x;
  int rc = setup_varlen(who, x, q, k, v, cu_seqlens, num_seqs, max_len, total_rows, hq, hkv, d, q_stride, k_stride, v_stride, scale,
                        dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (num_seqs == 0 || total_rows == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, hq * d, hkv * d, dtype)) != GMLM_OK) return rc;
  return launch_fwd(x, cdiv(max_len, BQ), num_seqs, hq, d, dtype, as_stream(stream));
}

extern "C" size_t gmlm_attention_bidir_gqa_varlen_workspace_bytes(int64_t total_rows, int64_t hq) {
  return attn_delta_bytes(1, hq, total_rows);   // delta [hq, total_rows]
}

extern "C" int gmlm_attention_bidir_gqa_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                                   const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                                   int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d,
                                                   int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                                   float dropout_p, void* dq, void* dk, void* dv, int64_t dq_stride,
                                                   int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                                   size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "attention_bidir_gqa_varlen_bwd";
  Params x;
  int rc = setup_varlen(who, x, q, k, v, cu_seqlens, num_seqs, max_len, total_rows, hq, hkv, d, q_stride, k_stride, v_stride, scale,
                        dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (num_seqs == 0 || total_rows == 0) return GMLM_OK;
  attn_fill_bwd(x.a, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, x.a, hq * d, hkv * d, dtype, workspace_bytes, attn_delta_bytes(1, hq, total_rows))) != GMLM_OK)
    return rc;
  return launch_bwd(x, cdiv(max_len, BQ), num_seqs, hq, hkv, d, total_rows * hq, total_rows, dtype, as_stream(stream));
}
