// Kernels of a Llama-architecture text encoder without the Q / K head norm (Llama, Qwen2, Mistral; C ABI in
// include/gmlm_hip_gqa.h), all in namespace gmlm::gqa:
//  * rope_heads: the rotate-half rotary embedding IN PLACE on the first `heads` = hq + hkv head rows of every token row of a
//    fused [q | k | v] buffer, at head dim 64 or 128 (the rotary pieces of row_kernels.hpp).  V columns are neither read nor
//    written.  A head row = D / V lanes x 16 bytes; every lane reads its 16 bytes, exchanges with the lane holding the other
//    half, and writes the same 16 bytes back: in place without a hazard.  fp32 arithmetic, one rounding on store; the table is
//    built on the host.  1-D grid capped at kRopeMaxBlocks, a block-uniform stride loop over groups of 256 / LPR head rows.
//    INV: the backward = the inverse rotation, so it needs no saved input and no workspace.
//  * causal attention with grouped KV heads at head dim 64 (gmlm_attention_causal_d64_*, padded and packed): the d = 128
//    family of attn_causal.hip at D = 64.  Forward and dQ are the streaming bodies of attn_stream.hpp with CAUSAL = GQA = true,
//    delta is the shared delta body, dK/dV is causal_dkv_body (attn_causal_dkv.hpp): the same text as causal128::dkv_kernel.
//    Tiling of causal128 (4 waves, 128 query rows; bf16: 64-key tiles double-buffered, fp32: 32-key tiles in one buffer): at
//    D = 64 the tiles and the accumulators are half as large, so its register and LDS budget holds with room to spare
//    (DESIGN.md section 4 "Llama, Qwen2 and Mistral encoders").
#include "attn_stream.hpp"
#include "attn_causal_dkv.hpp"
#include "attn_host.hpp"
#include "row_kernels.hpp"
#include "../../include/gmlm_hip_gqa.h"

namespace gmlm {
namespace gqa {

// ---- rotary embedding over head rows ---------------------------------------------------------------
constexpr int kRopeMaxBlocks = 2048;

template <typename T, int D, bool INV>
__global__ __launch_bounds__(256) void rope_heads_kernel(T* __restrict__ qkv, int64_t stride, const float* __restrict__ cs,
                                                         int64_t tokens, int64_t seq_len, int nh /* hq + hkv head rows per token */,
                                                         const int32_t* __restrict__ pos_ids, int64_t max_len) {
  constexpr int V = Store<T>::kVec, LPR = D / V, GPB = 256 / LPR;
  const int lr = threadIdx.x % LPR, grp = threadIdx.x / LPR;
  const int col = (lr * V) & (D / 2 - 1);
  const bool upper = lr >= LPR / 2;
  const int64_t items = tokens * nh;
  // the trip count is block-uniform: every lane of a wave reaches the exchange of every trip
  for (int64_t first = (int64_t)blockIdx.x * GPB; first < items; first += (int64_t)gridDim.x * GPB) {
    int64_t t;
    int hd;
    const bool live = head_row(first + grp, items, nh, t, hd);
    const float* csr = rope_row<D>(cs, t, seq_len, pos_ids, max_len);
    T* ptr = qkv + t * stride + (int64_t)hd * D + lr * V;
    float x[V], c[V], sn[V], o[V];
    Store<T>::ldv(ptr, x);
    load_f32<V>(csr + col, c);
    load_f32<V>(csr + D / 2 + col, sn);
#pragma unroll
    for (int v = 0; v < V; ++v) o[v] = rotate_half<LPR, INV>(x[v], c[v], sn[v], upper);
    if (live) Store<T>::stv(ptr, o);
  }
}

template <bool INV>
static int rope_heads(const char* who, void* qkv, int64_t stride, const float* cos_sin, int64_t max_len, int64_t tokens,
                      int64_t seq_len, const int32_t* pos_ids, int64_t heads, int64_t d, int dtype, gmlm_stream_t stream) {
  GMLM_REQUIRE(dtype == GMLM_F32 || dtype == GMLM_BF16, "%s: unsupported dtype", who);
  GMLM_REQUIRE(d == 64 || d == 128, "%s: head dim %ld not supported (this entry point takes 64 or 128)", who, (long)d);
  GMLM_REQUIRE(tokens >= 0 && heads > 0 && heads < 4096, "%s: bad sizes", who);
  GMLM_REQUIRE(max_len > 0, "%s: empty cos / sin table", who);
  if (!pos_ids) {
    GMLM_REQUIRE(seq_len >= 0 && seq_len <= max_len, "%s: sequence length %ld exceeds the %ld rows of the cos / sin table", who,
                 (long)seq_len, (long)max_len);
    GMLM_REQUIRE(seq_len > 0 || tokens == 0, "%s: %ld tokens in sequences of length 0", who, (long)tokens);
  }
  const int v = dtype == GMLM_F32 ? 4 : 8;
  GMLM_REQUIRE(stride >= heads * d && stride % v == 0, "%s: qkv row stride %ld must be >= %ld and a multiple of %d", who, (long)stride,
               (long)(heads * d), v);
  GMLM_REQUIRE(tokens * heads < ((int64_t)1 << 34), "%s: too many head rows", who);
  if (tokens == 0) return GMLM_OK;
  GMLM_REQUIRE(qkv && aligned16(qkv), "%s: null or not 16-byte aligned pointer", who);
  GMLM_REQUIRE(cos_sin && aligned16(cos_sin), "%s: null or misaligned cos / sin table", who);
  hipStream_t st = as_stream(stream);
  const int64_t items = tokens * heads, gpb = 256 / (d / v);     // head rows per block
  const int grid = grid_cap(cdiv(items, gpb), kRopeMaxBlocks);
#define GMLM_ROPE_HEADS_LAUNCH(T, D_)                                                                                          \
  rope_heads_kernel<T, D_, INV><<<grid, 256, 0, st>>>((T*)qkv, stride, cos_sin, tokens, seq_len, (int)heads, pos_ids, max_len)
  if (dtype == GMLM_BF16) { if (d == 64) GMLM_ROPE_HEADS_LAUNCH(bf16_t, 64); else GMLM_ROPE_HEADS_LAUNCH(bf16_t, 128); }
  else { if (d == 64) GMLM_ROPE_HEADS_LAUNCH(float, 64); else GMLM_ROPE_HEADS_LAUNCH(float, 128); }
#undef GMLM_ROPE_HEADS_LAUNCH
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

// ---- causal GQA attention at head dim 64 -------------------------------------------------------------
constexpr int D = 64, NW = 4, NT = NW * 64, BQ = NW * 32;

struct Params {
  AttnParams a;            // a.h = query heads; lse / delta are [b, hq, l]; a.lq == a.lk
  int64_t dout_stride;     // row stride of dO / O (= hq * 64)
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

template <typename T>
__global__ __launch_bounds__(NT) void causal64_fwd_kernel(Params x) {
  const Item it = decode(x.a);
  attn_fwd_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, true, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

// delta = rowsum(dO * O) over rows of [b * l, hq, 64]
template <typename T>
__global__ __launch_bounds__(256) void causal64_delta_kernel(const T* __restrict__ o, const T* __restrict__ o_lo,
                                                             const T* __restrict__ dout, int64_t rows /* b * l * hq */, int64_t lq,
                                                             int64_t hn, float* __restrict__ delta) {
  attn_delta_body<T>(o, o_lo, dout, rows, D, lq, hn, delta);
}

template <typename T>
__global__ __launch_bounds__(NT) void causal64_dq_kernel(Params x) {
  const Item it = decode(x.a);
  attn_dq_body<T, D, NW, false, Cfg<T>::KT, Cfg<T>::DBUF, true, true>(x.a, it.tile, it.b, it.hd, x.dout_stride, it.hd / x.group);
}

template <typename T>
__global__ __launch_bounds__(NT) void causal64_dkv_kernel(Params x) {
  const CausalKeyTile it = causal_key_tile(x.a, x.group);
  int64_t kvlen = it.l;                                      // kv_len clamped into [0, l], as the streaming bodies do
  if (x.a.kv_len) { kvlen = x.a.kv_len[it.b]; if (kvlen > it.l) kvlen = it.l; if (kvlen < 0) kvlen = 0; }
  causal_dkv_body<T, D, NW, Cfg<T>::QT, Cfg<T>::DBUF>(x.a, x.dout_stride, x.group, it, kvlen);
}

// the checks of attn_host.hpp up to the empty-problem return, in the order of the d = 128 family; fills the launch parameters
static int setup(const char* who, Params& x, const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b,
                 int64_t hq, int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                 float scale, float dropout_p, const void* out_lo, int dtype, bool sizes_ok = true) {
  int rc = attn_check_shape(who, sizes_ok && b >= 0 && hq > 0 && hkv > 0 && lq >= 0 && lk >= 0, d == 64, d, "this entry point takes 64",
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

#define GMLM_GQA_LAUNCH(KERNEL, grid, st, prm)                            \
  do {                                                                    \
    if (dtype == GMLM_BF16) KERNEL<bf16_t><<<grid, NT, 0, st>>>(prm);     \
    else KERNEL<float><<<grid, NT, 0, st>>>(prm);                         \
  } while (0)

// the three backward launches; tiles = query (= key) tiles of 128 per sequence, seqs = sequences, drows / dlq = the delta view
static int launch_bwd(Params& x, int64_t tiles, int64_t seqs, int64_t hq, int64_t hkv, int64_t drows, int64_t dlq, int dtype,
                      hipStream_t st) {
  AttnParams& p = x.a;
  GMLM_ATTN_DELTA_LAUNCH(causal64_delta_kernel, p, drows, dtype == GMLM_BF16 ? 8 : 16, st, dlq, hq);   // attn_delta_body: 64 / V lanes per row
  GMLM_LAUNCH_CHECK();
  const dim3 gq((unsigned)(tiles * seqs * hq));
  GMLM_GQA_LAUNCH(causal64_dq_kernel, gq, st, x);
  GMLM_LAUNCH_CHECK();
  const dim3 gk((unsigned)(tiles * seqs * hkv));
  GMLM_GQA_LAUNCH(causal64_dkv_kernel, gk, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

}  // namespace gqa
}  // namespace gmlm

using namespace gmlm;
using namespace gmlm::gqa;

extern "C" int gmlm_rope_heads_fwd(void* qkv, int64_t qkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens,
                                   int64_t seq_len, const int32_t* pos_ids, int64_t heads, int64_t d, int dtype, gmlm_stream_t stream) {
  return rope_heads<false>("rope_heads_fwd", qkv, qkv_stride, cos_sin, max_len, tokens, seq_len, pos_ids, heads, d, dtype, stream);
}

extern "C" int gmlm_rope_heads_bwd(void* dqkv, int64_t dqkv_stride, const float* cos_sin, int64_t max_len, int64_t tokens,
                                   int64_t seq_len, const int32_t* pos_ids, int64_t heads, int64_t d, int dtype, gmlm_stream_t stream) {
  return rope_heads<true>("rope_heads_bwd", dqkv, dqkv_stride, cos_sin, max_len, tokens, seq_len, pos_ids, heads, d, dtype, stream);
}

extern "C" int gmlm_attention_causal_d64_fwd(const void* q, const void* k, const void* v, const int32_t* kv_len, int64_t b, int64_t hq,
                                             int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                             int64_t v_stride, float scale, float dropout_p, void* out, void* out_lo, float* lse,
                                             int dtype, gmlm_stream_t stream) {
  static const char* who = "attention_causal_d64_fwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, hq, hkv, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, hq * D, hkv * D, dtype)) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(cdiv(lq, BQ) * b * hq));
  GMLM_GQA_LAUNCH(causal64_fwd_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_causal_d64_workspace_bytes(int64_t b, int64_t hq, int64_t lq) { return attn_delta_bytes(b, hq, lq); }

extern "C" int gmlm_attention_causal_d64_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                             const void* dout, const float* lse, const int32_t* kv_len, int64_t b, int64_t hq,
                                             int64_t hkv, int64_t lq, int64_t lk, int64_t d, int64_t q_stride, int64_t k_stride,
                                             int64_t v_stride, float scale, float dropout_p, void* dq, void* dk, void* dv,
                                             int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                             size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "attention_causal_d64_bwd";
  Params x;
  int rc = setup(who, x, q, k, v, kv_len, b, hq, hkv, lq, lk, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (b == 0 || lq == 0) return GMLM_OK;
  attn_fill_bwd(x.a, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, x.a, hq * D, hkv * D, dtype, workspace_bytes, attn_delta_bytes(b, hq, lq))) != GMLM_OK) return rc;
  return launch_bwd(x, cdiv(lq, BQ), b, hq, hkv, b * lq * hq, lq, dtype, as_stream(stream));
}

extern "C" int gmlm_attention_causal_d64_varlen_fwd(const void* q, const void* k, const void* v, const int32_t* cu_seqlens,
                                                    int64_t num_seqs, int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv,
                                                    int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                                    float dropout_p, void* out, void* out_lo, float* lse, int dtype,
                                                    gmlm_stream_t stream) {
  static const char* who = "attention_causal_d64_varlen_fwd";
  Params x;
  int rc = setup_varlen(who, x, q, k, v, cu_seqlens, num_seqs, max_len, total_rows, hq, hkv, d, q_stride, k_stride, v_stride, scale,
                        dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (num_seqs == 0 || total_rows == 0) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, hq * D, hkv * D, dtype)) != GMLM_OK) return rc;
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)(cdiv(max_len, BQ) * num_seqs * hq));
  GMLM_GQA_LAUNCH(causal64_fwd_kernel, grid, st, x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

extern "C" size_t gmlm_attention_causal_d64_varlen_workspace_bytes(int64_t total_rows, int64_t hq) {
  return attn_delta_bytes(1, hq, total_rows);   // delta [hq, total_rows]
}

extern "C" int gmlm_attention_causal_d64_varlen_bwd(const void* q, const void* k, const void* v, const void* out, const void* out_lo,
                                                    const void* dout, const float* lse, const int32_t* cu_seqlens, int64_t num_seqs,
                                                    int64_t max_len, int64_t total_rows, int64_t hq, int64_t hkv, int64_t d,
                                                    int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale,
                                                    float dropout_p, void* dq, void* dk, void* dv, int64_t dq_stride,
                                                    int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace,
                                                    size_t workspace_bytes, gmlm_stream_t stream) {
  static const char* who = "attention_causal_d64_varlen_bwd";
  Params x;
  int rc = setup_varlen(who, x, q, k, v, cu_seqlens, num_seqs, max_len, total_rows, hq, hkv, d, q_stride, k_stride, v_stride, scale,
                        dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (num_seqs == 0 || total_rows == 0) return GMLM_OK;
  attn_fill_bwd(x.a, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  if ((rc = attn_check_bwd_operands(who, x.a, hq * D, hkv * D, dtype, workspace_bytes, attn_delta_bytes(1, hq, total_rows))) != GMLM_OK)
    return rc;
  return launch_bwd(x, cdiv(max_len, BQ), num_seqs, hq, hkv, total_rows * hq, total_rows, dtype, as_stream(stream));
}
