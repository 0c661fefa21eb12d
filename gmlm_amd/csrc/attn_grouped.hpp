// Streaming self-attention with grouped KV heads (hq query heads share hkv KV heads), what the three families have in common:
//   gmlm_attention_causal_d128_*  attn_causal.hip  causal128::*       causal, d = 128        (Qwen3)
//   gmlm_attention_causal_d64_*   attn_gqa.hip     gqa::causal64_*    causal, d = 64         (Llama, Qwen2, Mistral)
//   gmlm_attention_bidir_gqa_*    attn_bidir.hip   bidir::gqa_*       bidirectional, d = 64 / 128   (EuroBERT, NomicBERT)
// and, for the launch parameters and the argument checks alone (its kernels are the four-waves-per-head plan of attn_wide.hpp):
//   gmlm_attention_gqa_d256_*     attn_gqa_wide.hip  gqaw::*          causal or bidirectional, d = 256   (Gemma3)
// A family's file holds its __global__ wrappers, one Family (its kernels, head dims and words) and its exports; everything else
// is here: the launch parameters, the argument checks in the order of attn_host.hpp, the launches and the two entry-point
// bodies.  A wrapper is decode() + one call: forward and dQ ARE attn_fwd_body / attn_dq_body (attn_stream.hpp) with GQA = true,
// delta is attn_delta_body, dK/dV is causal_dkv_body (attn_causal_dkv.hpp); only CAUSAL and D differ between the families.  The
// call stands in the wrapper itself, because these kernels are pinned to their instruction streams
// (profiles/attn_grouped_static.json) and one more __forceinline__ level changes them, whether it takes Params by reference, by
// value, or as (AttnParams&, stride, group).  Observed (hipcc of ROCm at this commit, -O3): every count equal, body_sha1 not, in all
// fwd and dkv instantiations; dq and delta unchanged.  In the forward the difference is the last ten instructions, the lse store
// after the key loop: v_log_f32 writes v0 instead of v2, and v_mov (the -inf constant) / v_add / v_mul move up between the
// s_add_u32 / s_addc_u32 of the address, with the v_cndmask before instead of after v_lshl_add_u64.  The dK/dV streams were not
// taken apart.
// Padded layout [b, l, heads, d] with per-operand row strides, so the fused [q | k | v] projection output is read (and its
// gradient written) without copies, or packed layout [T, heads, d]: the same kernels with AttnParams::cu set, sequence i = rows
// [cu[i], cu[i + 1]); a tile past its sequence returns block-uniformly.
// Tiling: 4 waves, 128 query rows per workgroup; Cfg<T> of attn_stream.hpp; 1-D grids of (tile, (sequence, head)) work items.
//  * causal: tiles wholly below the diagonal take the compare-free path of the non-causal kernels (block- or wave-uniform
//    test); only tiles that touch the diagonal compare key <= query per element (and key < kv_len);
//  * every wave reaches every barrier: a wave whose rows lie above a tile still stages K / V;
//  * causal: key 0 is valid for every query and a wave only computes tiles whose first key is <= its first query, so every row
//    of a computing wave has a valid key in every tile it computes: the running max is finite, -inf - (-inf) never occurs;
//  * bf16 backward: lse, delta and the kv_len mask ride in one extra contraction step as in the non-grouped kernels; the
//    causal mask is not rank-1, so diagonal tiles select P = 0 explicitly before dS;
//  * dK/dV: a workgroup owns 128 keys of one (sequence, KV head), walks the query heads of its group in order and, per head,
//    the query tiles (causal: from the diagonal on), accumulating into the same registers.  No atomics, no expanded K / V or
//    dK / dV in HBM.
#pragma once
#include <optional>
#include "attn_stream.hpp"
#include "attn_causal_dkv.hpp"
#include "attn_host.hpp"

namespace gmlm {
namespace grouped {

constexpr int NW = 4, NT = NW * 64, BQ = NW * 32;

struct Params {
  AttnParams a;            // a.h = query heads; lse / delta are [b, hq, l]; a.lq == a.lk
  int64_t dout_stride;     // row stride of dO / O (= hq * d)
  int32_t group;           // query heads per KV head (hq / hkv)
};

// ---- a family as data -------------------------------------------------------------------------------------------------------
// the four kernels of one (dtype, head dim); delta takes (out, out_lo, dout, rows, lq, heads, delta)
template <typename T>
struct Kernels {
  void (*fwd)(Params);
  void (*delta)(const T*, const T*, const T*, int64_t, int64_t, int64_t, float*);
  void (*dq)(Params);
  void (*dkv)(Params);
};
// what setup() is told about a family: its words in the refusals and its grids
struct Contract {
  const char* dims;             // how the head-dim refusal names the head dims taken
  const char* self;             // "causal self-attention" or "self-attention": the lq == lk refusal
  const char* no_dropout;       // how the dropout refusal names the kernels (attn_check_rates)
  int wave_rows = 0;            // 0: work items of BQ rows, delta by attn_delta_body.  > 0 (attn_gqa_wide.hip): work items of this many
                                // rows and a delta launch of one wave per (row, head), both grids bounded by setup()
};
struct Family {
  Contract c;
  Kernels<bf16_t> bf[2];        // [d == 128]; a head dim the family does not take stays empty
  Kernels<float> fp[2];         // INV: filled for the same head dims as bf (fwd() / bwd() read the head dims taken from bf alone)
  bool takes(int64_t d) const { return (d == 64 || d == 128) && bf[d == 128].fwd; }
};

// The sequences of a call.  Padded: n sequences of len rows each (= lk), rows = len.  Packed: n sequences of at most len rows,
// `rows` in all.  lse / delta are [n, hq, rows] padded and [hq, rows] packed: one "sequence" of `rows`.
struct Seqs {
  const int32_t *kv_len, *cu;
  int64_t n, len, lk, rows;
  bool packed;
  bool empty() const { return n == 0 || rows == 0; }
  int64_t lse_seqs() const { return packed ? 1 : n; }
};
inline Seqs padded(const int32_t* kv_len, int64_t b, int64_t lq, int64_t lk) { return {kv_len, nullptr, b, lq, lk, lq, false}; }
inline Seqs packed(const int32_t* cu, int64_t seqs, int64_t max_len, int64_t rows) { return {nullptr, cu, seqs, max_len, max_len, rows, true}; }

// the checks of attn_host.hpp up to the empty-problem return, with the family's words and grids; d_ok = the family takes head
// dim d; fills the launch parameters.  `window` (given by attn_gqa_band.hip alone): the band width of the call, refused outside [1, 2^30)
// right after the scale check; it is not stored here
inline int setup(const Contract& c, bool d_ok, const char* who, Params& x, const Seqs& s, const void* q, const void* k, const void* v,
                 int64_t hq, int64_t hkv, int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p,
                 const void* out_lo, int dtype, std::optional<int64_t> window = std::nullopt) {
  constexpr int64_t k2_30 = (int64_t)1 << 30;
  if (s.packed) {
    GMLM_REQUIRE(s.cu, "%s: null cu_seqlens", who);
    GMLM_REQUIRE(s.len > 0, "%s: max_len %ld must be positive", who, (long)s.len);
    GMLM_REQUIRE(s.n >= 0 && s.rows >= 0 && s.rows < k2_30, "%s: %ld packed rows (must be >= 0 and < 2^30)", who, (long)s.rows);
  }
  int rc = attn_check_shape(who, (s.packed ? s.len < k2_30 && s.n < k2_30 : s.n >= 0 && s.len >= 0 && s.lk >= 0) && hq > 0 && hkv > 0,
                            d_ok, d, c.dims, dtype, out_lo);
  if (rc != GMLM_OK) return rc;
  GMLM_REQUIRE(s.len == s.lk, "%s: %s needs lq == lk (got %ld and %ld)", who, c.self, (long)s.len, (long)s.lk);
  GMLM_REQUIRE(hq % hkv == 0, "%s: %ld query heads are not a multiple of %ld KV heads", who, (long)hq, (long)hkv);
  if ((rc = attn_check_rates(who, dropout_p, c.no_dropout, scale)) != GMLM_OK) return rc;
  if (window.has_value()) GMLM_REQUIRE(*window >= 1 && *window < k2_30, "%s: window %ld must be in [1, 2^30)", who, (long)*window);
  const bool fits = !c.wave_rows ? cdiv(s.len, BQ) * s.n * hq < ((int64_t)1 << 31)
                                 : hq < k2_30 && s.n < ((int64_t)1 << 31) &&
                                       (double)cdiv(s.len, (int64_t)c.wave_rows) * (double)s.n * (double)hq < 2147483648.0 &&
                                       (double)s.rows * (double)s.lse_seqs() * (double)hq < 4.0 * 2147483648.0;   // the delta launch
  GMLM_REQUIRE(s.len < k2_30 && fits, "%s: too many work items", who);
  x = Params{};
  attn_fill(x.a, q, k, v, s.kv_len, s.n, hq, s.rows, s.rows, q_stride, k_stride, v_stride, scale, 0.f, 0, nullptr);
  x.a.cu = s.cu;
  x.dout_stride = hq * d;
  x.group = (int32_t)(hq / hkv);
  return GMLM_OK;
}

// tiles = query (= key) tiles of 128 per sequence, seqs = sequences
template <typename T>
int launch_fwd(const Kernels<T>& k, const Params& x, int64_t tiles, int64_t seqs, hipStream_t st) {
  const int64_t hq = x.a.h;
  k.fwd<<<(unsigned)(tiles * seqs * hq), NT, 0, st>>>(x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

// the three backward launches; drows / dlq = the delta view: rows of [drows, d], lse index = (row / hq) within sequences of dlq
template <typename T>
int launch_bwd(const Kernels<T>& k, const Params& x, int64_t tiles, int64_t seqs, int64_t drows, int64_t dlq, hipStream_t st) {
  const AttnParams& p = x.a;
  const int64_t hq = p.h, hkv = hq / x.group;
  const int64_t lanes = x.dout_stride / hq / Pad<T>::v;          // attn_delta_body: d / V lanes per row
  k.delta<<<(unsigned)cdiv(drows * lanes, (int64_t)256), 256, 0, st>>>((const T*)p.out, (const T*)p.out_lo, (const T*)p.dout, drows, dlq,
                                                                     hq, p.delta);   // out_lo: NULL unless bf16 (attn_check_shape)
  GMLM_LAUNCH_CHECK();
  k.dq<<<(unsigned)(tiles * seqs * hq), NT, 0, st>>>(x);
  GMLM_LAUNCH_CHECK();
  k.dkv<<<(unsigned)(tiles * seqs * hkv), NT, 0, st>>>(x);
  GMLM_LAUNCH_CHECK();
  return GMLM_OK;
}

// ---- the entry points: a padded export passes padded(...), its varlen twin packed(...) --------------------------------------
inline int fwd(const Family& f, const char* who, const Seqs& s, const void* q, const void* k, const void* v, int64_t hq, int64_t hkv,
               int64_t d, int64_t q_stride, int64_t k_stride, int64_t v_stride, float scale, float dropout_p, void* out, void* out_lo,
               float* lse, int dtype, gmlm_stream_t stream) {
  Params x;
  int rc = setup(f.c, f.takes(d), who, x, s, q, k, v, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (s.empty()) return GMLM_OK;
  x.a.o_w = out; x.a.o_lo_w = out_lo; x.a.lse_w = lse;
  if ((rc = attn_check_fwd_operands(who, x.a, hq * d, hkv * d, dtype)) != GMLM_OK) return rc;
  const int64_t tiles = cdiv(s.len, BQ);
  return dtype == GMLM_BF16 ? launch_fwd(f.bf[d == 128], x, tiles, s.n, as_stream(stream))
                            : launch_fwd(f.fp[d == 128], x, tiles, s.n, as_stream(stream));
}

inline int bwd(const Family& f, const char* who, const Seqs& s, const void* q, const void* k, const void* v, const void* out,
               const void* out_lo, const void* dout, const float* lse, int64_t hq, int64_t hkv, int64_t d, int64_t q_stride,
               int64_t k_stride, int64_t v_stride, float scale, float dropout_p, void* dq, void* dk, void* dv, int64_t dq_stride,
               int64_t dk_stride, int64_t dv_stride, int dtype, void* workspace, size_t workspace_bytes, gmlm_stream_t stream) {
  Params x;
  int rc = setup(f.c, f.takes(d), who, x, s, q, k, v, hq, hkv, d, q_stride, k_stride, v_stride, scale, dropout_p, out_lo, dtype);
  if (rc != GMLM_OK) return rc;
  if (s.empty()) return GMLM_OK;
  attn_fill_bwd(x.a, out, out_lo, dout, lse, dq, dk, dv, dq_stride, dk_stride, dv_stride, workspace);
  const size_t need = attn_delta_bytes(s.lse_seqs(), hq, s.rows);
  if ((rc = attn_check_bwd_operands(who, x.a, hq * d, hkv * d, dtype, workspace_bytes, need)) != GMLM_OK) return rc;
  const int64_t tiles = cdiv(s.len, BQ), drows = s.lse_seqs() * s.rows * hq;
  return dtype == GMLM_BF16 ? launch_bwd(f.bf[d == 128], x, tiles, s.n, drows, s.rows, as_stream(stream))
                            : launch_bwd(f.fp[d == 128], x, tiles, s.n, drows, s.rows, as_stream(stream));
}

}  // namespace grouped
}  // namespace gmlm
