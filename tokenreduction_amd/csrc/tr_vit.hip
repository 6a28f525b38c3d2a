// Whole-model executor: enqueues the DeiT / Top-K / EViT forward pass on the caller's stream.
//
// Follows TopKVisionTransformer.forward (topk.py:179-212), EfficientVisionTransformer.forward
// (evit.py:209-244) and deit_viz.VisionTransformer.forward (:186-212), eval mode:
//   patch_embed -> cat(cls) + pos_embed -> 12 x Block -> norm -> x[:,0] -> head
// with Block_TopK.forward (topk.py:83-99):  x += attn(norm1(x)); [Top-K gather]; x += mlp(norm2(x)).
// tr_vit_config.global_pool == 1 replaces `norm -> x[:,0]` by `weighted mean of x[:,1:] -> norm` (timm's global_pool='avg' with fc_norm;
// tr_pool.hip, pooled_norm_head below): not a head the reference has.
//
// Host-side only: shape bookkeeping and kernel launches (no allocation, no synchronisation, no
// device->host copies), so one call is a fixed launch sequence that a caller may capture in a hipGraph.
// Token counts are static per (config) -- topk.py:56 int(ratio*196) -- so every buffer size is known up front.
#include <string.h>
#include "tr_common.h"
#include "tr_plan.h"

int tr_mlp_fused_wanted(int M, int D, int Hd, int have_scratch, int concurrent);      // tr_mlp_fused.hip: the schedule policy behind tr_set_mlp_fused
int tr_mlp_resid_ln_enabled();                                        // tr_mlp_fused.hip: tr_set_mlp_resid_ln's switch
// ... and its launches on a counter set that ONE memset in front of the forward has zeroed (block i uses set i)
int tr_mlp_fused_zero_counters(void* scratch, size_t scratch_bytes, int D, int Hd, int nsets, tr_stream_t s);
int tr_mlp_fused_bf16_set(const uint16_t* xn, const void* packed, const float* fc1_b, uint16_t* out, void* scratch, size_t scratch_bytes, int M, int D,
                          int Hd, int cset, tr_stream_t s);
int tr_mlp_fused_ln_bf16_set(const float* x, const uint16_t* delta, const float* g, const float* b, float eps, const void* packed, const float* fc1_b,
                             uint16_t* out, void* scratch, size_t scratch_bytes, int M, int D, int Hd, int cset, tr_stream_t s);
int tr_mlp_fused_resid_ln_bf16_set(const uint16_t* xn, const void* packed, const float* fc1_b, const float* fc2_b, float* x, const float* next_g,
                                   const float* next_b, float eps, uint16_t* xn_next, void* scratch, size_t scratch_bytes, int M, int D, int Hd,
                                   int cset, tr_stream_t s);
int tr_mlp_ln_wanted(int M, int D, int Hd, int have_scratch, int concurrent);         // tr_mlp_fused.hip: ... with the norm2 in front of it inside the launch (tr_set_mlp_ln)

// CLS tail (eval, bf16): after the last block's attention no row mixes with another one again, and the forward returns head(norm(x)[:, 0]) --
// so from that attention's output onward only the B CLS rows are computed (see vit_forward_impl).  1 (default) / 0: today's full-width block.
// Bit-identical either way; process-wide, read when the launches are enqueued (a captured hipGraph keeps the form it was captured with).
static std::atomic<int> g_cls_tail{1};
extern "C" int tr_set_cls_tail(int on) { return g_cls_tail.exchange(on != 0 ? 1 : 0); }

namespace {

using trplan::align_up;

struct Plan {
  int P, N0, D, H, Hd, C, kcols;
  size_t off_x0, off_x1, off_xn, off_qkv, off_ao, off_h, off_d, off_d2, off_cols, off_cls, off_scores, off_idx, off_compl, off_xcls, off_size0, off_size1, off_cluster, off_soft, off_mlp_sk, mlp_sk_bytes, off_misc, off_pool, total;
};

bool make_plan(const tr_vit_config* c, int B, Plan* p) {
  if (!c || B <= 0) return false;
  if (c->precision != TR_PREC_BF16 && c->precision != TR_PREC_FP32 && c->precision != TR_PREC_BF16X3) return false;
  const size_t es = c->precision != TR_PREC_BF16 ? 4 : 2;   // activation element size
  int gh, gw;
  if (!trplan::patch_grid(c, &gh, &gw)) return false;
  if (c->depth <= 0 || c->depth > TR_MAX_DEPTH) return false;
  if (c->num_heads <= 0 || c->embed_dim != c->num_heads * 64) return false;
  if (c->family < TR_FAMILY_DEIT || c->family > TR_FAMILY_HEURISTIC) return false;
  if (c->global_pool != 0 && c->global_pool != 1) return false;
  p->P = gh * gw;
  p->N0 = p->P + 1;
  p->D = c->embed_dim;
  p->H = c->num_heads;
  p->Hd = c->mlp_hidden;
  p->C = c->num_classes;
  p->kcols = c->in_chans * c->patch * c->patch;
  // C == 0: headless (deit_viz.py:142,182 -- head = nn.Identity()): the final-normed CLS rows are the output, no classifier runs
  if (p->kcols % 64 || p->D % 64 || p->Hd % 64 || p->C % 4 || p->Hd <= 0 || p->C < 0) return false;
  const size_t T = (size_t)B * p->N0;  // max tokens
  size_t o = 0;
  p->off_x0 = o;     o += align_up(T * p->D * 4);
  p->off_x1 = o;     o += align_up(T * p->D * 4);
  p->off_xn = o;     o += align_up(T * p->D * es);
  p->off_qkv = o;    o += align_up(T * 3 * p->D * es);
  p->off_ao = o;     o += align_up(T * p->D * es);
  p->off_h = o;      o += align_up(T * p->Hd * es);
  p->off_d = o;      o += align_up(T * p->D * es);
  p->off_d2 = o;     o += align_up(T * p->D * es);      // second residual buffer (norm2 without a stream write, see vit_forward_impl)
  p->off_cols = o;   o += align_up((size_t)B * p->P * p->kcols * es);
  p->off_cls = o;    o += align_up((size_t)B * p->H * p->N0 * 4);
  p->off_scores = o; o += align_up((size_t)B * p->N0 * 4);
  p->off_idx = o;    o += align_up((size_t)B * p->N0 * 4);
  p->off_compl = o;  o += align_up((size_t)B * p->N0 * 4);
  p->off_size0 = o;  o += align_up((size_t)B * p->N0 * 4);
  p->off_size1 = o;  o += align_up((size_t)B * p->N0 * 4);
  p->off_xcls = o;   o += align_up((size_t)B * p->D * es);
  p->off_cluster = o;
  if (c->family == TR_FAMILY_DPCKNN) o += align_up(tr_dpcknn_workspace_floats(B, p->N0) * 4 + (size_t)B * p->N0 * 4);
  if (c->family == TR_FAMILY_KMEDOIDS)
    o += align_up(tr_dpcknn_workspace_floats(B, p->N0) * 4) + align_up((size_t)B * p->H * 4 * p->N0 * 4);
  // soft-assignment families: token-major logits / scores / transport plan of a stage, fp32 [B*N0, soft_ld(K)]
  p->off_soft = o;
  if (trplan::soft_family(c->family)) {
    int kmax = 0;
    for (int i = 0; i < c->depth; ++i) kmax = c->keep[i] > kmax ? c->keep[i] : kmax;
    o += align_up(T * (size_t)trplan::soft_ld(kmax) * 4);
  }
  // stream-K scratch of the fused eval Mlp (tr_mlp_fused.hip): one accumulator slot of 192 KiB + a counter per compute unit, bf16 executor only
  p->off_mlp_sk = o;
  p->mlp_sk_bytes = c->precision == TR_PREC_BF16 ? tr_mlp_fused_scratch_bytes(p->D, p->Hd) : 0;
  o += align_up(p->mlp_sk_bytes);
  p->off_misc = o;          // device words read back by the host (ATS dynamic width)
  o += align_up(256);
  p->off_pool = o;          // global_pool == 1: the pooled patch tokens fp32 [B, D], the final norm's input (no slot otherwise)
  if (c->global_pool == 1) o += align_up((size_t)B * p->D * 4);
  p->total = o;
  return true;
}

// ---- precision dispatch: the executor is one launch sequence; TR_PREC_FP32 swaps every op for its fp32 validation twin;
// TR_PREC_BF16X3 is that fp32 executor with the Linears and the attention on the matrix cores as split-bf16 products (tr_split.hip)
inline int op_im2col(bool f32, const float* img, void* cols, int B, int C, int H, int W, int patch, tr_stream_t s) {
  return f32 ? tr_im2col_f32(img, static_cast<float*>(cols), B, C, H, W, patch, s)
             : tr_im2col_bf16(img, static_cast<uint16_t*>(cols), B, C, H, W, patch, s);
}
inline int op_im2col_u8(bool f32, const uint8_t* img, const float* lut, int layout, void* cols, int B, int C, int H, int W, int patch,
                        tr_stream_t s) {
  return f32 ? tr_im2col_u8_f32(img, lut, layout, static_cast<float*>(cols), B, C, H, W, patch, s)
             : tr_im2col_u8_bf16(img, lut, layout, static_cast<uint16_t*>(cols), B, C, H, W, patch, s);
}
inline int op_gemm(int prec, const void* A, const void* W, const float* bias, void* out, const float* aux, int aux_i, int M, int N,
                   int K, int epi, tr_stream_t s) {
  if (prec == TR_PREC_BF16)
    return tr_gemm_bf16(static_cast<const uint16_t*>(A), static_cast<const uint16_t*>(W), bias, out, aux, aux_i, M, N, K, epi, s);
  const int e32 = (epi == TR_EPI_BF16) ? TR_EPI_F32 : epi;      // "store bf16" becomes "store fp32"; GELU / PATCH / F32 keep their meaning
  if (prec == TR_PREC_BF16X3)
    return tr_gemm_split(static_cast<const float*>(A), static_cast<const float*>(W), bias, static_cast<float*>(out), aux, aux_i, M, N, K,
                         e32, s);
  return tr_gemm_f32(static_cast<const float*>(A), static_cast<const float*>(W), bias, static_cast<float*>(out), aux, aux_i, M, N, K,
                     e32, s);
}
inline int op_ln(bool f32, float* x, long ldx, const void* d, long ldd, const float* g, const float* b, void* y, int M, int D,
                 float eps, tr_stream_t s) {
  return f32 ? tr_layernorm_f32(x, ldx, static_cast<const float*>(d), ldd, g, b, static_cast<float*>(y), M, D, eps, s)
             : tr_layernorm_bf16(x, ldx, static_cast<const uint16_t*>(d), ldd, g, b, static_cast<uint16_t*>(y), M, D, eps, s);
}
// norm over x + pending residual(s): the plain norm1 of a block and the final norm.  d_attn != nullptr: the previous block's norm2 did
// not write the stream back (lazy norm2 below), so BOTH of its residuals are still pending -- (x + d_attn) + d, the reference's order.
// y_f32 (the final norm of a headless model): y is fp32 on every path -- on the bf16 path the same arithmetic stored unrounded
// (tr_layernorm_bf16_f32), so bf16(y) is what the bf16 forms store
inline int op_ln_pending(bool f32, float* x, long ldx, const void* d, const void* d_attn, long ldd, const float* g, const float* b, void* y,
                         int M, int D, float eps, tr_stream_t s, bool y_f32 = false) {
  const uint16_t* d1 = static_cast<const uint16_t*>(d_attn != nullptr ? d_attn : d);     // first residual added
  const uint16_t* d2 = d_attn != nullptr ? static_cast<const uint16_t*>(d) : nullptr;     // second (lazy norm2 only)
  if (y_f32 && !f32) return tr_layernorm_bf16_f32(x, ldx, x, ldx, d1, ldd, d2, ldd, g, b, static_cast<float*>(y), M, D, eps, s);
  if (d_attn == nullptr) return op_ln(f32, x, ldx, d, ldd, g, b, y, M, D, eps, s);
  return tr_layernorm2_bf16(x, ldx, x, ldx, d1, ldd, d2, ldd, g, b, static_cast<uint16_t*>(y), M, D, eps, s);
}
inline int op_attn(int prec, const void* qkv, void* out, float* cls_rows, const float* size, float* colsum, int B, int N, int H,
                   tr_stream_t s) {
  if (prec == TR_PREC_BF16X3)
    return tr_attention_split(static_cast<const float*>(qkv), static_cast<float*>(out), cls_rows, size, colsum, B, N, H, s);
  return prec == TR_PREC_FP32 ? tr_attention_f32(static_cast<const float*>(qkv), static_cast<float*>(out), cls_rows, size, colsum, B, N, H, s)
             : tr_attention_bf16(static_cast<const uint16_t*>(qkv), static_cast<uint16_t*>(out), cls_rows, size, colsum, B, N, H, s);
}
inline int op_gather(bool f32, const float* x, const void* d, const int32_t* idx, const int32_t* cidx, const float* scores,
                     const float* g, const float* b, float* x_out, void* y, int B, int N, int K, int D, float eps, tr_stream_t s) {
  return f32 ? tr_gather_layernorm_f32(x, static_cast<const float*>(d), idx, cidx, scores, g, b, x_out, static_cast<float*>(y), B, N, K,
                                       D, eps, s)
             : tr_gather_layernorm_bf16(x, static_cast<const uint16_t*>(d), idx, cidx, scores, g, b, x_out, static_cast<uint16_t*>(y),
                                        B, N, K, D, eps, s);
}

}  // namespace

extern "C" size_t tr_vit_workspace_bytes(const tr_vit_config* cfg, int B) {
  Plan p;
  if (!make_plan(cfg, B, &p)) return 0;
  return p.total;
}

#define TR_TRY(call)            \
  do {                          \
    int rc__ = (call);          \
    if (rc__ != TR_OK) return rc__; \
  } while (0)

namespace {

inline const uint16_t* u16(const void* p) { return static_cast<const uint16_t*>(p); }
inline uint16_t* u16(void* p) { return static_cast<uint16_t*>(p); }

// One forward being enqueued: vit_forward_impl builds it and calls its steps in the reference forward's order.
// tape != nullptr: TRAINING forward -- every activation the backward pass needs goes to its own slot of the tape (tr_plan.h)
// instead of the shared scratch, the residual stream is written out of place (the inputs of norm1 / norm2 of every block stay),
// fc1 keeps its pre-activation (GELU as a separate kernel), and the decisions (kept ids, sizes) are kept per block.
struct Fwd {
  // ---- fixed inputs, each read once ---------------------------------------------------------------------------------------------------
  const tr_vit_config* cfg;
  const tr_vit_weights* w;
  Plan p;
  int B, D, H, prec;
  tr_stream_t s;
  bool f32, train;              // f32: fp32 activations (TR_PREC_FP32 and TR_PREC_BF16X3)
  char *ws, *tape;
  const trplan::TapePlan* tp;
  const void* img;              // fp32 [B,C,H,W] (TR_INPUT_F32) or uint8 pixels normalized through pixel_lut by the patch embedding
  int input_format;
  const float *pixel_lut, *aug_noise;
  const tr_augment_rec* aug;
  long aug_noise_len;
  const float* drop_scale;      // DropPath: per block and image, attention branch then MLP branch
  float drop_mul;               // Dropout: survivors are scaled by 1 / (1 - p) like nn.Dropout
  float* logits;
  int32_t *kept_idx, *compl_idx;
  int* tokens_out;
  // Lazy norm2 (eval, bf16, families whose blocks all start with a plain norm1): a norm2 that no reduction follows reads x + d_attn but
  // does not store it; the next norm1 (or the final norm) adds d_attn and d_mlp in the reference's order and writes the stream once.
  // Bit-identical to the eager sequence (same fp32 additions), 22 instead of 24 bytes per element and block through the norms.
  bool lazy_base;
  // Fused block tail (tr_mlp_fused_resid_ln_bf16): where the fused eval Mlp runs and the next block starts with a plain norm1, ONE launch does
  // fc1 -> GELU -> fc2, adds the result to the stream in place and writes the next block's norm1 -- into the hidden-activation buffer, which the
  // fused Mlp leaves unused and which nothing touches until that block's own Mlp (its only reader is the next qkv GEMM).  The block's norm2
  // then writes the stream (eager): the kernel's accumulators start at the stream row.  OFF by default (tr_set_mlp_resid_ln): measured in the
  // model it loses 4 % against fused Mlp + LayerNorm launch (the epilogue stalls the workgroup; profiles/r05_mlp_lab.md).
  bool rl_base;
  int conc;                     // other forwards run beside this one: a launch need not fill the chip on its own
  // the fused Mlp's stream-K scratch is there and wanted.  Beside other forwards it is not: the other forward's launches fill the second
  // round's idle compute units, and whole blocks round-robin move no accumulators (125 MB per launch at the first stage): measured with two
  // forwards in flight +0.5 % (Top-K kr 0.7), +1.5 % (kr 0.5), +2 % (dense DeiT-S); one at a time -1.5 ... -4 % (tools/lab/inflight_ab2.py)
  bool sk_ok;
  bool pool;                    // global_pool == 1: the head reads the average of the patch tokens (pooled_norm_head), the last block stays full width
  bool one_memset;              // the stream-K counters of every fused-Mlp launch (block i: set i) are zeroed by ONE memset in front of the blocks

  // ---- buffers: the shared scratch ... ------------------------------------------------------------------------------------------------
  void *xn_shared, *ao_shared, *dbuf_shared, *dbuf2, *cols, *xcls;
  float *cls_rows, *scores, *colsum_part, *size_a, *size_b;
  int32_t *idx_ws, *compl_ws;
  // ... and what currently stands in for each buffer (training re-points them at the block's tape slots: begin_block)
  float *x, *x_alt;             // the residual stream and the buffer its next out-of-place form goes to
  void *xn, *qkv, *ao, *hbuf;
  void* dbuf;                   // bf16 output of proj / fc2, added to x by the NEXT norm

  // ---- cursors ------------------------------------------------------------------------------------------------------------------------
  int N;                        // tokens (incl. CLS) of the stream: the stage reducers and the in-block reducers lower it
  const void* pending = nullptr;        // residual not yet added to x (the previous block's fc2 output): mlp sets it, the next norm takes it
  const void* pending_attn = nullptr;   // the attention branch's residual of the previous block, not yet in x (lazy norm2 / cls_tail)
  long pending_ld = 0;          // row stride of the pending residuals at the final norm's CLS rows; 0: N * D (cls_tail sets D)
  const void* xn1_ready = nullptr;      // norm1 of the block about to start, written by the previous block's fused tail (mlp -> norm1_qkv)
  float* size_cur = nullptr;    // ToMe token sizes / ATS and Heuristic key masks: none until the first merge (tome.py:185)
  const float* policy_cur = nullptr;    // DyViT training: the keep policy every block attends under (all ones before the first stage)
  const float* noise_in;        // DPC-KNN density noise / DyViT Gumbel noise, consumed stage by stage
  float* soft_out;              // soft assignments of the stages, written back to back
  const uint8_t* drop_keep;     // Dropout keep masks, consumed in the order tr_vit_dropout_mask_bytes documents
  float* features_out;          // eval: the stream after every block, back to back; training: DyViT's distillation output
  // output taps (eval, tr_vit_forward_taps): the CLS rows after the blocks of tap_mask go to cls_out [B, n_taps, D] (tap_i: the next column),
  // the final norm of every row to final_tokens_out.  A CLS tap reads what is there -- it switches nothing off; final_tokens_out needs every
  // row of the last block and so keeps it full width (begin_block)
  uint32_t tap_mask = 0;
  int n_taps = 0, tap_i = 0;
  float *cls_out = nullptr, *final_tokens_out = nullptr;
  // level taps (eval, tr_vit_forward_levels): EVERY row of the stream after the blocks of level_mask, plus what is pending there, goes to the
  // next slab of level_out (level_i; a slab is B * N0 * D elements and holds [B, N, D]) -- as it stands (the rows of features_out) or through
  // the final norm.  Like a CLS tap it reads what is there; a tapped last block needs every row and so runs full width (begin_block)
  uint32_t level_mask = 0;
  int level_norm = 0, level_i = 0;
  float* level_out = nullptr;
  // dense feature maps in training (tr_vit_forward_train_dense): the stream entering the final norm and the final norm of every row go to
  // the caller's buffers -- DyViT's distillation output with the tape's xfin_all slot replaced by a caller-owned one
  float *dense_stream = nullptr, *dense_tokens = nullptr;
  // level taps in training (tr_vit_forward_train_levels, norm == 1): the summed rows of a tapped block go to the next slab of level_stream in
  // the launch that writes their final norm into level_out -- the norm's backward needs the rows that entered it
  float* level_stream = nullptr;
  // ---- the block being enqueued (pre_block, begin_block) ------------------------------------------------------------------------------
  bool have_xn = false;         // norm1(x) already in xn (written by a pre-block reducer)
  bool tail = false;            // this block runs as the CLS tail
  bool norm2_in_mlp = false;    // this block's norm2 runs inside its fused Mlp launch
  int K = 0, Ks = 0, r = 0;              // Top-K / EViT tokens kept, ATS sample_count, ToMe tokens merged away (0 = plain block)

  // the arguments of vit_forward_impl, validated; every member is set here
  Fwd(const tr_vit_config* cfg_, const tr_vit_weights* w_, const Plan& plan, int B_, tr_stream_t s_, void* workspace, char* tape_,
      const trplan::TapePlan* tp_, const void* img_, int input_format_, const float* pixel_lut_, const tr_augment_rec* aug_,
      const float* aug_noise_, long aug_noise_len_, float* logits_, int32_t* kept_idx_, int32_t* compl_idx_, float* soft_out_,
      const float* noise_in_, float* features_out_, int* tokens_out_, const float* drop_scale_, const uint8_t* drop_keep_, float drop_rate,
      const tr_vit_taps* taps, const tr_vit_levels* levels)
      : cfg(cfg_), w(w_), p(plan), B(B_), D(plan.D), H(plan.H), prec(cfg_->precision), s(s_), f32(cfg_->precision != TR_PREC_BF16),
        train(tape_ != nullptr), ws(static_cast<char*>(workspace)), tape(tape_), tp(tp_), img(img_), input_format(input_format_),
        pixel_lut(pixel_lut_), aug_noise(aug_noise_), aug(aug_), aug_noise_len(aug_noise_len_), drop_scale(drop_scale_),
        drop_mul(drop_keep_ != nullptr ? 1.0f / (1.0f - drop_rate) : 1.0f), logits(logits_), kept_idx(kept_idx_), compl_idx(compl_idx_),
        tokens_out(tokens_out_), N(plan.N0), noise_in(noise_in_), soft_out(soft_out_), drop_keep(drop_keep_), features_out(features_out_) {
    if (taps != nullptr) {
      tap_mask = taps->cls_blocks;
      n_taps = __builtin_popcount(tap_mask);
      cls_out = tap_mask != 0 ? taps->cls_out : nullptr;
      final_tokens_out = taps->final_tokens_out;
    }
    if (levels != nullptr && levels->blocks != 0) {
      level_mask = levels->blocks;
      level_norm = levels->norm;
      level_out = levels->tokens_out;
    }
    lazy_base = !train && !f32 && features_out == nullptr;
    rl_base = lazy_base && drop_keep == nullptr && drop_scale == nullptr && tr_mlp_resid_ln_enabled();
    conc = (!train && cfg->concurrent) ? 1 : 0;
    pool = cfg->global_pool == 1;
    sk_ok = p.mlp_sk_bytes > 0 && !conc;
    one_memset = !train && prec == TR_PREC_BF16 && sk_ok && w->blocks[0].mlp_pk != nullptr;
    x = scratch(p.off_x0);
    x_alt = scratch(p.off_x1);
    xn = xn_shared = ws + p.off_xn;
    qkv = ws + p.off_qkv;
    ao = ao_shared = ws + p.off_ao;
    hbuf = ws + p.off_h;
    dbuf = dbuf_shared = ws + p.off_d;
    dbuf2 = ws + p.off_d2;      // second residual buffer (norm2 without a stream write)
    cols = train ? static_cast<void*>(tape + tp->cols) : static_cast<void*>(ws + p.off_cols);
    cls_rows = scratch(p.off_cls);
    scores = scratch(p.off_scores);
    idx_ws = scratch<int32_t>(p.off_idx);
    compl_ws = scratch<int32_t>(p.off_compl);
    xcls = ws + p.off_xcls;
    colsum_part = cfg->family == TR_FAMILY_KMEDOIDS ? scratch(p.off_cluster + align_up(tr_dpcknn_workspace_floats(B, p.N0) * 4)) : nullptr;
    size_a = scratch(p.off_size0);
    size_b = scratch(p.off_size1);
  }

  // ---- small helpers ------------------------------------------------------------------------------------------------------------------
  template <class T = float> T* scratch(size_t off) const { return reinterpret_cast<T*>(ws + off); }
  template <class T = float> T* slot(size_t off) const { return reinterpret_cast<T*>(tape + off); }
  void* sk_scratch() const { return sk_ok ? ws + p.off_mlp_sk : nullptr; }
  void swap_x() { float* t = x; x = x_alt; x_alt = t; }
  // where a stage's kept / centre ids and its complement / assignment ids go: the block's tape slot, the caller's per-block slab, or scratch
  int32_t* kept_dst(int i) const {
    return train ? slot<int32_t>(tp->blk[i].idx) : kept_idx ? kept_idx + (size_t)i * B * p.N0 : idx_ws;
  }
  int32_t* compl_dst(int i) const {
    return train ? slot<int32_t>(tp->blk[i].idx2) : compl_idx ? compl_idx + (size_t)i * B * p.N0 : compl_ws;
  }
  void soft_advance(int Kc) { if (soft_out) soft_out += (size_t)B * Kc * (N - 1); }
  // what consumes the pending residuals after block j - 1: a plain norm1 (or the final norm) unless a pre-block reducer fires at block j
  bool starts_plain(int j) const {
    if (j >= cfg->depth) return true;
    switch (cfg->family) {
      case TR_FAMILY_DPCKNN: case TR_FAMILY_KMEDOIDS: case TR_FAMILY_PATCHMERGER: case TR_FAMILY_SINKHORN: case TR_FAMILY_DYVIT:
      case TR_FAMILY_SIT: return cfg->keep[j] <= 0;
      default: return true;                                   // in-block families (Top-K, EViT, ToMe, ATS), DeiT, Heuristic (masks only)
    }
  }
  // x + resid -> dst (out of place: x stays, on the tape), LayerNorm of the sum -> y (bf16); the stream continues in dst
  int stream_to(float* dst, const void* resid, const float* g, const float* b, void* y, float eps) {
    TR_TRY(tr_layernorm_bf16_to(x, D, dst, D, u16(resid), D, g, b, u16(y), B * N, D, eps, s));
    x = dst;
    return TR_OK;
  }
  // training: the stream entering stage i (x + the previous mlp output) goes to the block's tape slot x0
  int enter_stage(int i, const float* g, const float* b, void* y, float eps) {
    TR_TRY(stream_to(slot(tp->blk[i].x0), pending, g, b, y, eps));
    pending = nullptr;
    return TR_OK;
  }
  // the weighted sums of a soft assignment sc [B*N, ld] into x_alt: on MFMA where the bf16 executor can (K <= 192), else the family's own kernel
  template <class F>
  int soft_merge(float* sc, int ld, float scale, int softmax, const float* xh, float* soft, int Kc, F fallback) {
    if (!f32 && Kc <= 192) return tr_softassign_merge_fast(sc, ld, scale, softmax, x, xh, x_alt, soft, B, N, Kc, D, s);
    return fallback();
  }
  // Dropout (timm's drop_rate: pos_drop topk.py:186, proj_drop :53, the Mlp's two nn.Dropout): training only.  The caller draws the keep
  // masks (1 byte per element, in forward order: tr_vit_dropout_mask_bytes).  stream: buf is the fp32 stream, else a bf16 branch output.
  int drop(void* buf, size_t n, bool stream = false) {
    if (drop_keep == nullptr) return TR_OK;
    TR_TRY(stream ? tr_dropout_f32(static_cast<float*>(buf), static_cast<float*>(buf), drop_keep, drop_mul, n, s)
                  : tr_dropout_bf16(u16(buf), u16(buf), drop_keep, drop_mul, n, s));
    drop_keep += n;
    return TR_OK;
  }
  // DropPath on the branch output in dbuf (topk.py:87, :95): block i's per-image scale, branch 0 = attention, 1 = MLP
  int drop_path(int i, int branch) {
    if (drop_scale == nullptr) return TR_OK;
    return tr_rowscale_bf16(u16(dbuf), u16(dbuf), drop_scale + (size_t)(2 * i + branch) * B, B, N, D, s);
  }

  // ---- steps, in forward order --------------------------------------------------------------------------------------------------------
  // a1 + a2: patch embedding, CLS token, position embedding; pos_drop
  // uint8 pixels: the same choice of path, each with its uint8 loader (normalization through the LUT; same columns, same bits)
  int embed() {
    const bool pixels = input_format != TR_INPUT_F32;
    const uint8_t* u8img = static_cast<const uint8_t*>(img);
    const float* fimg = static_cast<const float*>(img);
    const int layout = input_format == TR_INPUT_U8_NHWC ? TR_LAYOUT_NHWC : TR_LAYOUT_NCHW;
    const int C = cfg->in_chans, IH = trplan::img_h(cfg), IW = trplan::img_w(cfg), patch = cfg->patch;
    if (!train && !f32 && tr_patch_embed_hw_supported(C, IH, IW, patch, D)) {
      // eval: unfold + GEMM + cls/pos in one launch (tr_patch.hip), at every batch size (the two paths differ in the last bit: an image's
      // tokens must not depend on its batch); training keeps the column matrix (PatchEmbed's weight-gradient operand)
      if (pixels)
        TR_TRY(tr_patch_embed_u8_hw_bf16(u8img, pixel_lut, layout, u16(w->patch_w), w->patch_b, w->cls_token, w->pos_embed, x, B, C, IH, IW, patch, D, s));
      else
        TR_TRY(tr_patch_embed_hw_bf16(fimg, u16(w->patch_w), w->patch_b, w->cls_token, w->pos_embed, x, B, C, IH, IW, patch, D, s));
    } else {
      if (pixels && aug != nullptr)      // training on uint8 pixels with the device-side erase / mixup / cutmix: the same columns, of the augmented image
        TR_TRY(tr_im2col_u8_aug_bf16(u8img, pixel_lut, layout, aug, aug_noise, aug_noise_len, u16(cols), B, C, IH, IW, patch, s));
      else if (pixels)
        TR_TRY(op_im2col_u8(f32, u8img, pixel_lut, layout, cols, B, C, IH, IW, patch, s));
      else
        TR_TRY(op_im2col(f32, fimg, cols, B, C, IH, IW, patch, s));
      TR_TRY(op_gemm(prec, cols, w->patch_w, w->patch_b, x, w->pos_embed, p.P, B * p.P, D, p.kcols, TR_EPI_PATCH_F32, s));
      TR_TRY(tr_cls_pos_rows(w->cls_token, w->pos_embed, x, B, p.N0, D, s));
    }
    return drop(x, (size_t)B * p.N0 * D, true);
  }

  // what the blocks need before the first one: the fused Mlp's zeroed counters, DyViT training's all-ones policy
  int before_blocks() {
    if (one_memset) TR_TRY(tr_mlp_fused_zero_counters(ws + p.off_mlp_sk, p.mlp_sk_bytes, D, p.Hd, cfg->depth, s));
    if (train && cfg->family == TR_FAMILY_DYVIT) {
      float* ones = slot(tp->ones);
      TR_TRY(tr_fill_f32(ones, 1.0f, (size_t)B * p.N0, s));
      policy_cur = ones;
    }
    return TR_OK;
  }

  // the reduction stage in FRONT of block i, for the families that have one there
  int pre_block(int i) {
    have_xn = false;
    const bool stage = cfg->keep[i] > 0;
    switch (cfg->family) {
      case TR_FAMILY_DPCKNN: return stage ? stage_dpcknn(i) : TR_OK;
      case TR_FAMILY_KMEDOIDS: return stage ? stage_kmedoids(i) : TR_OK;
      case TR_FAMILY_HEURISTIC: return w->stage[i].w3 != nullptr ? stage_heuristic(i) : TR_OK;
      case TR_FAMILY_PATCHMERGER: return stage ? stage_patchmerger(i) : TR_OK;
      case TR_FAMILY_SINKHORN: return stage ? stage_sinkhorn(i) : TR_OK;
      case TR_FAMILY_DYVIT: return !stage ? TR_OK : train ? stage_dyvit_train(i) : stage_dyvit(i);
      case TR_FAMILY_SIT: return !stage ? TR_OK : train ? stage_sit_train(i) : stage_sit(i);
      default: return TR_OK;
    }
  }

  // DPC-KNN / K-Medoids: x += previous mlp output ahead of the clustering.  Training: the stream entering the reduction stays on the tape
  // and the block's slots take over (x1: the reduced stream, norm1's input).  The norm output of that pass is not used -- it goes to the
  // shared scratch, NOT to xn, which still names the previous block's norm2 slot on the tape.
  int enter_cluster_stage(int i) {
    const tr_block_weights* bw = &w->blocks[i];
    if (train) {
      TR_TRY(enter_stage(i, bw->ln1_g, bw->ln1_b, xn_shared, cfg->ln_eps));
      x_alt = slot(tp->blk[i].x1);
      xn = tape + tp->blk[i].xn1;
    } else if (pending) TR_TRY(op_ln(f32, x, D, pending, D, bw->ln1_g, bw->ln1_b, xn, B * N, D, cfg->ln_eps, s));
    pending = nullptr;
    return TR_OK;
  }

  // a19 + a20: CTM (dpcknn.py:153-172) on x[:, 1:] BEFORE the block; merge fused with the block's norm1
  int stage_dpcknn(int i) {
    const tr_block_weights* bw = &w->blocks[i];
    const tr_stage_weights* sw = &w->stage[i];
    const int Kc = cfg->keep[i];
    TR_REQUIRE(Kc <= N - 1, TR_ERR_CONFIG, "tr_vit_forward: block %d asks for %d clusters of %d patch tokens", i, Kc, N - 1);
    TR_TRY(enter_cluster_stage(i));
    float* cws = scratch(p.off_cluster);
    float* wtok = train ? slot(tp->blk[i].scores) : cws + tr_dpcknn_workspace_floats(B, p.N0);
    int32_t* assign = compl_dst(i);
    TR_TRY(tr_dpcknn_cluster(x, noise_in, cws, kept_dst(i), assign, scores, B, N, D, Kc, cfg->knn_k > 0 ? cfg->knn_k : 5, f32 ? 0 : 1, s));
    if (noise_in) noise_in += (size_t)B * (N - 1);
    TR_TRY(tr_cluster_merge_layernorm(x, sw->w3, sw->b3, wtok, assign, bw->ln1_g, bw->ln1_b, x_alt, xn, f32 ? 1 : 0, B, N, Kc, D, cfg->ln_eps, s));
    swap_x();
    N = Kc + 1;
    have_xn = true;
    return TR_OK;
  }

  // a21: KMedoids (kmedoids.py:135-149) on x[:, 1:] BEFORE the block: the medoid tokens replace the patch tokens
  int stage_kmedoids(int i) {
    const tr_block_weights* bw = &w->blocks[i];
    const int Kc = cfg->keep[i];
    TR_REQUIRE(i > 0, TR_ERR_CONFIG, "tr_vit_forward: K-Medoids at block 0 has no previous attention to weigh the tokens "
                                     "(the reference fails there too: `attn` is unbound, kmedoids.py:240)");
    const int kinit = cfg->kmed_init[i];             // > 0: args.equal_weight, first medoid id + 1
    TR_REQUIRE(Kc <= N - 1, TR_ERR_CONFIG, "tr_vit_forward: block %d asks for %d medoids of %d patch tokens", i, Kc, N - 1);
    TR_TRY(enter_cluster_stage(i));
    int32_t* centers = kept_dst(i);
    if (kinit > 0)
      TR_TRY(tr_kmedoids_equal(x, kinit - 1, scratch(p.off_cluster), centers, compl_dst(i), B, N, D, Kc, cfg->cluster_iters, f32 ? 0 : 1, s));
    else
      TR_TRY(tr_kmedoids(x, colsum_part, scratch(p.off_cluster), centers, compl_dst(i), B, N, D, H, Kc, cfg->cluster_iters, f32 ? 0 : 1, s));
    TR_TRY(op_gather(f32, x, nullptr, centers, nullptr, nullptr, bw->ln1_g, bw->ln1_b, x_alt, xn, B, N, Kc, D, cfg->ln_eps, s));
    swap_x();
    N = Kc + 1;
    have_xn = true;
    return TR_OK;
  }

  // f4: a new spatial mask takes effect at this block and stays until the next one (heuristic.py:247-258)
  int stage_heuristic(int i) {
    TR_REQUIRE(w->stage[i].n_pad == N, TR_ERR_CONFIG, "tr_vit_forward: block %d mask has %d entries for %d tokens", i, w->stage[i].n_pad, N);
    float* mask_dst = train ? slot(tp->blk[i].size) : size_a;      // training keeps every block's mask
    TR_TRY(tr_broadcast_rows(w->stage[i].w3, mask_dst, B, N, s));
    size_cur = mask_dst;
    return TR_OK;
  }

  // f4: PatchMerger.forward patchmerger.py:35-39 on x[:, 1:] BEFORE the block
  int stage_patchmerger(int i) {
    const tr_stage_weights* sw = &w->stage[i];
    const int Kc = cfg->keep[i];
    TR_REQUIRE(Kc <= N - 1, TR_ERR_CONFIG, "tr_vit_forward: block %d asks for %d outputs of %d patch tokens", i, Kc, N - 1);
    TR_REQUIRE(sw->ln_g && sw->ln_b && sw->w1 && sw->b1 && sw->n_pad >= Kc && sw->n_pad % 8 == 0 &&
                   sw->n_pad == trplan::soft_ld(Kc),
               TR_ERR_CONFIG, "tr_vit_forward: block %d PatchMerger weights missing or n_pad=%d invalid for K=%d", i, sw->n_pad, Kc);
    return train ? patchmerger_train(i, sw, Kc) : patchmerger_eval(sw, Kc);
  }
  // every operand of the stage's backward stays on the tape; the merged stream is written to norm1's input slot (x1: no swap, no xn)
  int patchmerger_train(int i, const tr_stage_weights* sw, int Kc) {
    const trplan::BlockTape& bt = tp->blk[i];
    const int M = B * N;
    TR_REQUIRE(sw->n_pad == trplan::soft_ld(Kc), TR_ERR_CONFIG, "tr_vit_forward_train: block %d PatchMerger n_pad=%d K=%d", i, sw->n_pad, Kc);
    float *xh = slot(bt.sxh), *slog = slot(bt.slog), *swt = slot(bt.swt);
    uint16_t* pu = slot<uint16_t>(bt.pu);
    TR_TRY(enter_stage(i, sw->ln_g, sw->ln_b, pu, 1e-5f));
    TR_TRY(tr_layernorm_f32(x, D, nullptr, D, sw->ln_g, sw->ln_b, xh, M, D, 1e-5f, s));
    TR_TRY(tr_gemm_bf16(pu, u16(sw->w1), sw->b1, slog, nullptr, 0, M, sw->n_pad, D, TR_EPI_F32, s));
    TR_REQUIRE(hipMemcpyAsync(swt, slog, (size_t)M * sw->n_pad * 4, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(s)) == hipSuccess,
               TR_ERR_LAUNCH, "tr_vit_forward_train: copy failed");
    TR_TRY(tr_softassign_merge_fast(swt, sw->n_pad, sw->scale, 1, x, xh, slot(bt.x1), soft_out, B, N, Kc, D, s));
    soft_advance(Kc);
    x = slot(bt.x1);
    N = Kc + 1;
    return TR_OK;
  }
  int patchmerger_eval(const tr_stage_weights* sw, int Kc) {
    const int M = B * N;
    float* xh = static_cast<float*>(qkv);              // LayerNorm-ed tokens, fp32 [M, D]
    float* sc = scratch(p.off_soft);                   // similarities [M, n_pad]
    TR_TRY(op_ln(f32, x, D, pending, D, sw->ln_g, sw->ln_b, xn, M, D, 1e-5f, s));        // x += previous mlp output; GEMM operand
    pending = nullptr;
    TR_TRY(tr_layernorm_f32(x, D, nullptr, D, sw->ln_g, sw->ln_b, xh, M, D, 1e-5f, s));  // the rows that are summed
    TR_TRY(op_gemm(prec, xn, sw->w1, sw->b1, sc, nullptr, 0, M, sw->n_pad, D, TR_EPI_F32, s));
    TR_TRY(soft_merge(sc, sw->n_pad, sw->scale, 1, xh, soft_out, Kc,
                      [&] { return tr_softassign_merge(sc, sw->n_pad, sw->scale, x, xh, x_alt, soft_out, B, N, Kc, D, s); }));
    soft_advance(Kc);
    swap_x();
    N = Kc + 1;
    return TR_OK;
  }

  // a22: Sinkhorn.forward sinkhorn.py:66-86 on x[:, 1:] BEFORE the block
  int stage_sinkhorn(int i) {
    const tr_stage_weights* sw = &w->stage[i];
    const int Kc = cfg->keep[i];
    TR_REQUIRE(Kc <= N - 1, TR_ERR_CONFIG, "tr_vit_forward: block %d asks for %d clusters of %d patch tokens", i, Kc, N - 1);
    TR_REQUIRE(sw->w1 && sw->b1 && sw->n_pad >= Kc && sw->n_pad % 8 == 0 && sw->n_pad == trplan::soft_ld(Kc),
               TR_ERR_CONFIG, "tr_vit_forward: block %d Sinkhorn centres missing or n_pad=%d invalid for K=%d", i, sw->n_pad, Kc);
    return train ? sinkhorn_train(i, sw, Kc) : sinkhorn_eval(i, sw, Kc);
  }
  int sinkhorn_train(int i, const tr_stage_weights* sw, int Kc) {
    const trplan::BlockTape& bt = tp->blk[i];
    const tr_block_weights* bw = &w->blocks[i];
    const int M = B * N;
    const float eps = cfg->sinkhorn_eps > 0.f ? cfg->sinkhorn_eps : 1.0f;
    TR_REQUIRE(sw->n_pad == trplan::soft_ld(Kc), TR_ERR_CONFIG, "tr_vit_forward_train: block %d Sinkhorn n_pad=%d K=%d", i, sw->n_pad, Kc);
    float *xh = slot(bt.sxh), *slog = slot(bt.slog), *swt = slot(bt.swt);
    uint16_t* pu = slot<uint16_t>(bt.pu);
    // x0 = x + pending (the norm output of this pass is not used: shared scratch)
    TR_TRY(enter_stage(i, bw->ln1_g, bw->ln1_b, xn_shared, cfg->ln_eps));
    TR_TRY(tr_rownorm(x, xh, pu, 0, M, D, s));
    TR_TRY(tr_gemm_bf16(pu, u16(sw->w1), sw->b1, slog, nullptr, 0, M, sw->n_pad, D, TR_EPI_F32, s));
    TR_TRY(tr_sinkhorn(slog, sw->n_pad, eps, cfg->cluster_iters, swt, soft_out, B, N, Kc, s));
    soft_advance(Kc);
    TR_TRY(tr_softassign_merge_fast(swt, sw->n_pad, 1.0f, 0, x, xh, slot(bt.x1), nullptr, B, N, Kc, D, s));
    x = slot(bt.x1);                                   // norm1's input slot: no swap, no xn
    N = Kc + 1;
    return TR_OK;
  }
  int sinkhorn_eval(int i, const tr_stage_weights* sw, int Kc) {
    const tr_block_weights* bw = &w->blocks[i];
    const int M = B * N;
    const float eps = cfg->sinkhorn_eps > 0.f ? cfg->sinkhorn_eps : 1.0f;
    if (pending) TR_TRY(op_ln(f32, x, D, pending, D, bw->ln1_g, bw->ln1_b, xn, M, D, cfg->ln_eps, s));   // x += previous mlp output
    pending = nullptr;
    float* xh = static_cast<float*>(qkv);              // unit-norm tokens, fp32 [M, D] (the qkv slab is free here)
    float* sc = scratch(p.off_soft);                   // scores, then the transport plan in place [M, n_pad]
    TR_TRY(tr_rownorm(x, xh, xn, f32 ? 1 : 0, M, D, s));
    TR_TRY(op_gemm(prec, xn, sw->w1, sw->b1, sc, nullptr, 0, M, sw->n_pad, D, TR_EPI_F32, s));
    TR_TRY(tr_sinkhorn(sc, sw->n_pad, eps, cfg->cluster_iters, sc, soft_out, B, N, Kc, s));
    soft_advance(Kc);
    TR_TRY(soft_merge(sc, sw->n_pad, 1.0f, 0, xh, nullptr, Kc,
                      [&] { return tr_weighted_merge(sc, sw->n_pad, x, xh, x_alt, B, N, Kc, D, s); }));
    swap_x();
    N = Kc + 1;
    return TR_OK;
  }

  // a11 / f4: DyViT TRAINING (dyvit.py:221-229): PredictorLG on the patch tokens under the previous decision, a straight-through
  // Gumbel-softmax sample becomes this stage's policy; no token is removed (N stays).  Every activation goes to the stage's tape slots.
  int stage_dyvit_train(int i) {
    const tr_stage_weights* sw = &w->stage[i];
    const trplan::BlockTape& bt = tp->blk[i];
    const int M = B * N, Hh = sw->h_pad > 0 ? sw->h_pad : D / 2, Q = (D / 4 + 63) / 64 * 64;
    TR_REQUIRE(sw->ln_g && sw->ln_b && sw->w0 && sw->b0 && sw->w1 && sw->b1 && sw->w2 && sw->b2 && sw->w3 && sw->b3, TR_ERR_NULL,
               "tr_vit_forward_train: block %d predictor weights missing", i);
    // Hh: the D/2 hidden layer as packed -- zero-padded to a multiple of 64 (DeiT-T: 96 -> 128; zero weight rows / columns and zero
    // bias: the padded activations are gelu(0) = 0 and carry no gradient), like the D/4 layer is padded to Q rows
    TR_REQUIRE(Hh >= D / 2 && Hh % 64 == 0 && Hh == (D / 2 + 63) / 64 * 64 && sw->reserved_ == Q, TR_ERR_CONFIG,
               "tr_vit_forward_train: the DyViT predictor must be packed with its hidden layers padded to %d / %d columns (got h_pad=%d, %d)",
               (D / 2 + 63) / 64 * 64, Q, sw->h_pad, sw->reserved_);
    TR_REQUIRE(noise_in != nullptr, TR_ERR_NULL, "tr_vit_forward_train: DyViT needs the Gumbel noise of every stage (noise_in)");
    uint16_t *pu = slot<uint16_t>(bt.pu), *pcat = slot<uint16_t>(bt.pcat), *ph1 = slot<uint16_t>(bt.ph1), *ph2 = slot<uint16_t>(bt.ph2);
    float* pol = slot(bt.pol);
    TR_TRY(enter_stage(i, sw->ln_g, sw->ln_b, pu, 1e-5f));
    TR_TRY(tr_gemm_gelu_keep_bf16(pu, u16(sw->w0), sw->b0, slot<uint16_t>(bt.ppre0), pcat, M, D, D, s));
    TR_TRY(tr_pool_policy(pcat, policy_cur, B, N, D, 1e-6f, s));
    TR_TRY(tr_gemm_gelu_keep_bf16(pcat, u16(sw->w1), sw->b1, slot<uint16_t>(bt.ppre1), ph1, M, Hh, D, s));
    TR_TRY(tr_gemm_gelu_keep_bf16(ph1, u16(sw->w2), sw->b2, slot<uint16_t>(bt.ppre2), ph2, M, Q, Hh, s));
    TR_TRY(tr_dyvit_decide(ph2, Q, sw->w3, sw->b3, noise_in, policy_cur, pol, slot(bt.ysoft), slot(bt.sm), slot(bt.hard), B, N, D / 4, s));
    noise_in += (size_t)B * (N - 1) * 2;
    policy_cur = pol;
    return TR_OK;
  }

  // a23 TRAINING: TokenSlimmingModule (sit.py:36-40) with every activation on the tape
  int stage_sit_train(int i) {
    const tr_stage_weights* sw = &w->stage[i];
    const trplan::BlockTape& bt = tp->blk[i];
    const int Kc = cfg->keep[i], M = B * N, Hh = (D / 2 + 63) / 64 * 64;     // hidden width as packed (DeiT-T: 96 -> 128, zero padded)
    TR_REQUIRE(Kc <= N - 1, TR_ERR_CONFIG, "tr_vit_forward_train: block %d asks for %d of %d patch tokens", i, Kc, N - 1);
    TR_REQUIRE(sw->ln_g && sw->ln_b && sw->w0 && sw->b0 && sw->w1 && sw->b1, TR_ERR_NULL, "tr_vit_forward_train: block %d SiT weights missing", i);
    TR_REQUIRE(sw->n_pad == trplan::soft_ld(Kc) && (sw->h_pad == Hh || (sw->h_pad == 0 && Hh == D / 2)), TR_ERR_CONFIG,
               "tr_vit_forward_train: the SiT module must be packed with its hidden layer padded to %d columns and n_pad == %d (got h_pad=%d n_pad=%d)",
               Hh, trplan::soft_ld(Kc), sw->h_pad, sw->n_pad);
    float *slog = slot(bt.slog), *swt = slot(bt.swt);
    uint16_t *pu = slot<uint16_t>(bt.pu), *ph0 = slot<uint16_t>(bt.pcat);
    TR_TRY(enter_stage(i, sw->ln_g, sw->ln_b, pu, 1e-5f));
    TR_TRY(tr_gemm_gelu_keep_bf16(pu, u16(sw->w0), sw->b0, slot<uint16_t>(bt.ppre0), ph0, M, Hh, D, s));
    TR_TRY(tr_gemm_bf16(ph0, u16(sw->w1), sw->b1, slog, nullptr, 0, M, sw->n_pad, Hh, TR_EPI_F32, s));
    TR_REQUIRE(hipMemcpyAsync(swt, slog, (size_t)M * sw->n_pad * 4, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(s)) == hipSuccess,
               TR_ERR_LAUNCH, "tr_vit_forward_train: copy failed");
    TR_TRY(tr_softassign_merge_fast(swt, sw->n_pad, sw->scale, 1, x, x, slot(bt.x1), soft_out, B, N, Kc, D, s));
    soft_advance(Kc);
    x = slot(bt.x1);                                   // norm1's input slot: no swap, no xn
    N = Kc + 1;
    return TR_OK;
  }

  // eval DyViT / SiT: x (+= previous mlp output), the module's own LayerNorm (nn.LayerNorm default eps 1e-5: dyvit.py:97, sit.py:30) -> xn
  int enter_module_stage(int i, const tr_stage_weights* sw, int Kc) {
    TR_REQUIRE(Kc <= N - 1, TR_ERR_CONFIG, "tr_vit_forward: block %d asks for %d of %d patch tokens", i, Kc, N - 1);
    TR_REQUIRE(sw->ln_g && sw->ln_b && sw->w0 && sw->b0 && sw->w1 && sw->b1, TR_ERR_NULL,
               "tr_vit_forward: block %d has no reduction-module weights (tr_vit_weights.stage)", i);
    TR_TRY(op_ln(f32, x, D, pending, D, sw->ln_g, sw->ln_b, xn, B * N, D, 1e-5f, s));
    pending = nullptr;
    return TR_OK;
  }

  // a10: PredictorLG (dyvit.py:113-119, policy == 1 in eval) -> score -> argsort(desc)[:K] -> batch_index_select
  int stage_dyvit(int i) {
    const tr_stage_weights* sw = &w->stage[i];
    const tr_block_weights* bw = &w->blocks[i];
    const int Kc = cfg->keep[i], M = B * N;
    TR_TRY(enter_module_stage(i, sw, Kc));
    TR_REQUIRE(sw->w2 && sw->b2 && sw->w3 && sw->b3, TR_ERR_NULL, "tr_vit_forward: block %d predictor weights missing", i);
    const int Hh = sw->h_pad > 0 ? sw->h_pad : D / 2;            // hidden width as packed (zero-padded to 64 for DeiT-T)
    TR_REQUIRE(Hh >= D / 2 && (Hh % 64 == 0 || f32), TR_ERR_CONFIG, "tr_vit_forward: DyViT predictor hidden width %d invalid (D=%d)", Hh, D);
    TR_TRY(op_gemm(prec, xn, sw->w0, sw->b0, ao, nullptr, 0, M, D, D, TR_EPI_GELU_BF16, s));
    TR_TRY(tr_pool_broadcast(ao, f32 ? 1 : 0, B, N, D, 1e-6f, s));
    TR_TRY(op_gemm(prec, ao, sw->w1, sw->b1, qkv, nullptr, 0, M, Hh, D, TR_EPI_GELU_BF16, s));
    TR_TRY(op_gemm(prec, qkv, sw->w2, sw->b2, hbuf, nullptr, 0, M, D / 4, Hh, TR_EPI_GELU_BF16, s));
    TR_TRY(tr_dyvit_score(hbuf, f32 ? 1 : 0, sw->w3, sw->b3, cls_rows, M, D / 4, s));
    int32_t* idx_dst = kept_dst(i);
    TR_TRY(tr_cls_topk(cls_rows, idx_dst, nullptr, scores, B, 1, N, Kc, s));
    TR_TRY(op_gather(f32, x, nullptr, idx_dst, nullptr, nullptr, bw->ln1_g, bw->ln1_b, x_alt, xn, B, N, Kc, D, cfg->ln_eps, s));
    have_xn = true;
    swap_x();
    N = Kc + 1;
    return TR_OK;
  }

  // a23: TokenSlimmingModule (sit.py:36-40)
  int stage_sit(int i) {
    const tr_stage_weights* sw = &w->stage[i];
    const int Kc = cfg->keep[i], M = B * N;
    TR_TRY(enter_module_stage(i, sw, Kc));
    TR_REQUIRE(sw->n_pad >= Kc && sw->n_pad % 8 == 0 && sw->n_pad == trplan::soft_ld(Kc), TR_ERR_CONFIG,
               "tr_vit_forward: block %d SiT n_pad=%d invalid for K=%d", i, sw->n_pad, Kc);
    const int Hh = sw->h_pad > 0 ? sw->h_pad : D / 2;
    TR_REQUIRE(Hh >= D / 2 && (Hh % 64 == 0 || f32), TR_ERR_CONFIG, "tr_vit_forward: SiT hidden width %d invalid (D=%d)", Hh, D);
    TR_TRY(op_gemm(prec, xn, sw->w0, sw->b0, ao, nullptr, 0, M, Hh, D, TR_EPI_GELU_BF16, s));
    float* sc = scratch(p.off_soft);                   // logits [M, n_pad]
    TR_TRY(op_gemm(prec, ao, sw->w1, sw->b1, sc, nullptr, 0, M, sw->n_pad, Hh, TR_EPI_F32, s));
    TR_TRY(soft_merge(sc, sw->n_pad, sw->scale, 1, x, soft_out, Kc,
                      [&] { return tr_sit_merge(sc, sw->n_pad, sw->scale, x, x_alt, soft_out, B, N, Kc, D, s); }));
    soft_advance(Kc);
    swap_x();
    N = Kc + 1;
    return TR_OK;
  }

  // what block i reduces inside the block, whether it runs as the CLS tail; training: its tape slots replace the shared scratch
  int begin_block(int i) {
    const int fam = cfg->family;
    Ks = fam == TR_FAMILY_ATS ? cfg->keep[i] : 0;
    K = (fam == TR_FAMILY_TOPK || fam == TR_FAMILY_EVIT) ? cfg->keep[i] : 0;
    TR_REQUIRE(K >= 0 && K <= N - 1, TR_ERR_CONFIG, "tr_vit_forward: block %d keeps %d of %d patch tokens", i, K, N - 1);
    if (K == N - 1) K = 0;  // topk.py:57 / evit.py:79: left_tokens == N-1 -> plain block
    r = 0;                  // ToMe: r = min(r, (N - protected) // 2)  (tome.py:253)
    if (fam == TR_FAMILY_TOME) {
      TR_REQUIRE(cfg->keep[i] >= 0, TR_ERR_CONFIG, "tr_vit_forward: block %d has negative ToMe r", i);
      r = cfg->keep[i] < (N - 1) / 2 ? cfg->keep[i] : (N - 1) / 2;
    }
    // CLS tail: the last block of an eval forward that reduces nothing from its attention onward and whose stream nobody reads (no Features,
    // no final tokens, no level tap of this block, no average pool).
    // K and V still come from every row (norm1 and the qkv GEMM stay full width); the attention computes the CLS query only, and proj, norm2,
    // fc1, fc2 run on the B CLS rows: per-row operations of the same kernels, so these rows come out bit for bit as in the full-width block.
    // bf16 executor only: TR_PREC_FP32 / TR_PREC_BF16X3 (validation paths) keep the full-width block.
    tail = !train && i == cfg->depth - 1 && prec == TR_PREC_BF16 && features_out == nullptr && final_tokens_out == nullptr &&
           ((level_mask >> i) & 1u) == 0 && !pool && K == 0 && r == 0 && Ks == 0 &&
           drop_keep == nullptr && drop_scale == nullptr && policy_cur == nullptr && g_cls_tail.load(std::memory_order_relaxed) != 0;
    norm2_in_mlp = false;
    if (train) {
      const trplan::BlockTape& bt = tp->blk[i];
      xn = tape + bt.xn1; qkv = tape + bt.qkv; hbuf = tape + bt.h;
      ao = Ks > 0 ? ao_shared : static_cast<void*>(tape + bt.ao);      // ATS keeps only the sampled rows of attn @ v
      dbuf = (fam == TR_FAMILY_EVIT && K > 0) ? static_cast<void*>(tape + bt.dattn) : dbuf_shared;
      x_alt = slot(bt.x2);
    }
    return TR_OK;
  }

  // x (+= previous mlp output); norm1(x) -> xn unless a stage reducer or the previous block's fused tail has written it; qkv
  int norm1_qkv(int i) {
    const tr_block_weights* bw = &w->blocks[i];
    if (train && !have_xn) {
      TR_TRY(stream_to(slot(tp->blk[i].x1), pending, bw->ln1_g, bw->ln1_b, xn, cfg->ln_eps));
    } else if (!have_xn && xn1_ready == nullptr) {
      TR_TRY(op_ln_pending(f32, x, D, pending, pending_attn, D, bw->ln1_g, bw->ln1_b, xn, B * N, D, cfg->ln_eps, s));
      pending_attn = nullptr;
    }
    TR_REQUIRE(pending_attn == nullptr, TR_ERR_CONFIG, "tr_vit_forward: internal: block %d did not absorb the lazy residual", i);
    TR_TRY(op_gemm(prec, xn1_ready ? xn1_ready : xn, bw->qkv_w, bw->qkv_b, qkv, nullptr, 0, B * N, 3 * D, D, TR_EPI_BF16, s));
    xn1_ready = nullptr;
    return TR_OK;
  }

  // ToMe: log(size) bias on the keys; ATS / Heuristic: key mask as a 1/0 "size" (log 0 = -inf -> exactly zero weight, like
  // masked_fill(-finfo.max) underflowing in the reference's softmax, ats.py:117-120)
  const float* key_size() const {
    const int fam = cfg->family;
    return (fam == TR_FAMILY_TOME || fam == TR_FAMILY_ATS || fam == TR_FAMILY_HEURISTIC) ? size_cur : nullptr;
  }

  // the whole rest of the last block on the B CLS rows; the final norm takes both residuals at row stride D
  int cls_tail(int i) {
    const tr_block_weights* bw = &w->blocks[i];
    // every buffer below holds B compact rows [B, D] (or [B, Hd]); the stream keeps its row stride N * D
    uint16_t *const ao_c = u16(ao), *const xn_c = u16(xn), *const h_c = u16(hbuf), *const d_attn = u16(dbuf_shared), *const d_mlp = u16(dbuf2);
    TR_TRY(tr_attention_cls_bf16(u16(qkv), ao_c, key_size(), B, N, H, s));
    TR_TRY(tr_gemm_bf16(ao_c, u16(bw->proj_w), bw->proj_b, d_attn, nullptr, 0, B, D, D, TR_EPI_BF16, s));
    // norm2 of x + d_attn without a stream write (lazy): the final norm adds both residuals in the reference's order
    TR_TRY(tr_layernorm2_bf16(x, (long)N * D, nullptr, 0, d_attn, D, nullptr, 0, bw->ln2_g, bw->ln2_b, xn_c, B, D, cfg->ln_eps, s));
    // the GEMM pair, not the fused Mlp: two workgroups of that kernel would be one long latency chain (same bits: tr_mlp_fused.hip)
    TR_TRY(tr_gemm_bf16(xn_c, u16(bw->fc1_w), bw->fc1_b, h_c, nullptr, 0, B, p.Hd, D, TR_EPI_GELU_BF16, s));
    TR_TRY(tr_gemm_bf16(h_c, u16(bw->fc2_w), bw->fc2_b, d_mlp, nullptr, 0, B, D, p.Hd, TR_EPI_BF16, s));
    pending_attn = d_attn;
    pending = d_mlp;
    pending_ld = D;
    if (tokens_out) tokens_out[i] = N;
    return tap_cls(i);
  }

  // CLS tap after block i: the CLS rows of x plus what is still pending, in the order the next norm adds it -- (x + attention branch) + mlp
  // branch, the fp32 additions behind viz_data["Features"][i][:, 0].  Under the CLS tail the pending rows are the compact [B, D] buffers.
  int tap_cls(int i) {
    TR_TRY(tap_level(i));
    if (cls_out == nullptr || ((tap_mask >> i) & 1u) == 0) return TR_OK;
    const long ld = (long)N * D, ldp = pending_ld > 0 ? pending_ld : ld;
    const void* first = pending_attn != nullptr ? pending_attn : pending;
    const void* second = pending_attn != nullptr ? pending : nullptr;
    TR_TRY(tr_cls_tap(x, ld, first, ldp, second, ldp, f32 ? 1 : 0, cls_out + (size_t)tap_i * D, (long)n_taps * D, B, D, s));
    ++tap_i;
    return TR_OK;
  }

  // Level tap after block i: every row of the stream plus what is still pending, added in fp32 in the order the next norm adds it -- the rows
  // of viz_data["Features"][i] (tr_cls_tap at row stride D: its arithmetic is tr_residual_snapshot's behind an eager norm2) -- or their final
  // norm (tr_final_tokens_f32).  One launch; x is not written.  Behind a fused block tail nothing is pending: the rows are x itself.
  int tap_level(int i) {
    if (level_out == nullptr || ((level_mask >> i) & 1u) == 0) return TR_OK;
    TR_REQUIRE(pending_ld == 0, TR_ERR_CONFIG, "tr_vit_forward_levels: internal: level tap of block %d behind a CLS tail", i);
    const void* first = pending_attn != nullptr ? pending_attn : pending;
    const void* second = pending_attn != nullptr ? pending : nullptr;
    float* dst = level_out + (size_t)level_i * B * p.N0 * D;
    if (level_stream != nullptr)
      TR_TRY(tr_level_tap_norm(x, first, second, f32 ? 1 : 0, w->norm_g, w->norm_b, level_stream + (size_t)level_i * B * p.N0 * D, dst, B * N, D,
                               cfg->ln_eps, s));
    else if (level_norm != 0)
      TR_TRY(tr_final_tokens_f32(x, first, second, f32 ? 1 : 0, w->norm_g, w->norm_b, dst, B * N, D, cfg->ln_eps, s));
    else
      TR_TRY(tr_cls_tap(x, D, first, D, second, D, f32 ? 1 : 0, dst, D, B * N, D, s));
    ++level_i;
    return TR_OK;
  }

  // attn(norm1(x)) -> ao   [x + proj(ao) is the reference's post-attention x, topk.py:87]
  int attention(int i) {
    if (policy_cur != nullptr)       // DyViT training: softmax_with_policy in every block (dyvit.py:245-246)
      return tr_attention_policy_bf16(u16(qkv), u16(ao), policy_cur, B, N, H, s);
    // K-Medoids: the NEXT block's clustering is seeded by the column sums of THIS block's attention (kmedoids.py:240)
    const bool want_colsum = cfg->family == TR_FAMILY_KMEDOIDS && i + 1 < cfg->depth && cfg->keep[i + 1] > 0;
    return op_attn(prec, qkv, ao, (K > 0 || Ks > 0) ? cls_rows : nullptr, key_size(), want_colsum ? colsum_part : nullptr, B, N, H, s);
  }

  // a16-a18: sample token ids on the CLS attention x |v|, keep those rows of x and of attn @ v (-> xn: proj's operand)
  int reduce_ats(int i) {
    const tr_stage_weights* sw = &w->stage[i];
    const bool dyn = cfg->ats_dynamic != 0 && !train;
    // (dynamic width: N is the batch maximum of the previous stage and may be below the static Ks; the buffers -- ids, the mask in the
    // score buffer -- are sized for the first stage's N0 rows, which bounds Ks in either mode)
    TR_REQUIRE(Ks >= 2 && (dyn ? Ks <= p.N0 : Ks <= N), TR_ERR_CONFIG, "tr_vit_forward: block %d ATS sample_count %d out of range for %d tokens", i, Ks,
               dyn ? p.N0 : N);
    TR_REQUIRE(sw->w3 && sw->n_pad >= 1, TR_ERR_NULL, "tr_vit_forward: block %d has no ATS sample grid (tr_vit_weights.stage)", i);
    int32_t* ids = kept_dst(i);
    float* mask_next = train ? slot(tp->blk[i].size) : (size_cur == size_a) ? size_b : size_a;
    int Kg = Ks;             // rows the block keeps
    if (dyn) {
      // ats.py:77-78: the reference pads the unique ids to the batch maximum -- sample at the static bound (ids [B,Ks] stay the
      // Kept_Tokens record), read that maximum back (one int: the stream is synchronised HERE), continue on the first Kg columns
      float* mask_full = scores;                                   // [B,Ks]; the score buffer is not used by this family
      int32_t* width_dev = scratch<int32_t>(p.off_misc);
      TR_TRY(tr_ats_sample(cls_rows, qkv, f32 ? 1 : 0, size_cur, sw->w3, sw->n_pad, ids, mask_full, nullptr, B, N, H, Ks, s));
      TR_TRY(tr_ats_width(mask_full, width_dev, B, Ks, s));
      int32_t width = 0;
      hipError_t e = hipMemcpyAsync(&width, width_dev, sizeof(width), hipMemcpyDeviceToHost, static_cast<hipStream_t>(s));
      if (e == hipSuccess) e = hipStreamSynchronize(static_cast<hipStream_t>(s));
      TR_REQUIRE(e == hipSuccess, TR_ERR_LAUNCH, "tr_vit_forward: ATS dynamic width read-back at block %d: %s (not capturable in a hipGraph)", i,
                 hipGetErrorString(e));
      Kg = width < 2 ? 2 : (width > Ks ? Ks : width);              // CLS + at least one column (an all-masked batch cannot occur: >= 1 sample)
      TR_TRY(tr_ats_narrow(ids, mask_full, compl_ws, mask_next, B, Ks, Kg, s));
      ids = compl_ws;
    } else {
      TR_TRY(tr_ats_sample(cls_rows, qkv, f32 ? 1 : 0, size_cur, sw->w3, sw->n_pad, ids, mask_next, nullptr, B, N, H, Ks, s));
    }
    if (train) {          // sampled rows of the stream -> x0 slot, of attn @ v -> ao slot (proj's operand); norm1's input stays in x1
      float* xg = slot(tp->blk[i].x0);
      xn = tape + tp->blk[i].ao;
      TR_TRY(tr_ats_gather(x, ao, 0, ids, xg, xn, B, N, Ks, D, s));
      x = xg;
    } else {
      TR_TRY(tr_ats_gather(x, ao, f32 ? 1 : 0, ids, x_alt, xn, B, N, Kg, D, s));
      swap_x();
    }
    size_cur = mask_next;
    N = Kg;
    return TR_OK;
  }

  // proj -> dbuf (on the rows ATS kept, where it sampled), proj_drop (topk.py:53: inside the attention module, before the branch's DropPath)
  int proj(int i) {
    const tr_block_weights* bw = &w->blocks[i];
    TR_TRY(op_gemm(prec, Ks > 0 ? xn : ao, bw->proj_w, bw->proj_b, dbuf, nullptr, 0, B * N, D, D, TR_EPI_BF16, s));
    TR_TRY(drop(dbuf, (size_t)B * N * D));
    return drop_path(i, 0);
  }

  // Top-K on the CLS attention, then residual add + gather/compact (+ EViT fused token) + norm2 in one pass
  int reduce_topk(int i) {
    const tr_block_weights* bw = &w->blocks[i];
    const bool fuse = cfg->family == TR_FAMILY_EVIT;
    int32_t* idx_dst = kept_dst(i);
    int32_t* cidx_dst = fuse ? compl_dst(i) : nullptr;
    float* sc_dst = train ? slot(tp->blk[i].scores) : scores;
    if (train) xn = tape + tp->blk[i].xn2;
    TR_TRY(tr_cls_topk(cls_rows, idx_dst, cidx_dst, sc_dst, B, H, N, K, s));
    TR_TRY(op_gather(f32, x, dbuf, idx_dst, cidx_dst, sc_dst, bw->ln2_g, bw->ln2_b, x_alt, xn, B, N, K, D, cfg->ln_eps, s));
    swap_x();
    N = K + 1 + (fuse ? 1 : 0);
    return TR_OK;
  }

  // ToMe: bipartite matching on mean-over-heads K, then residual add + size-weighted merge + norm2 in one pass
  int reduce_tome(int i) {
    const tr_block_weights* bw = &w->blocks[i];
    const int na = (N + 1) / 2;
    if (train) xn = tape + tp->blk[i].xn2;
    int32_t* unm = kept_dst(i);
    int32_t* src = unm + (size_t)B * (na - r);
    int32_t* dst = src + (size_t)B * r;
    float* size_next = train ? slot(tp->blk[i].size) : (size_cur == size_a) ? size_b : size_a;
    TR_TRY(tr_tome_match(qkv, f32 ? 1 : 0, unm, src, dst, B, N, H, r, s));
    TR_TRY(tr_tome_merge_layernorm(x, dbuf, f32 ? 1 : 0, size_cur, unm, src, dst, bw->ln2_g, bw->ln2_b, x_alt, size_next, xn, B, N, r, D,
                                   cfg->ln_eps, s));
    swap_x();
    size_cur = size_next;
    N -= r;
    return TR_OK;
  }

  // norm2 of a block that reduces nothing after its attention: on the tape, lazy, inside the fused Mlp, or eager
  int norm2(int i) {
    const tr_block_weights* bw = &w->blocks[i];
    const int M = B * N;
    if (train) {
      xn = tape + tp->blk[i].xn2;
      return stream_to(x_alt, dbuf, bw->ln2_g, bw->ln2_b, xn, cfg->ln_eps);
    }
    if (lazy_base && starts_plain(i + 1) &&
        !(rl_base && i + 1 < cfg->depth && bw->mlp_pk != nullptr && tr_mlp_fused_wanted(M, D, p.Hd, sk_ok, conc))) {
      // lazy norm2.  Where the fused Mlp follows as ONE round of blocks, the norm moves INTO that launch (tr_mlp_fused_ln_bf16: its fc1 waves
      // normalise x + dbuf in registers; bit-identical to the launch below followed by the plain fused Mlp) -- no LayerNorm launch, no bf16
      // rows in between (tr_set_mlp_ln; under the stream-K schedule the separate launch is faster: tr_mlp_fused.hip)
      norm2_in_mlp = prec == TR_PREC_BF16 && drop_keep == nullptr && bw->mlp_pk != nullptr && tr_mlp_ln_wanted(M, D, p.Hd, sk_ok, conc);
      if (!norm2_in_mlp)
        TR_TRY(tr_layernorm2_bf16(x, D, nullptr, 0, u16(dbuf), D, nullptr, 0, bw->ln2_g, bw->ln2_b, u16(xn), M, D, cfg->ln_eps, s));
      pending_attn = dbuf;
      return TR_OK;
    }
    return op_ln(f32, x, D, dbuf, D, bw->ln2_g, bw->ln2_b, xn, M, D, cfg->ln_eps, s);
  }

  // mlp(norm2(x)) -> dbuf, added to x by the next block's norm1 (or the final norm)
  int mlp(int i) {
    const tr_block_weights* bw = &w->blocks[i];
    const int M = B * N, Hd = p.Hd, cset = one_memset ? i : -1;
    bool fused = false;
    if (train) {
      TR_TRY(tr_gemm_gelu_keep_bf16(u16(xn), u16(bw->fc1_w), bw->fc1_b, slot<uint16_t>(tp->blk[i].pre), u16(hbuf), M, Hd, D, s));
    } else if (prec == TR_PREC_BF16 && bw->mlp_pk != nullptr && tr_mlp_fused_wanted(M, D, Hd, sk_ok, conc)) {
      // eval: fc1 -> GELU -> fc2 in one launch, the hidden activation never leaves the CU (tr_mlp_fused.hip; bit-identical to the pair below,
      // taken where its block schedule fills the chip)
      fused = true;
    } else {
      TR_REQUIRE(!norm2_in_mlp, TR_ERR_CONFIG, "tr_vit_forward: internal: block %d skipped its norm2 launch but does not run the fused Mlp", i);
      TR_TRY(op_gemm(prec, xn, bw->fc1_w, bw->fc1_b, hbuf, nullptr, 0, M, Hd, D, TR_EPI_GELU_BF16, s));
    }
    TR_TRY(drop(hbuf, (size_t)M * Hd));      // timm Mlp: drop after the activation ...
    // the attention residual is still pending: fc2 writes beside it.  (Eval: the toggle persists across blocks; training: begin_block re-points dbuf)
    dbuf = (pending_attn == dbuf_shared) ? dbuf2 : dbuf_shared;
    const bool fused_tail = fused && rl_base && pending_attn == nullptr && i + 1 < cfg->depth && starts_plain(i + 1);
    if (fused_tail) {
      const tr_block_weights* nb = &w->blocks[i + 1];
      TR_TRY(tr_mlp_fused_resid_ln_bf16_set(u16(xn), bw->mlp_pk, bw->fc1_b, bw->fc2_b, x, nb->ln1_g, nb->ln1_b, cfg->ln_eps, u16(hbuf), sk_scratch(),
                                            p.mlp_sk_bytes, M, D, Hd, cset, s));
      xn1_ready = hbuf;
    } else if (fused && norm2_in_mlp)
      TR_TRY(tr_mlp_fused_ln_bf16_set(x, u16(pending_attn), bw->ln2_g, bw->ln2_b, cfg->ln_eps, bw->mlp_pk, bw->fc1_b, u16(dbuf), sk_scratch(),
                                      p.mlp_sk_bytes, M, D, Hd, cset, s));
    else if (fused)
      TR_TRY(tr_mlp_fused_bf16_set(u16(xn), bw->mlp_pk, bw->fc1_b, u16(dbuf), sk_scratch(), p.mlp_sk_bytes, M, D, Hd, cset, s));
    else
      TR_TRY(op_gemm(prec, hbuf, bw->fc2_w, bw->fc2_b, dbuf, nullptr, 0, M, D, Hd, TR_EPI_BF16, s));
    TR_TRY(drop(dbuf, (size_t)M * D));       // ... and after fc2
    TR_TRY(drop_path(i, 1));
    pending = fused_tail ? nullptr : dbuf;
    if (features_out && !train) {      // viz_data["Features"][i] (topk.py:197): x + mlp output, which x itself only absorbs in the next norm
      TR_TRY(tr_residual_snapshot(x, pending, f32 ? 1 : 0, features_out, (size_t)M * D, s));
      features_out += (size_t)M * D;
    }
    if (tokens_out) tokens_out[i] = N;
    return tap_cls(i);
  }

  // a5: (x += last mlp output and) norm on the CLS rows only (LayerNorm is per-row), then the classifier -- or, headless (C == 0), the
  // normed CLS rows themselves are the output (deit_viz.py:209-212 with head = nn.Identity()): the norm writes fp32 straight into `logits`
  int final_norm_head() {
    const bool headless = p.C == 0;
    const long ld = (long)N * D, ldd_cls = pending_ld > 0 ? pending_ld : ld;
    if (final_tokens_out != nullptr) {
      // norm(x) of every row, in fp32 arithmetic, before the CLS norm below writes the stream's CLS rows: the pending residuals are full width
      TR_REQUIRE(pending_ld == 0, TR_ERR_CONFIG, "tr_vit_forward: internal: final_tokens_out behind a CLS tail");
      const void* first = pending_attn != nullptr ? pending_attn : pending;
      const void* second = pending_attn != nullptr ? pending : nullptr;
      TR_TRY(tr_final_tokens_f32(x, first, second, f32 ? 1 : 0, w->norm_g, w->norm_b, final_tokens_out, B * N, D, cfg->ln_eps, s));
    }
    if (train && features_out != nullptr) {
      // DyViT distillation (dyvit.py:252-258): the final norm of EVERY row is an output; the whole stream stays for its backward
      TR_TRY(stream_to(slot(tp->xfin_all), pending, w->norm_g, w->norm_b, xn_shared, cfg->ln_eps));
      TR_TRY(tr_layernorm_f32(x, D, nullptr, D, w->norm_g, w->norm_b, features_out, B * N, D, cfg->ln_eps, s));
      pending = nullptr;
    }
    if (train && dense_stream != nullptr) {
      // the same two launches for a dense map of the last stream: every row's final norm is an output, the whole stream stays for its backward
      TR_TRY(stream_to(dense_stream, pending, w->norm_g, w->norm_b, xn_shared, cfg->ln_eps));
      TR_TRY(tr_layernorm_f32(x, D, nullptr, D, w->norm_g, w->norm_b, dense_tokens, B * N, D, cfg->ln_eps, s));
      pending = nullptr;
    }
    if (pool) return pooled_norm_head();
    if (train && headless)          // the CLS rows entering the norm stay on the tape (xfinal) for the backward; the tape's xcls is not needed
      return tr_layernorm_bf16_f32(x, ld, slot(tp->xfinal), D, u16(pending), ld, nullptr, 0, w->norm_g, w->norm_b, logits, B, D, cfg->ln_eps, s);
    if (train) {
      xcls = tape + tp->xcls;
      TR_TRY(tr_layernorm_bf16_to(x, ld, slot(tp->xfinal), D, u16(pending), ld, w->norm_g, w->norm_b, u16(xcls), B, D, cfg->ln_eps, s));
    } else if (headless) {
      return op_ln_pending(f32, x, ld, pending, pending_attn, ldd_cls, w->norm_g, w->norm_b, logits, B, D, cfg->ln_eps, s, true);
    } else {
      TR_TRY(op_ln_pending(f32, x, ld, pending, pending_attn, ldd_cls, w->norm_g, w->norm_b, xcls, B, D, cfg->ln_eps, s));
    }
    return op_gemm(prec, xcls, w->head_w, w->head_b, logits, nullptr, 0, B, p.C, D, TR_EPI_F32, s);
  }

  // global_pool == 1 (timm's global_pool='avg' with fc_norm): the weighted mean of the patch rows of x + the pending residuals -> B rows of D
  // fp32 (training: the tape's xfinal, the final norm's input), then the same final norm and classifier on those rows -- row stride D, nothing
  // pending.  Weights: ToMe's sizes after the last merge / the ATS padding mask, none (ones) before the first such stage and in every other
  // family -- Heuristic's size_cur is a KEY mask: its tokens all stay and all count
  int pooled_norm_head() {
    const bool headless = p.C == 0;
    TR_REQUIRE(pending_ld == 0, TR_ERR_CONFIG, "tr_vit_forward: internal: average pool behind a CLS tail");
    const void* first = pending_attn != nullptr ? pending_attn : pending;
    const void* second = pending_attn != nullptr ? pending : nullptr;
    float* pooled = train ? slot(tp->xfinal) : scratch(p.off_pool);
    TR_TRY(tr_token_pool(x, first, second, f32 ? 1 : 0, trplan::pool_weighted(cfg->family) ? size_cur : nullptr, pooled, B, N, D, s));
    if (train && headless)
      return tr_layernorm_bf16_f32(pooled, D, nullptr, 0, nullptr, 0, nullptr, 0, w->norm_g, w->norm_b, logits, B, D, cfg->ln_eps, s);
    if (headless) return op_ln_pending(f32, pooled, D, nullptr, nullptr, D, w->norm_g, w->norm_b, logits, B, D, cfg->ln_eps, s, true);
    if (train) xcls = tape + tp->xcls;
    TR_TRY(op_ln(f32, pooled, D, nullptr, D, w->norm_g, w->norm_b, xcls, B, D, cfg->ln_eps, s));
    return op_gemm(prec, xcls, w->head_w, w->head_b, logits, nullptr, 0, B, p.C, D, TR_EPI_F32, s);
  }
};

}  // namespace

static int vit_forward_impl(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format, const float* pixel_lut,
                            float* logits, void* workspace, size_t workspace_bytes, int32_t* kept_idx, int32_t* compl_idx, float* soft_out,
                            const float* noise_in, float* features_out, int* tokens_out, int B, tr_stream_t s, char* tape,
                            const trplan::TapePlan* tp, const float* drop_scale = nullptr, const uint8_t* drop_keep = nullptr, float drop_rate = 0.f,
                            const tr_augment_rec* aug = nullptr, const float* aug_noise = nullptr, long aug_noise_len = 0,
                            const tr_vit_taps* taps = nullptr, const tr_vit_levels* levels = nullptr,
                            const tr_vit_dense_train* dense = nullptr, const tr_vit_train_levels* train_levels = nullptr) {
  Plan p;
  TR_REQUIRE(cfg && w && img && logits && workspace, TR_ERR_NULL, "tr_vit_forward: null pointer");
  TR_REQUIRE(make_plan(cfg, B, &p), TR_ERR_CONFIG,
             "tr_vit_forward: invalid config (need embed_dim == 64*heads, dims %% 64 == 0, classes >= 0 and %% 4 == 0, depth <= %d, "
             "global_pool 0 or 1)",
             TR_MAX_DEPTH);
  TR_REQUIRE(workspace_bytes >= p.total, TR_ERR_SHAPE, "tr_vit_forward: workspace too small (%zu < %zu)", workspace_bytes, p.total);
  TR_REQUIRE(tr_aligned16(workspace), TR_ERR_ALIGN, "tr_vit_forward: workspace must be 16-byte aligned");
  TR_REQUIRE(input_format == TR_INPUT_F32 || input_format == TR_INPUT_U8_NCHW || input_format == TR_INPUT_U8_NHWC, TR_ERR_CONFIG,
             "tr_vit_forward: input_format %d is not a TR_INPUT_* format", input_format);
  TR_REQUIRE(input_format == TR_INPUT_F32 || pixel_lut != nullptr, TR_ERR_CONFIG, "tr_vit_forward: a uint8 input needs the pixel LUT");
  TR_REQUIRE(!(cfg->global_pool == 1 && tape != nullptr && cfg->family == TR_FAMILY_DYVIT), TR_ERR_CONFIG,
             "tr_vit_forward_train: global_pool = avg is not built for DyViT in training mode (masked tokens stay in the stream under a "
             "differentiable policy, there is no token set to average over); DyViT eval pools like Top-K");
  if (taps != nullptr && (taps->cls_blocks != 0 || taps->final_tokens_out != nullptr)) {
    TR_REQUIRE(tape == nullptr, TR_ERR_CONFIG, "tr_vit_forward_taps: output taps are an eval feature");
    TR_REQUIRE(features_out == nullptr, TR_ERR_CONFIG, "tr_vit_forward_taps: output taps and features_out in one call");
    TR_REQUIRE(taps->cls_blocks == 0 || taps->cls_out != nullptr, TR_ERR_CONFIG, "tr_vit_forward_taps: cls_blocks 0x%x without cls_out",
               taps->cls_blocks);
    TR_REQUIRE(cfg->depth >= 32 || (taps->cls_blocks >> cfg->depth) == 0, TR_ERR_CONFIG,
               "tr_vit_forward_taps: cls_blocks 0x%x names a block outside 0 ... %d", taps->cls_blocks, cfg->depth - 1);
    TR_REQUIRE(tr_aligned16(taps->cls_out) && tr_aligned16(taps->final_tokens_out), TR_ERR_ALIGN,
               "tr_vit_forward_taps: tap buffers must be 16-byte aligned");
  }
  if (levels != nullptr && (levels->blocks != 0 || levels->tokens_out != nullptr)) {
    const int n_levels = __builtin_popcount(levels->blocks);
    const size_t slab = (size_t)B * p.N0 * p.D;
    TR_REQUIRE(tape == nullptr, TR_ERR_CONFIG, "tr_vit_forward_levels: level taps are an eval feature");
    TR_REQUIRE(features_out == nullptr, TR_ERR_CONFIG, "tr_vit_forward_levels: level taps and features_out in one call");
    TR_REQUIRE(levels->blocks == 0 || levels->tokens_out != nullptr, TR_ERR_CONFIG, "tr_vit_forward_levels: blocks 0x%x without tokens_out",
               levels->blocks);
    TR_REQUIRE(cfg->depth >= 32 || (levels->blocks >> cfg->depth) == 0, TR_ERR_CONFIG,
               "tr_vit_forward_levels: blocks 0x%x names a block outside 0 ... %d", levels->blocks, cfg->depth - 1);
    TR_REQUIRE(levels->norm == 0 || levels->norm == 1, TR_ERR_CONFIG, "tr_vit_forward_levels: norm %d (0 or 1)", levels->norm);
    TR_REQUIRE(levels->tokens_elems >= n_levels * slab, TR_ERR_SHAPE, "tr_vit_forward_levels: tokens_out holds %zu elements, %d levels need %zu",
               levels->tokens_elems, n_levels, n_levels * slab);
    TR_REQUIRE(tr_aligned16(levels->tokens_out), TR_ERR_ALIGN, "tr_vit_forward_levels: tokens_out must be 16-byte aligned");
  }
  tr_prof_restart();

  Fwd f(cfg, w, p, B, s, workspace, tape, tp, img, input_format, pixel_lut, aug, aug_noise, aug_noise_len, logits, kept_idx, compl_idx, soft_out,
        noise_in, features_out, tokens_out, drop_scale, drop_keep, drop_rate, taps, levels);
  if (dense != nullptr) {          // (validated by vit_forward_train_impl)
    f.dense_stream = dense->stream_out;
    f.dense_tokens = dense->tokens_out;
  }
  if (train_levels != nullptr) {   // (validated by vit_forward_train_impl)
    f.level_mask = train_levels->blocks;
    f.level_norm = train_levels->norm;
    f.level_out = train_levels->tokens_out;
    f.level_stream = train_levels->norm != 0 ? train_levels->stream_out : nullptr;
  }

  // patch_embed -> cat(cls) + pos_embed -> depth x Block -> norm -> x[:,0] -> head, with
  // Block: [stage reducer]; x += attn(norm1(x)); [in-block reducer]; x += mlp(norm2(x))
  TR_TRY(f.embed());
  TR_TRY(f.before_blocks());
  for (int i = 0; i < cfg->depth; ++i) {
    TR_TRY(f.pre_block(i));
    TR_TRY(f.begin_block(i));
    TR_TRY(f.norm1_qkv(i));
    if (f.tail) {                 // the last block, on the CLS rows: leaves the loop with both residuals pending for the final norm
      TR_TRY(f.cls_tail(i));
      break;
    }
    TR_TRY(f.attention(i));
    if (f.Ks > 0) TR_TRY(f.reduce_ats(i));
    TR_TRY(f.proj(i));
    if (f.K > 0) TR_TRY(f.reduce_topk(i));
    else if (f.r > 0) TR_TRY(f.reduce_tome(i));
    else TR_TRY(f.norm2(i));
    TR_TRY(f.mlp(i));
  }
  return f.final_norm_head();
}


extern "C" int tr_vit_forward_status(const tr_vit_config* cfg, void* workspace, size_t workspace_bytes, int B, tr_stream_t s) {
  Plan p;
  TR_REQUIRE(make_plan(cfg, B, &p), TR_ERR_CONFIG, "tr_vit_forward_status: invalid config");
  TR_REQUIRE(workspace != nullptr, TR_ERR_NULL, "tr_vit_forward_status: null workspace");
  TR_REQUIRE(workspace_bytes >= p.total, TR_ERR_SHAPE, "tr_vit_forward_status: workspace of %zu bytes, tr_vit_workspace_bytes says %zu",
             workspace_bytes, p.total);
  if (p.mlp_sk_bytes == 0) {      // nothing on this executor keeps a device-side record: the stream's own state is the status
    hipError_t e = hipStreamSynchronize(static_cast<hipStream_t>(s));
    TR_REQUIRE(e == hipSuccess, TR_ERR_LAUNCH, "tr_vit_forward_status: %s", hipGetErrorString(e));
    return TR_OK;
  }
  return tr_mlp_fused_status(static_cast<unsigned char*>(workspace) + p.off_mlp_sk, p.mlp_sk_bytes, p.D, p.Hd, s);
}

extern "C" int tr_vit_forward(const tr_vit_config* cfg, const tr_vit_weights* w, const float* img, float* logits, void* workspace,
                              size_t workspace_bytes, int32_t* kept_idx, int32_t* compl_idx, float* soft_out,
                              const float* noise_in, float* features_out, int* tokens_out, int B, tr_stream_t s) {
  return vit_forward_impl(cfg, w, img, TR_INPUT_F32, nullptr, logits, workspace, workspace_bytes, kept_idx, compl_idx, soft_out, noise_in,
                          features_out, tokens_out, B, s, nullptr, nullptr);
}

extern "C" int tr_vit_forward_pixels(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format, const float* pixel_lut,
                                     float* logits, void* workspace, size_t workspace_bytes, int32_t* kept_idx, int32_t* compl_idx,
                                     float* soft_out, const float* noise_in, float* features_out, int* tokens_out, int B, tr_stream_t s) {
  return vit_forward_impl(cfg, w, img, input_format, pixel_lut, logits, workspace, workspace_bytes, kept_idx, compl_idx, soft_out, noise_in,
                          features_out, tokens_out, B, s, nullptr, nullptr);
}

extern "C" int tr_vit_forward_taps(const tr_vit_config* cfg, const tr_vit_weights* w, const float* img, float* logits, void* workspace,
                                   size_t workspace_bytes, int32_t* kept_idx, int32_t* compl_idx, float* soft_out, const float* noise_in,
                                   float* features_out, int* tokens_out, int B, tr_stream_t s, const tr_vit_taps* taps) {
  TR_REQUIRE(taps != nullptr, TR_ERR_NULL, "tr_vit_forward_taps: null tr_vit_taps");
  return vit_forward_impl(cfg, w, img, TR_INPUT_F32, nullptr, logits, workspace, workspace_bytes, kept_idx, compl_idx, soft_out, noise_in,
                          features_out, tokens_out, B, s, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr, nullptr, 0, taps);
}

extern "C" int tr_vit_forward_pixels_taps(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format,
                                          const float* pixel_lut, float* logits, void* workspace, size_t workspace_bytes, int32_t* kept_idx,
                                          int32_t* compl_idx, float* soft_out, const float* noise_in, float* features_out, int* tokens_out,
                                          int B, tr_stream_t s, const tr_vit_taps* taps) {
  TR_REQUIRE(taps != nullptr, TR_ERR_NULL, "tr_vit_forward_pixels_taps: null tr_vit_taps");
  return vit_forward_impl(cfg, w, img, input_format, pixel_lut, logits, workspace, workspace_bytes, kept_idx, compl_idx, soft_out, noise_in,
                          features_out, tokens_out, B, s, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr, nullptr, 0, taps);
}

extern "C" int tr_vit_forward_levels(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format, const float* pixel_lut,
                                     float* logits, void* workspace, size_t workspace_bytes, int32_t* kept_idx, int32_t* compl_idx, float* soft_out,
                                     const float* noise_in, float* features_out, int* tokens_out, int B, tr_stream_t s, const tr_vit_taps* taps,
                                     const tr_vit_levels* levels) {
  TR_REQUIRE(levels != nullptr, TR_ERR_NULL, "tr_vit_forward_levels: null tr_vit_levels");
  return vit_forward_impl(cfg, w, img, input_format, pixel_lut, logits, workspace, workspace_bytes, kept_idx, compl_idx, soft_out, noise_in,
                          features_out, tokens_out, B, s, nullptr, nullptr, nullptr, nullptr, 0.f, nullptr, nullptr, 0, taps, levels);
}

extern "C" size_t tr_vit_tape_bytes(const tr_vit_config* cfg, int B) {
  Plan p;
  trplan::TokenPlan t;
  trplan::TapePlan tp;
  if (!make_plan(cfg, B, &p) || cfg->precision != TR_PREC_BF16 || !trplan::trainable_family(cfg->family)) return 0;
  // beyond 224 tokens (384 x 384 inputs) the attention backward runs key-blocked (tr_attention_bwd_long.hip)
  if (p.N0 > 640) return 0;
  if (!trplan::make_token_plan(cfg, &t) || !trplan::make_tape_plan(cfg, B, t, &tp)) return 0;
  return tp.total;
}

// offsets (bytes) of block blk's tape slots, in BlockTape order: x0,x1,xn1,qkv,ao,dattn,x2,xn2,pre,h,idx,idx2,scores,size + token
// counts n_pre,n_att,n_mlp,kk: lets a host read the decisions (kept ids, sizes) a training forward left on the tape
extern "C" int tr_vit_tape_layout(const tr_vit_config* cfg, int B, int blk, size_t* out18) {
  Plan p;
  trplan::TokenPlan t;
  trplan::TapePlan tp;
  TR_REQUIRE(cfg && out18, TR_ERR_NULL, "tr_vit_tape_layout: null pointer");
  TR_REQUIRE(make_plan(cfg, B, &p) && trplan::make_token_plan(cfg, &t) && trplan::make_tape_plan(cfg, B, t, &tp) && blk >= 0 && blk < cfg->depth,
             TR_ERR_CONFIG, "tr_vit_tape_layout: invalid config or block");
  const trplan::BlockTape& b = tp.blk[blk];
  const bool dy = cfg->family == TR_FAMILY_DYVIT;       // DyViT: the stage's one-hot decisions / policy [B,N] sit in the "scores" / "size" places
  const size_t v[18] = {b.x0, b.x1, b.xn1, b.qkv, b.ao, b.dattn, b.x2, b.xn2, b.pre, b.h, b.idx, b.idx2, dy ? b.hard : b.scores,
                        dy ? b.pol : b.size,
                        (size_t)t.n_pre[blk], (size_t)t.n_att[blk], (size_t)t.n_mlp[blk], (size_t)t.kk[blk]};
  for (int i = 0; i < 18; ++i) out18[i] = v[i];
  return TR_OK;
}

static int vit_forward_train_impl(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format, const float* pixel_lut,
                                  float* logits, void* workspace, size_t workspace_bytes, void* tape, size_t tape_bytes, const float* noise_in,
                                  float* features_out, const float* drop_scale, int* tokens_out, int B, tr_stream_t s, const uint8_t* dropout_keep,
                                  float drop_rate, const tr_augment_rec* aug = nullptr, const float* aug_noise = nullptr, long aug_noise_len = 0,
                                  const tr_vit_dense_train* dense = nullptr, const tr_vit_train_levels* levels = nullptr) {
  TR_REQUIRE(cfg && tape, TR_ERR_NULL, "tr_vit_forward_train: null pointer");
  TR_REQUIRE((dropout_keep == nullptr) == (drop_rate == 0.f) && drop_rate >= 0.f && drop_rate < 1.f, TR_ERR_CONFIG,
             "tr_vit_forward_train: dropout needs a keep mask AND 0 < drop_rate < 1 (got mask %p, rate %g)", (const void*)dropout_keep, (double)drop_rate);
  TR_REQUIRE(cfg->precision == TR_PREC_BF16, TR_ERR_CONFIG, "tr_vit_forward_train: the training path is bf16 only");
  TR_REQUIRE(trplan::trainable_family(cfg->family), TR_ERR_CONFIG, "tr_vit_forward_train: family %d has no training path yet", cfg->family);
  trplan::TokenPlan t;
  trplan::TapePlan tp;
  TR_REQUIRE(trplan::make_token_plan(cfg, &t) && trplan::make_tape_plan(cfg, B, t, &tp), TR_ERR_CONFIG, "tr_vit_forward_train: invalid config");
  TR_REQUIRE(tape_bytes >= tp.total, TR_ERR_SHAPE, "tr_vit_forward_train: tape too small (%zu < %zu)", tape_bytes, tp.total);
  TR_REQUIRE(tr_aligned16(tape), TR_ERR_ALIGN, "tr_vit_forward_train: tape must be 16-byte aligned");
  for (int i = 0; i < cfg->depth; ++i)
    TR_REQUIRE(t.n_att[i] <= 640, TR_ERR_SHAPE, "tr_vit_forward_train: %d tokens in block %d (the training path holds 640)", t.n_att[i], i);
  TR_REQUIRE(features_out == nullptr || cfg->family == TR_FAMILY_DYVIT, TR_ERR_CONFIG, "tr_vit_forward_train: features_out is DyViT's distillation output");
  if (dense == nullptr)
    return vit_forward_impl(cfg, w, img, input_format, pixel_lut, logits, workspace, workspace_bytes, nullptr, nullptr, nullptr, noise_in,
                            features_out, tokens_out, B, s, static_cast<char*>(tape), &tp, drop_scale, dropout_keep, drop_rate, aug, aug_noise,
                            aug_noise_len);
  // tr_vit_forward_train_dense: the caller's buffers, checked before any launch
  const size_t slab = (size_t)B * t.N0;
  if (levels == nullptr)
    TR_REQUIRE(dense->tokens_out && dense->stream_out, TR_ERR_NULL, "tr_vit_forward_train_dense: tokens_out / stream_out is NULL");
  else {
    // tr_vit_forward_train_levels: the last block's pair comes as a pair or not at all; the level slabs
    const int n_levels = __builtin_popcount(levels->blocks);
    TR_REQUIRE((dense->tokens_out != nullptr) == (dense->stream_out != nullptr), TR_ERR_NULL,
               "tr_vit_forward_train_levels: dense->tokens_out and dense->stream_out come together (both or neither)");
    TR_REQUIRE(levels->blocks != 0 && (cfg->depth >= 32 || (levels->blocks >> cfg->depth) == 0), TR_ERR_CONFIG,
               "tr_vit_forward_train_levels: blocks 0x%x names no block, or one outside 0 ... %d", levels->blocks, cfg->depth - 1);
    TR_REQUIRE(levels->norm == 0 || levels->norm == 1, TR_ERR_CONFIG, "tr_vit_forward_train_levels: norm %d (0 or 1)", levels->norm);
    TR_REQUIRE(levels->tokens_out && (levels->norm == 0 || levels->stream_out), TR_ERR_NULL,
               "tr_vit_forward_train_levels: tokens_out (norm == 1: or stream_out) is NULL");
    TR_REQUIRE(levels->level_elems >= n_levels * slab * cfg->embed_dim, TR_ERR_SHAPE,
               "tr_vit_forward_train_levels: the level buffers hold %zu elements, %d levels of [%d, %d, %d] need %zu", levels->level_elems, n_levels, B,
               t.N0, cfg->embed_dim, n_levels * slab * cfg->embed_dim);
    TR_REQUIRE(tr_aligned16(levels->tokens_out) && tr_aligned16(levels->stream_out), TR_ERR_ALIGN,
               "tr_vit_forward_train_levels: the level buffers must be 16-byte aligned");
  }
  TR_REQUIRE((dense->kept_idx != nullptr) == (dense->compl_idx != nullptr), TR_ERR_NULL,
             "tr_vit_forward_train_dense: kept_idx and compl_idx come together (both or neither)");
  TR_REQUIRE(dense->tokens_out == nullptr || dense->rows_elems >= slab * cfg->embed_dim, TR_ERR_SHAPE, "tr_vit_forward_train_dense: tokens_out / stream_out hold %zu elements, [%d, %d, %d] needs %zu",
             dense->rows_elems, B, t.N0, cfg->embed_dim, slab * cfg->embed_dim);
  TR_REQUIRE(dense->kept_idx == nullptr || dense->idx_elems >= slab * cfg->depth, TR_ERR_SHAPE,
             "tr_vit_forward_train_dense: kept_idx / compl_idx hold %zu elements, %d slabs of [%d, %d] need %zu", dense->idx_elems, cfg->depth, B, t.N0,
             slab * cfg->depth);
  size_t soft_need = 0;
  if (trplan::soft_family(cfg->family))
    for (int i = 0; i < cfg->depth; ++i) soft_need += t.kk[i] > 0 ? (size_t)B * t.kk[i] * (t.n_pre[i] - 1) : 0;
  TR_REQUIRE(dense->soft_out == nullptr || dense->soft_elems >= soft_need, TR_ERR_SHAPE,
             "tr_vit_forward_train_dense: soft_out holds %zu elements, the soft stages write %zu", dense->soft_elems, soft_need);
  TR_REQUIRE(tr_aligned16(dense->tokens_out) && tr_aligned16(dense->stream_out) && tr_aligned16(dense->kept_idx) && tr_aligned16(dense->compl_idx) &&
                 tr_aligned16(dense->soft_out),
             TR_ERR_ALIGN, "tr_vit_forward_train_dense: the output buffers must be 16-byte aligned");
  TR_TRY(vit_forward_impl(cfg, w, img, input_format, pixel_lut, logits, workspace, workspace_bytes, nullptr, nullptr, dense->soft_out, noise_in,
                          nullptr, tokens_out, B, s, static_cast<char*>(tape), &tp, drop_scale, dropout_keep, drop_rate, aug, aug_noise,
                          aug_noise_len, nullptr, nullptr, dense->tokens_out != nullptr ? dense : nullptr, levels));
  if (dense->kept_idx == nullptr) return TR_OK;
  // the decisions stay on the tape for the backward; the slabs take a copy of each deciding block's two slots (a slot IS a slab: B * N0 ints,
  // written by the kernels that write the eval slabs)
  hipStream_t st = static_cast<hipStream_t>(s);
  for (int i = 0; i < cfg->depth; ++i) {
    if (t.kk[i] <= 0) continue;
    const char* tb = static_cast<const char*>(tape);
    TR_REQUIRE(hipMemcpyAsync(dense->kept_idx + i * slab, tb + tp.blk[i].idx, slab * 4, hipMemcpyDeviceToDevice, st) == hipSuccess &&
                   hipMemcpyAsync(dense->compl_idx + i * slab, tb + tp.blk[i].idx2, slab * 4, hipMemcpyDeviceToDevice, st) == hipSuccess,
               TR_ERR_LAUNCH, "tr_vit_forward_train_dense: copy of block %d's decisions failed", i);
  }
  return TR_OK;
}

extern "C" int tr_vit_forward_train_dense(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format,
                                          const float* pixel_lut, const tr_augment_rec* aug, const float* aug_noise, long aug_noise_len,
                                          float* logits, void* workspace, size_t workspace_bytes, void* tape, size_t tape_bytes,
                                          const float* noise_in, const float* drop_scale, int* tokens_out, int B, tr_stream_t s,
                                          const uint8_t* dropout_keep, float drop_rate, const tr_vit_dense_train* dense) {
  TR_REQUIRE(cfg && dense, TR_ERR_NULL, "tr_vit_forward_train_dense: null config or tr_vit_dense_train");
  TR_REQUIRE(cfg->family != TR_FAMILY_DYVIT, TR_ERR_CONFIG,
             "tr_vit_forward_train_dense: DyViT keeps every token under a policy in training and has its own feature output (features_out)");
  if (aug != nullptr) {
    TR_REQUIRE(input_format == TR_INPUT_U8_NCHW || input_format == TR_INPUT_U8_NHWC, TR_ERR_CONFIG,
               "tr_vit_forward_train_dense: the augmentation runs on uint8 pixels (input_format %d)", input_format);
    TR_REQUIRE(B > 0 && B % 2 == 0, TR_ERR_SHAPE, "tr_vit_forward_train_dense: an augmented batch must be even, got B = %d", B);
  }
  return vit_forward_train_impl(cfg, w, img, input_format, pixel_lut, logits, workspace, workspace_bytes, tape, tape_bytes, noise_in, nullptr,
                                drop_scale, tokens_out, B, s, dropout_keep, drop_rate, aug, aug_noise, aug_noise_len, dense);
}

extern "C" int tr_vit_forward_train_levels(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format,
                                           const float* pixel_lut, const tr_augment_rec* aug, const float* aug_noise, long aug_noise_len,
                                           float* logits, void* workspace, size_t workspace_bytes, void* tape, size_t tape_bytes,
                                           const float* noise_in, const float* drop_scale, int* tokens_out, int B, tr_stream_t s,
                                           const uint8_t* dropout_keep, float drop_rate, const tr_vit_dense_train* dense,
                                           const tr_vit_train_levels* levels) {
  TR_REQUIRE(cfg && dense && levels, TR_ERR_NULL, "tr_vit_forward_train_levels: null config, tr_vit_dense_train or tr_vit_train_levels");
  TR_REQUIRE(cfg->family != TR_FAMILY_DYVIT, TR_ERR_CONFIG,
             "tr_vit_forward_train_levels: DyViT keeps every token under a policy in training and has its own feature output (features_out)");
  if (aug != nullptr) {
    TR_REQUIRE(input_format == TR_INPUT_U8_NCHW || input_format == TR_INPUT_U8_NHWC, TR_ERR_CONFIG,
               "tr_vit_forward_train_levels: the augmentation runs on uint8 pixels (input_format %d)", input_format);
    TR_REQUIRE(B > 0 && B % 2 == 0, TR_ERR_SHAPE, "tr_vit_forward_train_levels: an augmented batch must be even, got B = %d", B);
  }
  return vit_forward_train_impl(cfg, w, img, input_format, pixel_lut, logits, workspace, workspace_bytes, tape, tape_bytes, noise_in, nullptr,
                                drop_scale, tokens_out, B, s, dropout_keep, drop_rate, aug, aug_noise, aug_noise_len, dense, levels);
}

extern "C" int tr_vit_forward_train(const tr_vit_config* cfg, const tr_vit_weights* w, const float* img, float* logits, void* workspace,
                                    size_t workspace_bytes, void* tape, size_t tape_bytes, const float* noise_in, float* features_out,
                                    const float* drop_scale, int* tokens_out, int B, tr_stream_t s, const uint8_t* dropout_keep, float drop_rate) {
  return vit_forward_train_impl(cfg, w, img, TR_INPUT_F32, nullptr, logits, workspace, workspace_bytes, tape, tape_bytes, noise_in, features_out,
                                drop_scale, tokens_out, B, s, dropout_keep, drop_rate);
}

extern "C" int tr_vit_forward_train_pixels(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format,
                                           const float* pixel_lut, float* logits, void* workspace, size_t workspace_bytes, void* tape,
                                           size_t tape_bytes, const float* noise_in, float* features_out, const float* drop_scale, int* tokens_out,
                                           int B, tr_stream_t s, const uint8_t* dropout_keep, float drop_rate) {
  return vit_forward_train_impl(cfg, w, img, input_format, pixel_lut, logits, workspace, workspace_bytes, tape, tape_bytes, noise_in,
                                features_out, drop_scale, tokens_out, B, s, dropout_keep, drop_rate);
}

extern "C" int tr_vit_forward_train_aug(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format,
                                        const float* pixel_lut, const tr_augment_rec* aug, const float* aug_noise, long aug_noise_len,
                                        float* logits, void* workspace, size_t workspace_bytes, void* tape, size_t tape_bytes,
                                        const float* noise_in, float* features_out, const float* drop_scale, int* tokens_out, int B,
                                        tr_stream_t s, const uint8_t* dropout_keep, float drop_rate) {
  TR_REQUIRE(aug != nullptr, TR_ERR_NULL, "tr_vit_forward_train_aug: null augmentation table");
  TR_REQUIRE(input_format == TR_INPUT_U8_NCHW || input_format == TR_INPUT_U8_NHWC, TR_ERR_CONFIG,
             "tr_vit_forward_train_aug: the augmentation runs on uint8 pixels (input_format %d)", input_format);
  TR_REQUIRE(B > 0 && B % 2 == 0, TR_ERR_SHAPE, "tr_vit_forward_train_aug: the batch must be even, got B = %d", B);
  return vit_forward_train_impl(cfg, w, img, input_format, pixel_lut, logits, workspace, workspace_bytes, tape, tape_bytes, noise_in,
                                features_out, drop_scale, tokens_out, B, s, dropout_keep, drop_rate, aug, aug_noise, aug_noise_len);
}

// Bytes of the dropout keep mask of one training forward (1 byte per element, 1 = keep), in the order the forward consumes it:
// the embedded tokens [B,N0,D] (pos_drop), then per block proj's output rows [B*n_proj,D], the Mlp's hidden layer [B*n_mlp,Hd] and its
// output [B*n_mlp,D] -- the order in which the reference module draws them (topk.py:186, :53, timm Mlp).  0 = no training path.
extern "C" size_t tr_vit_dropout_mask_bytes(const tr_vit_config* cfg, int B) {
  trplan::TokenPlan t;
  if (cfg == nullptr || B <= 0 || !trplan::make_token_plan(cfg, &t)) return 0;
  const size_t D = (size_t)cfg->embed_dim, Hd = (size_t)cfg->mlp_hidden;
  size_t n = (size_t)B * t.N0 * D;
  for (int i = 0; i < cfg->depth; ++i) n += (size_t)B * (trplan::proj_rows(cfg, t, i) * D + (size_t)t.n_mlp[i] * (Hd + D));
  return n;
}
