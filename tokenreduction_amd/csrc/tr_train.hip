// Backward executor: enqueues the gradient pass of a training forward (tr_vit_forward_train) on the caller's stream.
//
// The reference's training step is `output = model(samples); loss = criterion(...); loss.backward()` (engine.py:50-76) with
// torch.autograd deriving the backward of the eager ops; under DistributedDataParallel (train.py:405-407) the parameter
// gradients are all-reduced in buckets while the backward is still running.  Here the backward is one fixed launch sequence over
// the tape the forward left (tr_plan.h): block by block in reverse, for each nn.Linear a weight-gradient GEMM that also sums the bias
// gradient (tr_linear_bwd_params) and a data-gradient GEMM (tr_gemm_bf16 on the transposed weight), the attention / LayerNorm / GELU backward
// kernels, and the backward of the block's token reduction (Top-K scatter topk.py:89-93, EViT fused token evit.py:111-123, ToMe
// merge tome.py:309-323).  A call may cover a RANGE of blocks [blk_hi .. blk_lo]: the caller walks the model in a few ranges and,
// after each, starts that range's gradient bucket on RCCL from a second stream while the next range runs (the DDP overlap).
// Host-side only: no allocation, no synchronisation -- capturable in a hipGraph.
//
// vit_backward validates, works out the frozen-unit plan, builds one Bwd and calls its steps ("The backward executor, step
// by step"); tests/test_backward_trace_gpu.py pins the launch sequence and the gradient bits.
#include "tr_common.h"
#include "tr_plan.h"

using trplan::align_up;

// tr_backward.hip: deferred reduction of the LayerNorm parameter gradients (one launch per backward call instead of one per norm)
void tr_ln_defer_begin(float* region, size_t floats, hipStream_t st);
int tr_ln_defer_flush();
void tr_ln_defer_end();
void tr_ln_defer_pause(bool on);

namespace {

struct BwdPlan {
  size_t g0, g1, gb0, gb1, gb2, dxn, dqkv, dao, dh, zeros, wsf, dscore, gfused, invmap, dxcls, dl16, dpol, dprev, dpolpart, soft_dp, soft_ds, soft_s, attn_stats, lnpart, gpool, total;
  size_t wsf_floats, lnpart_floats, zeros_floats, attn_stats_floats;
};

bool make_bwd_plan(const tr_vit_config* c, int B, const trplan::TokenPlan& t, BwdPlan* p) {
  const size_t D = c->embed_dim, Hd = c->mlp_hidden, T = (size_t)B * t.N0;
  const size_t kcols = (size_t)c->in_chans * c->patch * c->patch;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += align_up(bytes); return at; };
  p->g0 = take(T * D * 4);
  p->g1 = take(T * D * 4);
  p->gb0 = take(T * D * 2);
  p->gb1 = take(T * D * 2);
  p->gb2 = take(T * D * 2);          // spare: keeps fc2's dY alive past norm2's backward (the block's four weight gradients run as one launch)
  p->dxn = take(T * D * 2);
  p->dqkv = take(T * 3 * D * 2);
  p->dao = take(T * D * 2);
  p->dh = take(T * Hd * 2);
  size_t zmax = 3 * D > Hd ? 3 * D : Hd;          // the zero bias of every data-gradient GEMM: the widest output
  if (kcols > zmax) zmax = kcols;
  p->zeros_floats = zmax;
  p->zeros = take(zmax * 4);
  // scratch of the two-stage reductions: the largest request of any call below
  size_t f = tr_wgrad_workspace_floats((int)T, (int)(3 * D), (int)D);
  auto upd = [&](size_t v) { if (v > f) f = v; };
  upd(tr_wgrad_workspace_floats((int)T, (int)Hd, (int)D));
  upd(tr_wgrad_workspace_floats((int)T, (int)D, (int)Hd));
  upd(tr_wgrad_workspace_floats((int)T, (int)D, (int)D));
  upd(tr_wgrad_workspace_floats(B * t.P, (int)D, (int)kcols));
  upd(tr_colsum_workspace_floats((int)T, (int)(3 * D)));
  upd(tr_colsum_workspace_floats((int)T, (int)Hd));
  upd(tr_layernorm_bwd_workspace_floats((int)T, (int)D));
  if (c->num_classes > 0) upd(tr_wgrad_workspace_floats(B, c->num_classes, (int)D));      // the classifier's weight gradient (none headless)
  upd((size_t)(8 * B + 1) * (D + 4));          // tr_cluster_merge_bwd: eight workgroups per image
  upd(tr_dyvit_decide_bwd_workspace_floats(B, t.N0, (int)(D / 4)));
  upd(tr_wgrad_workspace_floats((int)T, (int)(D / 2), (int)D));
  int soft_k = 0;                    // soft-assignment families: the widest stage
  if (trplan::soft_family(c->family))
    for (int i = 0; i < c->depth; ++i) soft_k = t.kk[i] > soft_k ? t.kk[i] : soft_k;
  if (soft_k > 0) {
    upd(tr_wgrad_workspace_floats((int)T, trplan::soft_ld(soft_k), (int)D));
    upd(tr_token_softmax_bwd_workspace_floats(B, soft_k));
  }
  for (int i = 0; i < c->depth; ++i) {          // the paired weight-gradient launches of every block, at the block's own token counts
    const int M1 = B * t.n_att[i], M2 = B * t.n_mlp[i];
    const int Mp = (c->family == TR_FAMILY_ATS && t.kk[i] > 0) ? M2 : M1;
    upd(tr_linear_bwd_params2_workspace_floats(M2, (int)D, (int)Hd, M2, (int)Hd, (int)D));
    upd(tr_linear_bwd_params2_workspace_floats(Mp, (int)D, (int)D, M1, (int)(3 * D), (int)D));
    const tr_linear_grad four[4] = {{nullptr, (long)D, nullptr, (long)Hd, nullptr, nullptr, M2, (int)D, (int)Hd},
                                    {nullptr, (long)Hd, nullptr, (long)D, nullptr, nullptr, M2, (int)Hd, (int)D},
                                    {nullptr, (long)D, nullptr, (long)D, nullptr, nullptr, Mp, (int)D, (int)D},
                                    {nullptr, (long)(3 * D), nullptr, (long)D, nullptr, nullptr, M1, (int)(3 * D), (int)D}};
    upd(tr_linear_bwd_group_workspace_floats(four, 4));
  }
  p->wsf_floats = f;
  p->wsf = take(f * 4);
  p->dscore = take(T * 4);
  p->gfused = take((size_t)B * D * 4);
  p->invmap = take(T * 4);
  p->dxcls = take((size_t)B * D * 2);
  p->dl16 = c->num_classes > 0 ? take((size_t)B * c->num_classes * 2) : 0;
  p->dpol = take(T * 4);
  p->dprev = take(T * 4);
  p->dpolpart = take(T * c->num_heads * 4);
  // scratch of the key-blocked attention backward (384 x 384 inputs), sized once at the widest block
  p->attn_stats_floats = t.N0 > 224 ? tr_attention_bwd_long_workspace_floats(B, t.N0, c->num_heads) : 0;
  p->attn_stats = t.N0 > 224 ? take(p->attn_stats_floats * 4) : 0;
  p->soft_dp = p->soft_ds = p->soft_s = 0;
  if (soft_k > 0) {
    p->soft_dp = take(T * trplan::soft_ld(soft_k) * 4);
    p->soft_ds = take(T * trplan::soft_ld64(soft_k) * 2);
    p->soft_s = take(T * D * 4);
  }
  // the LayerNorm parameter-gradient partials of a pass (reduced by one launch at its end; a flush after 16 norms reuses the region from its
  // start): two norms per block, one per reduction stage that owns a norm, the final norm -- never more than 16 slices in flight
  int ln_norms = 2 * c->depth + 2;
  for (int i = 0; i < c->depth; ++i) ln_norms += c->keep[i] > 0 ? 1 : 0;
  p->lnpart_floats = (size_t)(ln_norms < 16 ? ln_norms : 16) * tr_layernorm_bwd_workspace_floats((int)T, (int)D);
  p->lnpart = take(p->lnpart_floats * 4);
  p->gpool = c->global_pool == 1 ? take((size_t)B * D * 4) : 0;      // gradient of the pooled rows fp32 [B, D] (tr_token_pool_bwd's input)
  p->total = o;
  return true;
}

#define TR_TRY(call)                \
  do {                              \
    int rc__ = (call);              \
    if (rc__ != TR_OK) return rc__; \
  } while (0)

inline float* F(const void* p) { return const_cast<float*>(static_cast<const float*>(p)); }
inline const uint16_t* U(const void* p) { return static_cast<const uint16_t*>(p); }

// A parameter unit of `grads` (the two gradients one launch produces together): 1 = present, 0 = frozen (both NULL), -1 = half-NULL.
inline int unit(const void* a, const void* b) { return (a != nullptr) == (b != nullptr) ? (a != nullptr ? 1 : 0) : -1; }
inline bool stage_any(const tr_stage_weights& g) {
  return g.ln_g || g.ln_b || g.w0 || g.b0 || g.w1 || g.b1 || g.w2 || g.b2 || g.w3 || g.b3;
}
// every gradient pointer the backward of block i's reduction stage writes through is there (w: the forward's weights)
inline bool stage_complete(const tr_vit_config* c, const tr_stage_weights& w, const tr_stage_weights& g) {
  switch (c->family) {
    case TR_FAMILY_DYVIT: return g.ln_g && g.ln_b && g.w0 && g.b0 && g.w1 && g.b1 && g.w2 && g.b2 && g.w3 && g.b3;
    case TR_FAMILY_SIT: return g.ln_g && g.ln_b && g.w0 && g.b0 && g.w1 && g.b1 && g.b2;
    case TR_FAMILY_PATCHMERGER: return g.ln_g && g.ln_b && g.w1;
    case TR_FAMILY_SINKHORN: return g.w1 != nullptr;
    case TR_FAMILY_DPCKNN: return w.w3 == nullptr || (g.w3 && g.b3);       // no score Linear with args.equal_weight
    default: return true;
  }
}

// Frozen parameters: which units of `grads` are there (1 / 0), and the block the walk stops at -- block i whose own parameter gradients
// end the walk (nothing below it takes a gradient); depth: no block takes one; -1: the embedding (or dx) does, the walk goes all the way
struct Frozen { int u_head, u_norm, u_embed, u_patch, stop; };

int frozen_plan(const tr_vit_config* cfg, const tr_vit_weights* w, const tr_vit_weights* wt, const tr_vit_weights* grads,
                const trplan::TokenPlan& t, const float* dx, Frozen* f) {
  f->u_head = cfg->num_classes > 0 ? unit(grads->head_w, grads->head_b) : 0;
  f->u_norm = unit(grads->norm_g, grads->norm_b);
  f->u_embed = unit(grads->pos_embed, grads->cls_token);
  f->u_patch = unit(grads->patch_w, grads->patch_b);
  TR_REQUIRE(f->u_head >= 0 && f->u_norm >= 0 && f->u_embed >= 0 && f->u_patch >= 0, TR_ERR_NULL,
             "tr_vit_backward: a gradient unit (head, norm, pos_embed + cls_token, patch) is half NULL: both pointers or neither");
  int stop = (f->u_embed || f->u_patch || dx != nullptr) ? -1 : cfg->depth;
  if (dx != nullptr) {
    TR_REQUIRE(wt->patch_w != nullptr, TR_ERR_NULL, "tr_vit_backward_dx: wt->patch_w (the patch weight transposed) is NULL");
    TR_REQUIRE(tr_patch_embed_dgrad_hw_supported(cfg->in_chans, trplan::img_h(cfg), trplan::img_w(cfg), cfg->patch, cfg->embed_dim), TR_ERR_SHAPE,
               "tr_vit_backward_dx: no input gradient for in_chans %d, img_size %d x %d, patch %d, embed_dim %d (tr_patch_embed_dgrad_hw)",
               cfg->in_chans, trplan::img_h(cfg), trplan::img_w(cfg), cfg->patch, cfg->embed_dim);
    TR_REQUIRE(tr_aligned16(dx), TR_ERR_ALIGN, "tr_vit_backward_dx: dx must be 16-byte aligned");
  }
  for (int i = 0; i < cfg->depth; ++i) {
    const tr_block_weights& b = grads->blocks[i];
    const int u[6] = {unit(b.ln1_g, b.ln1_b), unit(b.qkv_w, b.qkv_b), unit(b.proj_w, b.proj_b),
                      unit(b.ln2_g, b.ln2_b), unit(b.fc1_w, b.fc1_b), unit(b.fc2_w, b.fc2_b)};
    bool any = stage_any(grads->stage[i]);
    for (int k = 0; k < 6; ++k) {
      TR_REQUIRE(u[k] >= 0, TR_ERR_NULL, "tr_vit_backward: a gradient unit of block %d is half NULL: both pointers or neither", i);
      any = any || u[k] == 1;
    }
    if (any && stop == cfg->depth) stop = i;
  }
  for (int i = stop < 0 ? 0 : stop; i < cfg->depth; ++i) {
    const bool reached = i > stop || stage_any(grads->stage[i]);          // the stop block's stage runs only when it owns a gradient
    TR_REQUIRE(t.kk[i] <= 0 || !reached || stage_complete(cfg, w->stage[i], grads->stage[i]), TR_ERR_NULL,
               "tr_vit_backward: the backward reaches the reduction stage of block %d (a parameter at or below it takes a gradient) but its "
               "gradient pointers are NULL: stage modules are frozen only below the lowest block that takes a gradient", i);
  }
  f->stop = stop;
  return TR_OK;
}

// One backward call being enqueued: vit_backward builds it and calls its steps, the reference forward's order reversed.
struct Bwd {
  // ---- fixed inputs, each read once ---------------------------------------------------------------------------------------------------
  const tr_vit_config* cfg;
  const tr_vit_weights *w, *wt, *grads;
  const trplan::TokenPlan& t;
  const trplan::TapePlan& tp;
  const BwdPlan& bp;
  int B, D, H, Hd, C, kcols;
  tr_stream_t s;
  hipStream_t st;
  const char* tape_;
  char* ws_;
  int acc;                      // 1: the gradients are added to the buffers, 0: overwritten
  const float* drop_scale;      // DropPath: per block and image, attention branch then MLP branch
  const uint8_t* dropout_keep;  // Dropout keep masks in the order the forward consumed them (tr_vit_dropout_mask_bytes): [pos | block 0: proj, hidden, fc2 | block 1: ...]
  float drop_mul;
  size_t drop_off[TR_MAX_DEPTH + 1];      // where block i's masks start
  const float *dlogits, *dpred, *dfeat;
  float* dx;
  // dense feature maps (tr_vit_backward_dense): the gradient of the final norm of EVERY row (bf16, or fp32 to be rounded) and the stream that
  // entered the norm, the forward's stream_out; both NULL in every other call
  const void* dtokens = nullptr;
  bool dtokens_bf16 = false;
  const float* dstream = nullptr;
  // multi-level dense maps (tr_vit_backward_levels): per block the token gradient of the level tapped there (bf16 for lev_norm, else fp32)
  // and, for lev_norm, the stream slab that entered the final norm; NULL where the block has no level or the level no gradient.  The level
  // of block depth-1 is not here: it travels as dtokens / dstream (lev_norm) or as lev_last (fp32, the rows as they stand)
  const void* lev_dtok[TR_MAX_DEPTH] = {};
  const float* lev_stream[TR_MAX_DEPTH] = {};
  const float* lev_last = nullptr;
  bool lev_norm = false;
  // The four parameter-gradient products of a block (fc2, fc1, proj, qkv) run as ONE launch after the attention backward, when all four dY
  // exist -- provided nothing has rewritten fc2's dY (the bf16 stream gradient gb) by then: norm2's backward writes its bf16 output into the
  // spare buffer instead and the two trade places.  With DropPath / dropout the scaled dY copies live in scratch that is reused: pairs then.
  bool four;                    // the branches' dY are the stream gradient itself (no scaled / masked copies)
  int stop;                     // Frozen::stop
  bool u_head, u_norm, u_embed, u_patch;

  // ---- buffers: the stream gradient (fp32 g, its bf16 copy gb; the _alt pair is what a token-reducing block writes, gb_spare see `four`) ...
  float *g, *g_alt;
  uint16_t *gb, *gb_alt, *gb_spare;
  // ... and the scratch
  uint16_t *dxn, *dqkv, *dao, *dh, *dxcls;
  float *zeros, *wsf, *dscore, *gfused, *dpol, *dprev;
  int32_t* invmap;
  size_t wsn;

  // ---- the block being walked (begin_block) -------------------------------------------------------------------------------------------
  const trplan::BlockTape* bt = nullptr;
  const tr_block_weights *bw = nullptr, *bwt = nullptr, *bg = nullptr;
  int Na = 0, Nm = 0, M1 = 0, M2 = 0, Mp = 0, K = 0;      // tokens in the attention / the Mlp, rows of both, rows through proj, kk[i]
  const uint8_t *keep_proj = nullptr, *keep_h = nullptr, *keep_fc2 = nullptr;      // [Mp, D], [M2, Hd], [M2, D]
  tr_linear_grad LG[4];         // the weight gradients not launched yet: mlp_bwd and block_wgrads add, mlp_bwd (pairs) / block_wgrads launch
  int nlg = 0;
  const uint16_t* gy_proj = nullptr;      // proj's dY: stays valid until norm1's backward rewrites gb (ATS: the swapped-out buffer)
  const float* dcls = nullptr;  // EViT: the gradient of the CLS attention row norm2_gather leaves for attention_bwd
  bool stage_here = false;      // the block has a reduction stage that owns a gradient (block_wgrads)

  // the arguments of vit_backward, validated; every member is set here
  Bwd(const tr_vit_config* cfg_, const tr_vit_weights* w_, const tr_vit_weights* wt_, const tr_vit_weights* grads_, const trplan::TokenPlan& t_,
      const trplan::TapePlan& tp_, const BwdPlan& bp_, const Frozen& fr, int B_, tr_stream_t s_, const void* tape, void* workspace, int accumulate,
      const float* drop_scale_, const uint8_t* dropout_keep_, float drop_rate, const float* dlogits_, const float* dpred_, const float* dfeat_,
      float* dx_)
      : cfg(cfg_), w(w_), wt(wt_), grads(grads_), t(t_), tp(tp_), bp(bp_), B(B_), D(cfg_->embed_dim), H(cfg_->num_heads), Hd(cfg_->mlp_hidden),
        C(cfg_->num_classes), kcols(cfg_->in_chans * cfg_->patch * cfg_->patch), s(s_), st(static_cast<hipStream_t>(s_)),
        tape_(static_cast<const char*>(tape)), ws_(static_cast<char*>(workspace)), acc(accumulate ? 1 : 0), drop_scale(drop_scale_),
        dropout_keep(dropout_keep_), drop_mul(dropout_keep_ != nullptr ? 1.0f / (1.0f - drop_rate) : 1.0f), dlogits(dlogits_), dpred(dpred_),
        dfeat(dfeat_), dx(dx_), four(drop_scale_ == nullptr && dropout_keep_ == nullptr), stop(fr.stop), u_head(fr.u_head != 0),
        u_norm(fr.u_norm != 0), u_embed(fr.u_embed != 0), u_patch(fr.u_patch != 0), wsn(bp_.wsf_floats) {
    drop_off[0] = (size_t)B * t.N0 * D;
    for (int i = 0; i < cfg->depth; ++i) drop_off[i + 1] = drop_off[i] + (size_t)B * (trplan::proj_rows(cfg, t, i) * D + (size_t)t.n_mlp[i] * (Hd + D));
    g = ws<float>(bp.g0);
    g_alt = ws<float>(bp.g1);
    gb = ws<uint16_t>(bp.gb0);
    gb_alt = ws<uint16_t>(bp.gb1);
    gb_spare = ws<uint16_t>(bp.gb2);
    dxn = ws<uint16_t>(bp.dxn);
    dqkv = ws<uint16_t>(bp.dqkv);
    dao = ws<uint16_t>(bp.dao);
    dh = ws<uint16_t>(bp.dh);
    dxcls = ws<uint16_t>(bp.dxcls);
    zeros = ws<float>(bp.zeros);
    wsf = ws<float>(bp.wsf);
    dscore = ws<float>(bp.dscore);
    gfused = ws<float>(bp.gfused);
    dpol = ws<float>(bp.dpol);
    dprev = ws<float>(bp.dprev);
    invmap = ws<int32_t>(bp.invmap);
  }

  // ---- small helpers ------------------------------------------------------------------------------------------------------------------
  template <class T> T* ws(size_t off) const { return reinterpret_cast<T*>(ws_ + off); }
  template <class T> const T* tape(size_t off) const { return reinterpret_cast<const T*>(tape_ + off); }
  int zero(void* p, size_t bytes) {
    TR_REQUIRE(hipMemsetAsync(p, 0, bytes, st) == hipSuccess, TR_ERR_LAUNCH, "tr_vit_backward: memset failed");
    return TR_OK;
  }
  // The stream-gradient buffers move in two ways, each under ONE predicate that the step which moves them and rewind_to both read:
  // a block whose norm2 backward writes gb in place (no gather / merge between norm2 and the stream) rotates the spare in, when the
  // block's four weight gradients are one launch; every token-reducing block of the built families swaps g / gb with their _alt pair
  // once (DyViT's stages keep every token: no swap).
  bool gathers(int j) const {
    return (cfg->family == TR_FAMILY_TOPK || cfg->family == TR_FAMILY_EVIT || cfg->family == TR_FAMILY_TOME) && t.kk[j] > 0;
  }
  bool rotates_spare(int j) const { return four && !gathers(j); }
  bool swaps_stream(int j) const { return t.kk[j] > 0 && cfg->family != TR_FAMILY_DYVIT; }
  void rotate_spare() { uint16_t* tb = gb; gb = gb_spare; gb_spare = tb; }
  void swap_stream() {
    float* tg = g; g = g_alt; g_alt = tg;
    uint16_t* tb = gb; gb = gb_alt; gb_alt = tb;
  }
  // which stream-gradient buffers are current at block blk_hi: the moves of the blocks above, in a block's own order (norm2's rotation first)
  void rewind_to(int blk_hi) {
    for (int j = cfg->depth - 1; j > blk_hi; --j) {
      if (rotates_spare(j)) rotate_spare();
      if (swaps_stream(j)) swap_stream();
    }
  }
  // the last block below i (inclusive: at or below i) whose reduction is in force, or -1: kk > 0; Heuristic (kk is 0 everywhere): a
  // block that sets a key mask
  int last_reducer(int i, bool inclusive) const {
    for (int j = inclusive ? i : i - 1; j >= 0; --j)
      if (cfg->family == TR_FAMILY_HEURISTIC ? w->stage[j].w3 != nullptr : t.kk[j] > 0) return j;
    return -1;
  }
  // what that block left on the tape: ToMe token sizes / ATS and Heuristic key masks (none before the first), DyViT's policy (all ones)
  const float* size_at(int i, bool inclusive) const {
    const int j = last_reducer(i, inclusive);
    return j < 0 ? nullptr : tape<float>(tp.blk[j].size);
  }
  const float* pol_at(int i, bool inclusive) const {
    const int j = last_reducer(i, inclusive);
    return tape<float>(j < 0 ? tp.ones : tp.blk[j].pol);
  }
  // data gradient of a Linear: out [M, N] bf16 = dy [M, K] @ wT [K, N]
  int dgrad(const uint16_t* dy, const void* wT, uint16_t* out, int M, int N, int Kd) {
    return tr_gemm_bf16(dy, U(wT), zeros, out, nullptr, 0, M, N, Kd, TR_EPI_BF16, s);
  }
  // LayerNorm backward of M rows: g_out = g_in + d x (dy through the norm of x), gb_out its bf16 copy; dgamma / dbeta: the norm's unit of
  // grads (NULL: frozen).  ldgo: row stride of g_out (0: D); add: accumulate (-1: acc); idx ...: norm2_gather's scatter
  int ln_bwd(const uint16_t* dy, const float* x, const float* gamma, const void* dgamma, const void* dbeta, const float* g_in, float* g_out,
             uint16_t* gb_out, int M, float eps, long ldgo = 0, int add = -1, const int32_t* idx = nullptr, int Kk = 0, int n_in = 0, int n_out = 0,
             float* g_fused = nullptr) {
    return tr_layernorm_bwd(dy, x, D, gamma, g_in, g_in != nullptr ? D : 0, g_out, ldgo ? ldgo : D, gb_out, idx, Kk, n_in, n_out, g_fused, F(dgamma),
                            F(dbeta), add < 0 ? acc : add, wsf, wsn, M, D, eps, s);
  }
  int head_bwd() {
    return tr_head_bwd(dlogits, U(w->head_w), tape<uint16_t>(tp.xcls), dxcls, F(grads->head_w), F(grads->head_b), acc, ws<uint16_t>(bp.dl16), wsf,
                       wsn, B, C, D, s);
  }

  // ---- steps, in call order -----------------------------------------------------------------------------------------------------------
  // classifier + final norm (topk.py:201-203): the gradient enters the CLS rows of the last block's output stream (pooled head: the patch
  // rows).  *go: the walk continues into the blocks
  int head_and_final_norm(bool* go) {
    *go = false;
    const bool walk = stop < cfg->depth;          // a block (or the embedding) takes a gradient: the stream gradient is needed
    if (!walk && !u_norm) return u_head ? head_bwd() : TR_OK;       // head-only probe: the classifier's parameter gradients and nothing else
    TR_TRY(zero(zeros, bp.zeros_floats * 4));
    const int Nl = t.n_mlp[cfg->depth - 1];
    TR_TRY(C == 0 ? tr_f32_to_bf16(dlogits, dxcls, (size_t)B * D, s) : head_bwd());
    // average-pooled head: xfinal holds the pooled patch tokens; the norm's row gradient goes to a [B, D] buffer and tr_token_pool_bwd
    // spreads it over the patch rows with the forward's weights (the sizes / the mask the last merging / sampling block left on the tape;
    // no gradient with respect to them) -- it writes every element of g, the CLS rows' zeros included: no memset
    const bool pool = cfg->global_pool == 1;
    float* gpool = pool ? ws<float>(bp.gpool) : nullptr;
    if (pool)
      TR_REQUIRE(cfg->family != TR_FAMILY_DYVIT, TR_ERR_CONFIG, "tr_vit_backward: global_pool = avg is not built for DyViT in training mode");
    else
      TR_TRY(zero(g, (size_t)B * Nl * D * 4));
    TR_TRY(ln_bwd(dxcls, tape<float>(tp.xfinal), w->norm_g, grads->norm_g, grads->norm_b, nullptr, pool ? gpool : g, nullptr, B, cfg->ln_eps,
                  pool ? D : (long)Nl * D));
    if (pool) {
      if (!walk && dtokens == nullptr) return TR_OK;      // the final norm was the lowest parameter
      if (walk) TR_TRY(tr_token_pool_bwd(gpool, trplan::pool_weighted(cfg->family) ? size_at(cfg->depth - 1, true) : nullptr, g, B, Nl, D, s));
    }
    if (dfeat != nullptr) {
      // distillation: gradient wrt the final norm of every row (dyvit.py:252): a second pass of the norm's backward over all rows
      TR_REQUIRE(cfg->family == TR_FAMILY_DYVIT, TR_ERR_CONFIG, "tr_vit_backward: dfeat is DyViT's distillation gradient");
      TR_TRY(tr_f32_to_bf16(dfeat, dxn, (size_t)B * Nl * D, s));
      TR_TRY(ln_bwd(dxn, tape<float>(tp.xfin_all), w->norm_g, grads->norm_g, grads->norm_b, g, g, nullptr, B * Nl, cfg->ln_eps, 0, 1));
    }
    if (dtokens != nullptr) {
      // dense map: the same second pass for every family, on the caller's copy of the stream.  It adds into g -- the CLS rows' gradient, or
      // the pool's spread -- and into the norm's parameter gradients; with a pooled head and no walk g holds nothing and is only scratch
      const uint16_t* dy = U(dtokens);
      if (!dtokens_bf16) {
        TR_TRY(tr_f32_to_bf16(static_cast<const float*>(dtokens), dxn, (size_t)B * Nl * D, s));
        dy = dxn;
      }
      TR_TRY(ln_bwd(dy, dstream, w->norm_g, grads->norm_g, grads->norm_b, (pool && !walk) ? nullptr : g, g, nullptr, B * Nl, cfg->ln_eps, 0, 1));
    }
    if (!walk) return TR_OK;      // the final norm was the lowest parameter
    // the last block's level taken as it stands: its gradient is the stream gradient's own (the bf16 copy is made below)
    if (lev_last != nullptr) TR_TRY(tr_stream_grad_add(lev_last, g, nullptr, (size_t)B * Nl * D, s));
    TR_TRY(tr_f32_to_bf16(g, gb, (size_t)B * Nl * D, s));
    if (cfg->family == TR_FAMILY_DYVIT) TR_TRY(zero(dpol, (size_t)B * t.N0 * 4));
    *go = true;
    return TR_OK;
  }

  void begin_block(int i) {
    bt = &tp.blk[i];
    bw = &w->blocks[i];
    bwt = &wt->blocks[i];
    bg = &grads->blocks[i];
    Na = t.n_att[i];
    Nm = t.n_mlp[i];
    M1 = B * Na;
    M2 = B * Nm;
    K = t.kk[i];
    Mp = (int)trplan::proj_rows(cfg, t, i) * B;      // ATS: only the sampled rows went through proj (ats.py:86,129)
    keep_proj = dropout_keep ? dropout_keep + drop_off[i] : nullptr;
    keep_h = dropout_keep ? keep_proj + (size_t)Mp * D : nullptr;
    keep_fc2 = dropout_keep ? keep_h + (size_t)M2 * Hd : nullptr;
    nlg = 0;
    gy_proj = nullptr;
    dcls = nullptr;
    stage_here = false;
  }

  // A level tapped after block i: its gradient joins g, here the gradient of the summed stream after block i (B * Nm rows), before the block's
  // first step.  Through the final norm: the norm's backward over all rows, as the last block's second pass -- adds into g, rewrites gb, adds
  // into the norm's parameter gradients, reduced at once (the deferred table must not hold two segments with one destination).  As it stands:
  // g += dtok, gb = bf16(g).
  int level_inject(int i) {
    if (lev_dtok[i] == nullptr) return TR_OK;
    if (!lev_norm) return tr_stream_grad_add(static_cast<const float*>(lev_dtok[i]), g, gb, (size_t)M2 * D, s);
    tr_ln_defer_pause(true);
    const int rc = ln_bwd(U(lev_dtok[i]), lev_stream[i], w->norm_g, grads->norm_g, grads->norm_b, g, g, gb, M2, cfg->ln_eps, 0, 1);
    tr_ln_defer_pause(false);
    return rc;
  }
  // The levels below the stop block of a partly frozen model: nobody reads their stream gradient, but a trainable final norm still takes its
  // parameter gradients from them -- descending block order, g (dead by now) as scratch
  int levels_below_stop() {
    if (!lev_norm || !u_norm) return TR_OK;
    for (int i = (stop < cfg->depth - 1 ? stop : cfg->depth - 1) - 1; i >= 0; --i) {
      if (lev_dtok[i] == nullptr) continue;
      tr_ln_defer_pause(true);
      const int rc = ln_bwd(U(lev_dtok[i]), lev_stream[i], w->norm_g, grads->norm_g, grads->norm_b, nullptr, g, nullptr, B * t.n_mlp[i], cfg->ln_eps, 0, 1);
      tr_ln_defer_pause(false);
      TR_TRY(rc);
    }
    return TR_OK;
  }

  // mlp: x2 -> norm2 -> fc1 -> gelu -> fc2 -> (+ residual), down to norm2's dY in dxn
  int mlp_bwd(int i) {
    const uint16_t* gy = gb;          // the branch's dY: the stream gradient, times the branch's DropPath scale when there is one
    if (drop_scale != nullptr) {
      TR_TRY(tr_rowscale_bf16(gb, dao, drop_scale + (size_t)(2 * i + 1) * B, B, Nm, D, s));
      gy = dao;
    }
    if (dropout_keep != nullptr) {    // the Mlp's second dropout (after fc2): the same mask on fc2's dY
      TR_TRY(tr_dropout_bf16(gy, dao, keep_fc2, drop_mul, (size_t)M2 * D, s));
      gy = dao;
    }
    TR_TRY(tr_gemm_dgelu_bf16(gy, U(bwt->fc2_w), tape<uint16_t>(bt->pre), dh, M2, Hd, D, s));          // d fc2 input, times gelu'(pre): d pre
    if (dropout_keep != nullptr)      // ... and the first one (after the activation): d pre = (dY W) * keep/(1-p) * gelu'(pre), the factors commute
      TR_TRY(tr_dropout_bf16(dh, dh, keep_h, drop_mul, (size_t)M2 * Hd, s));
    // fc2's and fc1's parameter gradients: both dY (gy, dh) exist now; launched here as a pair, or with proj's and qkv's by block_wgrads
    // (a frozen layer is left out of the list: what remains is planned as a group of its own; an empty list launches nothing)
    if (bg->fc2_w != nullptr) LG[nlg++] = {gy, (long)D, tape<uint16_t>(bt->h), (long)Hd, F(bg->fc2_w), F(bg->fc2_b), M2, D, Hd};
    if (bg->fc1_w != nullptr) LG[nlg++] = {dh, (long)Hd, tape<uint16_t>(bt->xn2), (long)D, F(bg->fc1_w), F(bg->fc1_b), M2, Hd, D};
    if (!four) TR_TRY(launch_wgrads());
    return dgrad(dh, bwt->fc1_w, dxn, M2, D, Hd);
  }
  int launch_wgrads() {
    if (nlg > 0) TR_TRY(tr_linear_bwd_group(LG, nlg, acc, wsf, wsn, s));
    nlg = 0;
    return TR_OK;
  }

  // norm2 (+ the block's in-block token reduction)
  int norm2_bwd(int i) {
    const int f = cfg->family;
    if (swaps_stream(i) && (f == TR_FAMILY_TOPK || f == TR_FAMILY_EVIT)) return norm2_gather(i);
    if (swaps_stream(i) && f == TR_FAMILY_TOME) return norm2_tome(i);
    return norm2_plain(i);
  }
  // Top-K / EViT: the kept rows' gradients scatter back to the rows they were gathered from (EViT: + the fused token's backward)
  int norm2_gather(int i) {
    const bool fuse = cfg->family == TR_FAMILY_EVIT;
    TR_TRY(zero(g_alt, (size_t)M1 * D * 4));
    TR_TRY(zero(gb_alt, (size_t)M1 * D * 2));
    TR_TRY(ln_bwd(dxn, tape<float>(bt->x2), bw->ln2_g, bg->ln2_g, bg->ln2_b, g, g_alt, gb_alt, M2, cfg->ln_eps, 0, -1, tape<int32_t>(bt->idx), K, Nm,
                  Na, fuse ? gfused : nullptr));
    if (fuse) {
      TR_TRY(zero(dscore, (size_t)M1 * 4));
      TR_TRY(tr_evit_fuse_bwd(tape<float>(bt->x1), tape<uint16_t>(bt->dattn), tape<int32_t>(bt->idx2), tape<float>(bt->scores), gfused, g_alt,
                              gb_alt, dscore, B, Na, K, D, s));
      dcls = dscore;
    }
    swap_stream();
    return TR_OK;
  }
  int norm2_tome(int i) {
    TR_TRY(ln_bwd(dxn, tape<float>(bt->x2), bw->ln2_g, bg->ln2_g, bg->ln2_b, g, g, nullptr, M2, cfg->ln_eps));
    const int na = (Na + 1) / 2;
    const int32_t* unm = tape<int32_t>(bt->idx);
    const int32_t* src = unm + (size_t)B * (na - K);
    const int32_t* dst = src + (size_t)B * K;
    // sizes entering this block's merge: after the previous merging block
    TR_TRY(tr_tome_merge_bwd(g, size_at(i, false), tape<float>(bt->size), unm, src, dst, invmap, g_alt, gb_alt, B, Na, K, D, s));
    swap_stream();
    return TR_OK;
  }
  int norm2_plain(int i) {
    TR_TRY(ln_bwd(dxn, tape<float>(bt->x2), bw->ln2_g, bg->ln2_g, bg->ln2_b, g, g, rotates_spare(i) ? gb_spare : gb, M2, cfg->ln_eps));
    if (rotates_spare(i)) rotate_spare();       // gb_spare: fc2's dY, until this block's weight-gradient launch
    return TR_OK;
  }

  // proj: DropPath / proj_drop on its dY, the data gradient into dao (ATS: scattered back to the rows the block sampled from)
  int proj_bwd(int i) {
    const uint16_t* gy = gb;
    if (drop_scale != nullptr) {
      TR_TRY(tr_rowscale_bf16(gb, dh, drop_scale + (size_t)(2 * i) * B, B, Mp / B, D, s));
      gy = dh;
    }
    if (dropout_keep != nullptr) {    // proj_drop (topk.py:53): the same mask on proj's dY
      TR_TRY(tr_dropout_bf16(gy, dh, keep_proj, drop_mul, (size_t)Mp * D, s));
      gy = dh;
    }
    gy_proj = gy;
    if (!(swaps_stream(i) && cfg->family == TR_FAMILY_ATS)) return dgrad(gy, bwt->proj_w, dao, M1, D, D);
    // d(attn @ v) of the sampled rows and the stream's gradient go back to the rows they were sampled from (ats.py:86,157)
    TR_TRY(dgrad(gy, bwt->proj_w, dxn, Mp, D, D));
    TR_TRY(zero(g_alt, (size_t)M1 * D * 4));
    TR_TRY(zero(dao, (size_t)M1 * D * 2));
    TR_TRY(tr_ats_scatter(g, dxn, tape<int32_t>(bt->idx), g_alt, dao, B, Na, Nm, D, s));
    swap_stream();          // gb is rewritten by norm1's backward (qkv_norm1_bwd)
    return TR_OK;
  }

  // softmax(q k^T) v: dao -> dqkv; the policy (DyViT), key-blocked (more than 224 tokens: 384 x 384 inputs) and short forms
  int attention_bwd(int i) {
    const int f = cfg->family;
    const uint16_t* qkv = tape<uint16_t>(bt->qkv);
    float* stats = ws<float>(bp.attn_stats);
    if (f == TR_FAMILY_DYVIT) {
      const float* pol = pol_at(i, true);      // the policy this block attended under: the last predictor stage at or before it
      float* dpart = ws<float>(bp.dpolpart);
      if (Na > 224)
        TR_TRY(tr_attention_policy_bwd_long_bf16(qkv, dao, pol, dqkv, dpart, stats, bp.attn_stats_floats, B, Na, H, s));
      else
        TR_TRY(tr_attention_policy_bwd_bf16(qkv, dao, pol, dqkv, dpart, B, Na, H, s));
      return tr_head_sum(dpart, dpol, B, H, Na, s);
    }
    // ToMe: log(size) bias of this block's keys (tome.py:48-49), ATS: the key mask (ats.py:117-120) -- what the last block BELOW left;
    // Heuristic: the spatial key mask in force at this block, the last one set at or before it
    const float* size_att = (f == TR_FAMILY_TOME || f == TR_FAMILY_ATS) ? size_at(i, false) : f == TR_FAMILY_HEURISTIC ? size_at(i, true) : nullptr;
    if (Na > 224) return tr_attention_bwd_long_bf16(qkv, dao, size_att, dcls, dqkv, stats, bp.attn_stats_floats, B, Na, H, s);
    return tr_attention_bwd_bf16(qkv, dao, size_att, dcls, dqkv, B, Na, H, s);
  }

  // the block's parameter gradients (dY: the branch gradients kept above, dh and dqkv): one launch for all four, or the second pair.
  // *done: this is the stop block and what follows only feeds the blocks below (no norm1 parameters, no stage that owns a gradient)
  int block_wgrads(int i, bool* done) {
    if (bg->proj_w != nullptr) LG[nlg++] = {gy_proj, (long)D, tape<uint16_t>(bt->ao), (long)D, F(bg->proj_w), F(bg->proj_b), Mp, D, D};
    if (bg->qkv_w != nullptr) LG[nlg++] = {dqkv, (long)(3 * D), tape<uint16_t>(bt->xn1), (long)D, F(bg->qkv_w), F(bg->qkv_b), M1, 3 * D, D};
    TR_TRY(launch_wgrads());
    stage_here = K > 0 && stage_any(grads->stage[i]);
    *done = i == stop && bg->ln1_g == nullptr && !stage_here;
    return TR_OK;
  }

  // qkv's data gradient and norm1.  *done: this is the stop block and its stage owns no gradient
  int qkv_norm1_bwd(int i, bool* done) {
    TR_TRY(dgrad(dqkv, bwt->qkv_w, dxn, M1, D, 3 * D));
    const float* x1 = tape<float>(bt->x1);
    if (swaps_stream(i) && cfg->family == TR_FAMILY_KMEDOIDS) {
      // norm1 ran on the gathered medoid rows (kmedoids.py:243-248): its backward scatter-ADDS into the pre-reduction stream's gradient
      const size_t nfull = (size_t)B * t.n_pre[i] * D;
      TR_TRY(zero(g_alt, nfull * 4));
      TR_TRY(tr_layernorm_bwd_scatter_add(dxn, x1, bw->ln1_g, g, g_alt, tape<int32_t>(bt->idx), K, t.n_pre[i], F(bg->ln1_g), F(bg->ln1_b), acc, wsf,
                                          wsn, M1, D, cfg->ln_eps, s));
      if (i > stop) TR_TRY(tr_f32_to_bf16(g_alt, gb_alt, nfull, s));          // (the bf16 copy only feeds the blocks below)
      swap_stream();
    } else {
      TR_TRY(ln_bwd(dxn, x1, bw->ln1_g, bg->ln1_g, bg->ln1_b, g, g, gb, M1, cfg->ln_eps));
    }
    *done = i == stop && !stage_here;
    return TR_OK;
  }

  // the reduction stage in front of the block
  int stage_bwd(int i) {
    const int f = cfg->family;
    if (f == TR_FAMILY_DYVIT) return K > 0 ? stage_dyvit_bwd(i) : TR_OK;       // (a predictor stage moves no buffer: not under swaps_stream)
    if (!swaps_stream(i)) return TR_OK;
    if (trplan::soft_family(f)) return stage_soft_bwd(i);
    return f == TR_FAMILY_DPCKNN ? stage_dpcknn_bwd(i) : TR_OK;
  }
  // PredictorLG + Gumbel straight-through of this stage (dyvit.py:221-224), backwards.  d keep = the policy gradient collected
  // from the blocks that attended under this stage's policy (+ the later stage's d prev_decision) + d out_pred_prob
  int stage_dyvit_bwd(int i) {
    const tr_stage_weights *sw = &w->stage[i], *swt = &wt->stage[i], *sg = &grads->stage[i];
    // Hr: the predictor's real hidden width (the shapes of the parameter gradients); Hh: as packed and as laid out on the tape
    // (DeiT-T: 96 -> 128 with zero weights: the padded columns of every activation and gradient are zero)
    const int Hr = D / 2, Hh = (D / 2 + 63) / 64 * 64, Q = (D / 4 + 63) / 64 * 64, Cq = D / 4;
    int stage = 0;
    for (int j = 0; j < i; ++j) stage += t.kk[j] > 0 ? 1 : 0;
    if (dpred != nullptr) TR_TRY(tr_add_patch_rows(dpol, dpred + (size_t)stage * B * t.P, B, Na, s));
    const float* prev = pol_at(i, false);       // prev_decision entering this stage, [B,N] layout
    TR_TRY(zero(dprev, (size_t)M1 * 4));
    uint16_t *d2 = dqkv, *d1 = dao, *d0 = dh;   // scratch: [M1, Q], [M1, Hh], [M1, D]
    TR_TRY(tr_dyvit_decide_bwd(dpol, prev, tape<float>(bt->hard), tape<float>(bt->ysoft), tape<float>(bt->sm), tape<uint16_t>(bt->ph2), Q, sw->w3, d2,
                               dprev, F(sg->w3), F(sg->b3), acc, wsf, wsn, B, Na, Cq, s));
    TR_TRY(tr_gelu_bwd_bf16(tape<uint16_t>(bt->ppre2), d2, (size_t)M1 * Q, s));
    TR_TRY(tr_linear_bwd_params(d2, Q, 0, tape<uint16_t>(bt->ph1), Hh, F(sg->w2), F(sg->b2), acc, wsf, wsn, M1, Cq, Hr, s));
    TR_TRY(tr_gemm_dgelu_bf16(d2, U(swt->w2), tape<uint16_t>(bt->ppre1), d1, M1, Hh, Q, s));
    TR_TRY(tr_linear_bwd_params(d1, Hh, 0, tape<uint16_t>(bt->pcat), D, F(sg->w1), F(sg->b1), acc, wsf, wsn, M1, Hr, D, s));
    TR_TRY(dgrad(d1, swt->w1, dxn, M1, D, Hh));          // d [local | global]
    TR_TRY(tr_pool_policy_bwd(dxn, tape<uint16_t>(bt->ppre0), tape<uint16_t>(bt->pcat), prev, d0, dprev, B, Na, D, s));
    TR_TRY(tr_gelu_bwd_bf16(tape<uint16_t>(bt->ppre0), d0, (size_t)M1 * D, s));
    TR_TRY(tr_linear_bwd_params(d0, D, 0, tape<uint16_t>(bt->pu), D, F(sg->w0), F(sg->b0), acc, wsf, wsn, M1, D, D, s));
    TR_TRY(dgrad(d0, swt->w0, dxn, M1, D, D));
    TR_TRY(ln_bwd(dxn, tape<float>(bt->x0), sw->ln_g, sg->ln_g, sg->ln_b, g, g, gb, M1, 1e-5f));
    // what is left of the policy gradient belongs to the previous stage's decision
    TR_REQUIRE(hipMemcpyAsync(dpol, dprev, (size_t)M1 * 4, hipMemcpyDeviceToDevice, st) == hipSuccess, TR_ERR_LAUNCH, "tr_vit_backward: copy failed");
    return TR_OK;
  }
  // soft-assignment stage before the block (sit.py:36-40, patchmerger.py:35-39, sinkhorn.py:66-86): g = d of the merged stream
  // [B, K+1, D] -> the stream entering the stage [B, n_pre, D] + the stage's parameters (tr_soft_bwd.hip)
  int stage_soft_bwd(int i) {
    const tr_stage_weights *sw = &w->stage[i], *swt = &wt->stage[i], *sg = &grads->stage[i];
    const int Np = t.n_pre[i], Ms = B * Np, ld = trplan::soft_ld(K), ld64 = trplan::soft_ld64(K);
    const bool sit = cfg->family == TR_FAMILY_SIT, sink = cfg->family == TR_FAMILY_SINKHORN;
    const float *x0 = tape<float>(bt->x0), *wts = tape<float>(bt->swt), *slog = tape<float>(bt->slog);
    float* dwt = ws<float>(bp.soft_dp);
    uint16_t* ds = ws<uint16_t>(bp.soft_ds);
    float* dsrc = sit ? g_alt : ws<float>(bp.soft_s);       // SiT sums the stream's own rows: d src IS a stream gradient
    TR_TRY(zero(ds, (size_t)Ms * ld64 * 2));
    TR_TRY(zero(dsrc, (size_t)Ms * D * 4));
    TR_TRY(tr_soft_dweights(g, sit ? x0 : tape<float>(bt->sxh), dwt, ld, B, Np, K, D, s));
    TR_TRY(tr_soft_dsrc(g, wts, ld, dsrc, B, Np, K, D, s));
    if (sink)
      TR_TRY(tr_sinkhorn_bwd(slog, dwt, ld, cfg->sinkhorn_eps > 0.f ? cfg->sinkhorn_eps : 1.0f, cfg->cluster_iters, ds, ld64, B, Np, K, s));
    else
      TR_TRY(tr_token_softmax_bwd(wts, dwt, slog, ld, sw->scale, ds, ld64, sit ? F(sg->b2) : nullptr, acc, wsf, wsn, B, Np, K, s));
    if (sit) {
      TR_TRY(soft_sit_scores_bwd(ds, swt, sg, Ms, ld, ld64));
    } else {      // the similarity / score product: d queries (d centres) and d of its token operand
      TR_TRY(tr_wgrad_bf16(ds, ld64, 0, tape<uint16_t>(bt->pu), D, F(sg->w1), acc, wsf, wsn, Ms, ld, D, s));
      TR_TRY(dgrad(ds, swt->w1, dxn, Ms, D, ld64));
      TR_TRY(zero(g_alt, (size_t)Ms * D * 4));
    }
    if (sink) TR_TRY(tr_rownorm_bwd(x0, dsrc, dxn, g_alt, Ms, D, s));            // d unit-norm rows = merge part + score-product part
    // the CLS row passes the stage untouched
    TR_REQUIRE(hipMemcpy2DAsync(g_alt, (size_t)Np * D * 4, g, (size_t)(K + 1) * D * 4, (size_t)D * 4, B, hipMemcpyDeviceToDevice, st) == hipSuccess,
               TR_ERR_LAUNCH, "tr_vit_backward: copy failed");
    if (sink) {
      TR_TRY(tr_f32_to_bf16(g_alt, gb_alt, (size_t)Ms * D, s));
    } else {
      if (!sit) TR_TRY(tr_add_into_bf16(dsrc, dxn, (size_t)Ms * D, s));          // PatchMerger sums the LayerNorm output: both uses meet here
      TR_TRY(ln_bwd(dxn, x0, sw->ln_g, sg->ln_g, sg->ln_b, g_alt, g_alt, gb_alt, Ms, 1e-5f));
    }
    swap_stream();
    return TR_OK;
  }
  // SiT's score Mlp (Linear -> GELU -> Linear), backwards: ds [Ms, ld64] -> dxn
  int soft_sit_scores_bwd(const uint16_t* ds, const tr_stage_weights* swt, const tr_stage_weights* sg, int Ms, int ld, int ld64) {
    const int Hr = D / 2, Hh = (D / 2 + 63) / 64 * 64;     // real / packed hidden width (DeiT-T: 96 / 128)
    uint16_t* d1 = dh;                    // [Ms, Hh]
    TR_TRY(tr_linear_bwd_params(ds, ld64, 0, tape<uint16_t>(bt->pcat), Hh, F(sg->w1), F(sg->b1), acc, wsf, wsn, Ms, ld, Hr, s));
    TR_TRY(tr_gemm_dgelu_bf16(ds, U(swt->w1), tape<uint16_t>(bt->ppre0), d1, Ms, Hh, ld64, s));
    TR_TRY(tr_linear_bwd_params(d1, Hh, 0, tape<uint16_t>(bt->pu), D, F(sg->w0), F(sg->b0), acc, wsf, wsn, Ms, Hr, D, s));
    return dgrad(d1, swt->w0, dxn, Ms, D, Hh);
  }
  // CTM before the block (dpcknn.py:257-260): gradient of the merged tokens -> the tokens they were merged from + the score Linear
  int stage_dpcknn_bwd(int i) {
    TR_TRY(tr_cluster_merge_bwd(g, tape<float>(bt->x0), tape<float>(bt->x1), tape<float>(bt->scores), tape<int32_t>(bt->idx2), w->stage[i].w3, g_alt,
                                gb_alt, F(grads->stage[i].w3), F(grads->stage[i].b3), acc, wsf, wsn, B, t.n_pre[i], K, D, s));
    swap_stream();
    return TR_OK;
  }

  // embedding (topk.py:181-186): g is d x0 [B, N0, D]
  int embed_bwd() {
    if (dropout_keep != nullptr) {      // pos_drop (topk.py:186): on the stream gradient and on its bf16 copy (the patch projection's dY)
      TR_TRY(tr_dropout_f32(g, g, dropout_keep, drop_mul, (size_t)B * t.N0 * D, s));
      TR_TRY(tr_dropout_bf16(gb, gb, dropout_keep, drop_mul, (size_t)B * t.N0 * D, s));
    }
    if (u_embed) TR_TRY(tr_embed_bwd(g, F(grads->pos_embed), F(grads->cls_token), acc, B, t.N0, D, s));
    if (u_patch)
      TR_TRY(tr_linear_bwd_params(gb, D, t.P, tape<uint16_t>(tp.cols), kcols, F(grads->patch_w), F(grads->patch_b), acc, wsf, wsn, B * t.P, D, kcols, s));
    // the input gradient: the patch projection's data gradient, folded back into the image (every element of dx written once)
    if (dx != nullptr) TR_TRY(tr_patch_embed_dgrad_hw(gb, D, U(wt->patch_w), dx, B, cfg->in_chans, trplan::img_h(cfg), trplan::img_w(cfg), cfg->patch, D, s));
    return TR_OK;
  }
};

// every norm of the block loop leaves its d gamma / d beta partials in bp.lnpart; one reduce launch after the loop (tr_ln_defer_flush)
struct LnDeferScope {
  LnDeferScope(float* r, size_t n, hipStream_t st) { tr_ln_defer_begin(r, n, st); }
  ~LnDeferScope() { tr_ln_defer_end(); }
};

}  // namespace

extern "C" size_t tr_vit_backward_workspace_bytes(const tr_vit_config* cfg, int B) {
  trplan::TokenPlan t;
  BwdPlan p;
  if (!cfg || B <= 0 || !trplan::trainable_family(cfg->family) || !trplan::make_token_plan(cfg, &t) || !make_bwd_plan(cfg, B, t, &p)) return 0;
  return p.total;
}

// wt: the weight MATRICES transposed (bf16): blocks[i].qkv_w = qkv.weight^T [D,3D], proj_w = proj.weight^T [D,D], fc1_w = fc1.weight^T
//     [D,Hd], fc2_w = fc2.weight^T [Hd,D]; patch_w = the patch weight^T [in_chans*patch*patch, D], read by tr_vit_backward_dx only; other fields
//     unused.  w: the forward's weights (head_w and the LayerNorm gammas are read).
// grads: same layout as tr_vit_weights, every pointer an fp32 gradient buffer of the parameter's shape (matrices included).
// Frozen parameters: a UNIT of grads may be NULL (both pointers, never one) and its gradient work is left out -- {head_w, head_b},
//     {norm_g, norm_b}, per block {ln1_g, ln1_b} {qkv_w, qkv_b} {proj_w, proj_b} {ln2_g, ln2_b} {fc1_w, fc1_b} {fc2_w, fc2_b},
//     {pos_embed, cls_token}, {patch_w, patch_b}: a NULL Linear unit is left out of the block's weight-gradient group, a NULL norm runs the
//     LayerNorm backward without its parameter partials, a NULL head unit runs the classifier's data gradient only.  The walk STOPS at
//     the lowest block that owns a gradient: when the embedding unit, the patch unit and every unit and stage pointer of the blocks
//     below block i are NULL, block i's own parameter gradients are the last launches (its qkv data gradient and a frozen norm1 do not
//     run), and a range call below that block launches nothing; with no block unit at all only the classifier (+ a present final norm)
//     runs.  Stage modules (grads->stage[i]) are not skipped one by one: a stage the walk reaches needs all its pointers (TR_ERR_NULL
//     otherwise); they may be NULL only below the stop block.
// accumulate != 0: gradients are added to the buffers (engine.py:41 grad accumulation), else overwritten.
// [blk_hi .. blk_lo] (blk_hi >= blk_lo): the blocks this call walks, in reverse.  blk_hi == depth-1 also runs the classifier and
// the final norm first; blk_lo == 0 also runs the embedding gradients last.
// Headless (num_classes == 0): dlogits is the gradient of the CLS features fp32 [B,D]; it enters the final norm's backward rounded to bf16
// (what the classifier's data gradient hands it), and w->head_* / grads->head_* are not read.
// Average-pooled head (global_pool == 1): the tape's xfinal holds the pooled patch tokens, the final norm's backward writes its row gradient
// to a [B,D] buffer and tr_token_pool_bwd spreads it over the patch rows of g (zeros in the CLS rows; weights: the sizes / the mask the
// last merging / sampling block left on the tape) instead of the memset + CLS-row write; everything below is the same walk.
// DyViT only: dpred (nullable) fp32 [stages, B, P]: gradient wrt each stage's out_pred_prob (the ratio loss, losses.py:113-118), stages in
// block order; dfeat (nullable) fp32 [B, N0, D]: gradient wrt the final-norm token features (distillation, losses.py:134-156; row 0 = 0).  The gradient of the residual stream stays in the
// workspace between calls, so a backward pass is the calls (depth-1 .. a), (a-1 .. b), ..., (c .. 0) in this order.
// dx (nullable): the gradient with respect to the input image, fp32 [B, in_chans, img, img] (tr_vit_backward_dx).  With dx the walk goes all the
// way down whatever is frozen (stop = -1: a fully frozen model is valid, the stage pointers are required everywhere), and the call with
// blk_lo == 0 ends with one more launch: tr_patch_embed_dgrad on gb (after pos_drop's mask) and wt->patch_w = the patch weight transposed.
static int vit_backward(const tr_vit_config* cfg, const tr_vit_weights* w, const tr_vit_weights* wt, const tr_vit_weights* grads,
                        const float* dlogits, const float* dpred, const float* dfeat, const float* drop_scale, const void* tape_,
                        size_t tape_bytes, void* workspace, size_t workspace_bytes, int accumulate, int blk_hi, int blk_lo, int B,
                        tr_stream_t s, const uint8_t* dropout_keep, float drop_rate, float* dx, const void* dtokens = nullptr,
                        int dtokens_is_bf16 = 0, const float* stream = nullptr, const tr_vit_level_grads* lev = nullptr) {
  TR_REQUIRE(cfg && w && wt && grads && dlogits && tape_ && workspace, TR_ERR_NULL, "tr_vit_backward: null pointer");
  if (lev != nullptr && lev->present == 0) lev = nullptr;
  if (lev != nullptr) {
    const int n_levels = __builtin_popcount(lev->blocks);
    TR_REQUIRE(cfg->family != TR_FAMILY_DYVIT, TR_ERR_CONFIG, "tr_vit_backward_levels: DyViT's feature gradient is dfeat");
    TR_REQUIRE(lev->blocks != 0 && (cfg->depth >= 32 || (lev->blocks >> cfg->depth) == 0) && (lev->norm == 0 || lev->norm == 1) &&
                   (n_levels >= 32 || (lev->present >> n_levels) == 0),
               TR_ERR_CONFIG, "tr_vit_backward_levels: blocks 0x%x / norm %d / present 0x%x do not name levels of a depth-%d model", lev->blocks,
               lev->norm, lev->present, cfg->depth);
    TR_REQUIRE(lev->dtokens && (lev->norm == 0 || lev->stream), TR_ERR_NULL, "tr_vit_backward_levels: dtokens (norm == 1: or stream) is NULL");
    TR_REQUIRE(lev->level_stride % 8 == 0 && tr_aligned16(lev->dtokens) && tr_aligned16(lev->stream), TR_ERR_ALIGN,
               "tr_vit_backward_levels: dtokens / stream must be 16-byte aligned, level_stride a multiple of 8");
    TR_REQUIRE(dtokens == nullptr || ((lev->blocks >> (cfg->depth - 1)) & 1u) == 0 ||
                   ((lev->present >> (n_levels - 1)) & 1u) == 0,
               TR_ERR_CONFIG, "tr_vit_backward_levels: the level of block %d has a gradient AND dtokens is given", cfg->depth - 1);
  }
  if (dtokens != nullptr) {
    TR_REQUIRE(stream != nullptr, TR_ERR_NULL, "tr_vit_backward_dense: dtokens needs the forward's stream_out");
    TR_REQUIRE(cfg->family != TR_FAMILY_DYVIT, TR_ERR_CONFIG, "tr_vit_backward_dense: DyViT's feature gradient is dfeat");
    TR_REQUIRE(tr_aligned16(dtokens) && tr_aligned16(stream), TR_ERR_ALIGN, "tr_vit_backward_dense: dtokens / stream must be 16-byte aligned");
  }
  TR_REQUIRE((dropout_keep == nullptr) == (drop_rate == 0.f) && drop_rate >= 0.f && drop_rate < 1.f, TR_ERR_CONFIG,
             "tr_vit_backward: dropout needs the forward's keep mask AND its drop_rate (got mask %p, rate %g)", (const void*)dropout_keep, (double)drop_rate);
  TR_REQUIRE(cfg->precision == TR_PREC_BF16 && trplan::trainable_family(cfg->family), TR_ERR_CONFIG,
             "tr_vit_backward: family %d / precision %d has no training path", cfg->family, cfg->precision);
  trplan::TokenPlan t;
  trplan::TapePlan tp;
  BwdPlan bp;
  TR_REQUIRE(trplan::make_token_plan(cfg, &t) && trplan::make_tape_plan(cfg, B, t, &tp) && make_bwd_plan(cfg, B, t, &bp), TR_ERR_CONFIG,
             "tr_vit_backward: invalid config");
  TR_REQUIRE(lev == nullptr || lev->level_stride >= (size_t)B * t.N0 * cfg->embed_dim, TR_ERR_SHAPE,
             "tr_vit_backward_levels: level_stride %zu is below B * N0 * D = %zu", lev ? lev->level_stride : 0, (size_t)B * t.N0 * cfg->embed_dim);
  TR_REQUIRE(tape_bytes >= tp.total && workspace_bytes >= bp.total, TR_ERR_SHAPE, "tr_vit_backward: tape (%zu < %zu) or workspace (%zu < %zu) too small",
             tape_bytes, tp.total, workspace_bytes, bp.total);
  TR_REQUIRE(tr_aligned16(tape_) && tr_aligned16(workspace), TR_ERR_ALIGN, "tr_vit_backward: tape / workspace must be 16-byte aligned");
  TR_REQUIRE(blk_lo >= 0 && blk_hi >= blk_lo && blk_hi < cfg->depth, TR_ERR_CONFIG, "tr_vit_backward: bad block range [%d .. %d]", blk_hi, blk_lo);
  Frozen fr;
  TR_TRY(frozen_plan(cfg, w, wt, grads, t, dx, &fr));
  const int stop = fr.stop;
  if (blk_hi < stop && blk_hi < cfg->depth - 1) return TR_OK;        // the whole range lies below the stop block

  Bwd b(cfg, w, wt, grads, t, tp, bp, fr, B, s, tape_, workspace, accumulate, drop_scale, dropout_keep, drop_rate, dlogits, dpred, dfeat, dx);
  b.dtokens = dtokens;
  b.dtokens_bf16 = dtokens_is_bf16 != 0;
  b.dstream = stream;
  if (lev != nullptr) {
    b.lev_norm = lev->norm != 0;
    for (int i = 0, l = 0; i < cfg->depth; ++i) {
      if (((lev->blocks >> i) & 1u) == 0) continue;
      const int at = l++;
      if (((lev->present >> at) & 1u) == 0) continue;
      const void* dt = b.lev_norm ? static_cast<const void*>(static_cast<const uint16_t*>(lev->dtokens) + at * lev->level_stride)
                                  : static_cast<const void*>(static_cast<const float*>(lev->dtokens) + at * lev->level_stride);
      if (i < cfg->depth - 1) {
        b.lev_dtok[i] = dt;
        b.lev_stream[i] = b.lev_norm ? lev->stream + at * lev->level_stride : nullptr;
      } else if (b.lev_norm) {     // the last block's level IS the dense map of tr_vit_backward_dense
        b.dtokens = dt;
        b.dtokens_bf16 = true;
        b.dstream = lev->stream + at * lev->level_stride;
      } else {
        b.lev_last = static_cast<const float*>(dt);
      }
    }
  }
  b.rewind_to(blk_hi);
  if (blk_hi == cfg->depth - 1) {
    bool go = false;
    TR_TRY(b.head_and_final_norm(&go));
    if (!go) return stop >= cfg->depth ? b.levels_below_stop() : TR_OK;
  }
  LnDeferScope ln_scope(b.ws<float>(bp.lnpart), bp.lnpart_floats, b.st);
  for (int i = blk_hi; i >= blk_lo && i >= stop; --i) {
    // Block, reversed: x += mlp(norm2(x)); [in-block reducer]; x += attn(norm1(x)); [stage reducer]
    bool done = false;
    b.begin_block(i);
    TR_TRY(b.level_inject(i));
    TR_TRY(b.mlp_bwd(i));
    TR_TRY(b.norm2_bwd(i));
    TR_TRY(b.proj_bwd(i));
    TR_TRY(b.attention_bwd(i));
    TR_TRY(b.block_wgrads(i, &done));
    if (done) break;
    TR_TRY(b.qkv_norm1_bwd(i, &done));
    if (done) break;
    TR_TRY(b.stage_bwd(i));
  }
  TR_TRY(tr_ln_defer_flush());
  if (stop >= blk_lo && stop <= blk_hi) TR_TRY(b.levels_below_stop());      // (the walk ended at the stop block in this call)
  if (blk_lo > 0 || stop >= 0) return TR_OK;
  return b.embed_bwd();
}

extern "C" int tr_vit_backward(const tr_vit_config* cfg, const tr_vit_weights* w, const tr_vit_weights* wt, const tr_vit_weights* grads,
                               const float* dlogits, const float* dpred, const float* dfeat, const float* drop_scale, const void* tape_,
                               size_t tape_bytes, void* workspace, size_t workspace_bytes, int accumulate, int blk_hi, int blk_lo, int B,
                               tr_stream_t s, const uint8_t* dropout_keep, float drop_rate) {
  return vit_backward(cfg, w, wt, grads, dlogits, dpred, dfeat, drop_scale, tape_, tape_bytes, workspace, workspace_bytes, accumulate, blk_hi, blk_lo, B,
                      s, dropout_keep, drop_rate, nullptr);
}

extern "C" int tr_vit_backward_dx(const tr_vit_config* cfg, const tr_vit_weights* w, const tr_vit_weights* wt, const tr_vit_weights* grads,
                                  const float* dlogits, const float* dpred, const float* dfeat, const float* drop_scale, const void* tape_,
                                  size_t tape_bytes, void* workspace, size_t workspace_bytes, int accumulate, int blk_hi, int blk_lo, int B,
                                  tr_stream_t s, const uint8_t* dropout_keep, float drop_rate, float* dx) {
  return vit_backward(cfg, w, wt, grads, dlogits, dpred, dfeat, drop_scale, tape_, tape_bytes, workspace, workspace_bytes, accumulate, blk_hi, blk_lo, B,
                      s, dropout_keep, drop_rate, dx);
}

extern "C" int tr_vit_backward_dense(const tr_vit_config* cfg, const tr_vit_weights* w, const tr_vit_weights* wt, const tr_vit_weights* grads,
                                     const float* dlogits, const float* dpred, const float* dfeat, const float* drop_scale, const void* tape_,
                                     size_t tape_bytes, void* workspace, size_t workspace_bytes, int accumulate, int blk_hi, int blk_lo, int B,
                                     tr_stream_t s, const uint8_t* dropout_keep, float drop_rate, float* dx, const void* dtokens,
                                     int dtokens_is_bf16, const float* stream) {
  return vit_backward(cfg, w, wt, grads, dlogits, dpred, dfeat, drop_scale, tape_, tape_bytes, workspace, workspace_bytes, accumulate, blk_hi, blk_lo, B,
                      s, dropout_keep, drop_rate, dx, dtokens, dtokens_is_bf16, stream);
}

extern "C" int tr_vit_backward_levels(const tr_vit_config* cfg, const tr_vit_weights* w, const tr_vit_weights* wt, const tr_vit_weights* grads,
                                      const float* dlogits, const float* dpred, const float* dfeat, const float* drop_scale, const void* tape_,
                                      size_t tape_bytes, void* workspace, size_t workspace_bytes, int accumulate, int blk_hi, int blk_lo, int B,
                                      tr_stream_t s, const uint8_t* dropout_keep, float drop_rate, float* dx, const void* dtokens,
                                      int dtokens_is_bf16, const float* stream, const tr_vit_level_grads* lev) {
  return vit_backward(cfg, w, wt, grads, dlogits, dpred, dfeat, drop_scale, tape_, tape_bytes, workspace, workspace_bytes, accumulate, blk_hi, blk_lo, B,
                      s, dropout_keep, drop_rate, dx, dtokens, dtokens_is_bf16, stream, lev);
}
