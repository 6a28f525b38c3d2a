/*
 * tokenreduction_hip.h -- C ABI of the MI355X (gfx950) ViT-with-token-reduction hot path.
 *
 * The reference (JoakimHaurum/TokenReduction) is pure PyTorch and has NO native boundary
 * (SURVEY.md section 2a); its hot path is model.forward() of models/{deit_viz,topk,evit}.py.
 * This header is the native boundary this build introduces under the reference's Python
 * plugin API.  Each entry point names the reference lines it replaces.
 *
 * Conventions (every entry point):
 *   - all data pointers are DEVICE pointers owned by the caller (e.g. the PyTorch allocator);
 *     outputs and workspace are pre-allocated by the caller; nothing is allocated or freed here;
 *   - work is enqueued on the caller's stream (`tr_stream_t` = hipStream_t); no call synchronises,
 *     so every call is hipGraph-capturable; no global mutable state (re-entrant per stream);
 *   - bf16 tensors are passed as uint16_t* (raw bits); row-major, innermost dimension contiguous;
 *   - return value: 0 = ok, <0 = error (TR_ERR_*); tr_last_error() gives a thread-local message;
 *   - head_dim is 64 for every DeiT size (models_act.py:1087,1120,1153) and is required.
 */
#ifndef TOKENREDUCTION_HIP_H
#define TOKENREDUCTION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* tr_stream_t; /* hipStream_t */

#define TR_OK 0
#define TR_ERR_SHAPE (-1)     /* unsupported / inconsistent shape */
#define TR_ERR_ALIGN (-2)     /* pointer or leading dimension not 16-byte aligned */
#define TR_ERR_NULL (-3)      /* required pointer is NULL */
#define TR_ERR_LAUNCH (-4)    /* hipLaunch failed (message has hipGetErrorString) */
#define TR_ERR_CONFIG (-5)    /* invalid tr_vit_config */

/* GEMM epilogues: out = epilogue(A[M,K] * W[N,K]^T + bias[N]) */
#define TR_EPI_BF16 0       /* out bf16 [M,N]                            (qkv Linear, topk.py:44)          */
#define TR_EPI_GELU_BF16 1  /* out bf16 [M,N] = gelu_erf(.)              (timm Mlp fc1+act)                */
#define TR_EPI_RESID_F32 2  /* out fp32 [M,N] += (.)  (in-place residual: topk.py:87 / :95)                */
#define TR_EPI_F32 3        /* out fp32 [M,N]                            (head, topk.py:203)               */
#define TR_EPI_PATCH_F32 4  /* out fp32 token rows: row m=(b,p) -> out[(b*(P+1)+1+p), :] = (.) + pos[1+p,:]
                               (PatchEmbed + pos_embed, topk.py:181-186); aux = pos_embed, aux_i = P        */

int tr_version(void);
const char* tr_last_error(void);

/* Launch profiler: between tr_profile_begin(stream) and tr_profile_end, every launch this thread enqueues through the entry points
 * below drops a HIP event on `stream`; tr_profile_end waits for the stream and returns, per launch group ("mark"), a label
 * (48 chars), the milliseconds since the previous mark (kernel + its dependent-launch boundary), and the group's algorithmic
 * FLOPs / bytes where the entry point states them (0 otherwise).  Returns the number of marks (only `max` are written).
 * Not capturable in a hipGraph.  This is how bench.py times the executor kernel by kernel. */
int tr_profile_begin(tr_stream_t s);
int tr_profile_end(int max, char* labels, float* ms, double* flops, double* bytes);

/* a1 (PatchEmbed, call site topk.py:181): unfold 16x16 patches.  img fp32 [B,C,H,W] ->
 * cols bf16 [B*(H/p)*(W/p), C*p*p], column order (c, iy, ix) = Conv2d weight.view(D,-1) order. */
int tr_im2col_bf16(const float* img, uint16_t* cols, int B, int C, int H, int W, int patch, tr_stream_t s);
int tr_im2col_f32(const float* img, float* cols, int B, int C, int H, int W, int patch, tr_stream_t s);   /* fp32 validation path */

/* a2 (topk.py:183-186): x[b*N + 0, :] = cls_token + pos_embed[0] for every image (fp32). */
int tr_cls_pos_rows(const float* cls_token, const float* pos_embed, float* x, int B, int N, int D, tr_stream_t s);

/* a1 + a2 in one launch (the eval forward's patch embedding; timm PatchEmbed + topk.py:181-186): x fp32 [B, P+1, D] with
 * x[b,0,:] = cls_token + pos_embed[0], x[b,1+p,:] = W . patch(b,p) + bias + pos_embed[1+p]; W bf16 [D, C*16*16] (Conv2d weight.view(D,-1)),
 * img fp32 [B,C,HW,HW].  The unfold happens on the way into the LDS (the bf16 column matrix of tr_im2col_bf16 is never written), one
 * workgroup per image and 384 output columns.  Same arithmetic as tr_im2col_bf16 + tr_gemm_bf16(TR_EPI_PATCH_F32) + tr_cls_pos_rows.
 * tr_patch_embed_supported: patch 16, HW %% 16 == 0, D %% 384 == 0 (other shapes: the three-launch path). */
int tr_patch_embed_supported(int C, int HW, int patch, int D);
int tr_patch_embed_bf16(const float* img, const uint16_t* W, const float* bias, const float* cls_token, const float* pos_embed, float* x,
                        int B, int C, int HW, int patch, int D, tr_stream_t s);
/* The same launch on a rectangular image, img fp32 [B,C,H,W]: P = (H/16) (W/16) patches in row-major order, patch p = (p / (W/16), p % (W/16)).
 * The HW entries above are these with H = W = HW (one kernel, the same bits).  tr_patch_embed_hw_supported: patch 16, H and W positive
 * multiples of 16, D a positive multiple of 384, C * H * W < 2^30 (the kernel's 32-bit source offsets). */
int tr_patch_embed_hw_supported(int C, int H, int W, int patch, int D);
int tr_patch_embed_hw_bf16(const float* img, const uint16_t* W_, const float* bias, const float* cls_token, const float* pos_embed, float* x,
                           int B, int C, int H, int W, int patch, int D, tr_stream_t s);

/* PatchEmbed's data gradient (the gradient of the stride-16 Conv2d with respect to the image): for patch p = (py, px) of image b
 *   dx[b, c, 16 py + iy, 16 px + ix] = sum_k dY[(b, p), k] * W[k, (c, iy, ix)]
 * dY bf16 token rows at row stride ldy (elements): row (b, p) is dY + (b (P+1) + 1 + p) ldy -- the yskip = P convention of tr_wgrad_bf16,
 * the CLS row of every image is never read; Wt bf16 [C*16*16, D] = the patch weight TRANSPOSED; dx fp32 [B, C, HW, HW].  fp32
 * accumulation on the bf16 MFMA path in one fixed order; every element of dx is written exactly once (patches do not overlap): no memset,
 * no atomics, no accumulate flag.  tr_patch_embed_dgrad_supported: patch 16, HW % 16 == 0 (up to 4096), C = 1 or 3, D = 128, 192, 384 or 768;
 * anything else is TR_ERR_SHAPE. */
int tr_patch_embed_dgrad_supported(int C, int HW, int patch, int D);
int tr_patch_embed_dgrad(const uint16_t* dY, long ldy, const uint16_t* Wt, float* dx, int B, int C, int HW, int patch, int D, tr_stream_t s);
/* The same launch on a rectangular image: dx fp32 [B, C, H, W], P = (H/16) (W/16) row-major patches; H and W multiples of 16 up to 4096 each.
 * tr_patch_embed_dgrad is this with H = W = HW. */
int tr_patch_embed_dgrad_hw_supported(int C, int H, int W, int patch, int D);
int tr_patch_embed_dgrad_hw(const uint16_t* dY, long ldy, const uint16_t* Wt, float* dx, int B, int C, int H, int W, int patch, int D,
                            tr_stream_t s);

/* Raw uint8 pixels: img uint8 [B,C,H,W] (layout TR_LAYOUT_NCHW) or [B,H,W,C] (TR_LAYOUT_NHWC), 16-byte aligned; lut fp32 [C][256] is the
 * normalized value of every pixel value, lut[c][v] = (v / 255 - mean[c]) / std[c] computed by the host (torchvision's ToTensor + Normalize
 * order).  The kernels only gather from it: their output is bitwise what the fp32 entry points give for the normalized image.
 * tr_im2col_u8_*: as tr_im2col_bf16 / _f32.  tr_patch_embed_u8_bf16: as tr_patch_embed_bf16 (same shapes; NHWC with C = 1 or 3). */
#define TR_LAYOUT_NCHW 0
#define TR_LAYOUT_NHWC 1
int tr_im2col_u8_bf16(const uint8_t* img, const float* lut, int layout, uint16_t* cols, int B, int C, int H, int W, int patch, tr_stream_t s);
int tr_im2col_u8_f32(const uint8_t* img, const float* lut, int layout, float* cols, int B, int C, int H, int W, int patch, tr_stream_t s);
int tr_patch_embed_u8_bf16(const uint8_t* img, const float* lut, int layout, const uint16_t* W, const float* bias, const float* cls_token,
                           const float* pos_embed, float* x, int B, int C, int HW, int patch, int D, tr_stream_t s);
/* tr_patch_embed_u8_bf16 on a rectangular image (shapes: tr_patch_embed_hw_supported; NHWC with C = 1 or 3) */
int tr_patch_embed_u8_hw_bf16(const uint8_t* img, const float* lut, int layout, const uint16_t* W_, const float* bias, const float* cls_token,
                              const float* pos_embed, float* x, int B, int C, int H, int W, int patch, int D, tr_stream_t s);

/* Train-time augmentation of a uint8 batch on the device: RandomErasing (datasets.py:93-95, per image, before mixing) and timm's Mixup
 * (mixup / cutmix, engine.py:47-48), applied to the normalized values while the image is unfolded.  The batch B is even and image b's
 * partner is j = B - 1 - b (timm's x.flip(0)).  One record per image, a DEVICE array of B records, 16-byte aligned:
 *   src(i,c,y,x) = noise[noise_off_i + (c*eh_i + (y - ey_i))*ew_i + (x - ex_i)]  if erased_i and (y,x) inside [ey_i, ey_i+eh_i) x [ex_i, ex_i+ew_i)
 *                = lut[c][img[i,c,y,x]]                                          otherwise
 *   kind 0: out = src(b)    kind 1: out = rn(rn(src(b)*lam) + rn(src(j)*oml))  (fp32; two roundings and an add, never an fma; lam and oml
 *   are independent numbers)    kind 2: out = src(j) inside [yl,yh) x [xl,xh), src(b) outside.
 * noise: one packed fp32 device buffer of noise_len floats; an erased image owns a [C, eh, ew] block at noise_off (NULL allowed when
 * noise_len == 0).  Boxes are clamped to the image and a noise index outside [0, noise_len) reads as 0.0f: a wrong table gives wrong
 * pixels, never a read outside the buffers.  A table of all-zero records gives the bits of tr_im2col_u8_bf16.
 * tr_im2col_u8_aug_bf16: the columns of tr_im2col_u8_bf16 for the augmented image.  tr_pixels_augment_f32: the augmented image itself,
 * fp32 [B,C,H,W] (NCHW whatever the input layout) -- what the float pipeline would hold.  Both refuse the shapes tr_im2col_u8_* refuses
 * and an odd B (TR_ERR_SHAPE). */
typedef struct tr_augment_rec {
  int32_t kind;                 /* 0 none, 1 blend (mixup), 2 paste (cutmix) */
  float lam, oml;               /* kind 1: the two fp32 factors */
  int32_t yl, yh, xl, xh;       /* kind 2: the box pasted from the partner */
  int32_t erased;               /* non-zero: this image has an erase box */
  int32_t ey, eh, ex, ew;       /* erase box: top, height, left, width */
  int64_t noise_off;            /* first float of this image's [C, eh, ew] block in `noise` */
  int32_t reserved_[2];         /* pads the record to 64 bytes (one cache line per image) */
} tr_augment_rec;
int tr_im2col_u8_aug_bf16(const uint8_t* img, const float* lut, int layout, const tr_augment_rec* aug, const float* noise, long noise_len,
                          uint16_t* cols, int B, int C, int H, int W, int patch, tr_stream_t s);
int tr_pixels_augment_f32(const uint8_t* img, const float* lut, int layout, const tr_augment_rec* aug, const float* noise, long noise_len,
                          float* out, int B, int C, int H, int W, int patch, tr_stream_t s);

/* a3/a4 Linear layers (nn.Linear: y = x W^T + b, W is [N,K] row-major like the state dict).
 * A bf16 [M,K], W bf16 [N,K], bias fp32 [N]; K % 64 == 0, N % 4 == 0.  `out` dtype/meaning per epilogue;
 * aux/aux_i only for TR_EPI_PATCH_F32. */
int tr_gemm_bf16(const uint16_t* A, const uint16_t* W, const float* bias, void* out, const float* aux, int aux_i,
                 int M, int N, int K, int epilogue, tr_stream_t s);

/* a4, eval forward: the whole timm Mlp of a block (models/topk.py:78 construction, :95 `x = x + self.mlp(self.norm2(x))`; the residual
 * add stays in the next LayerNorm) in ONE launch: out bf16 [M,D] = fc2(gelu_erf(fc1(xn))) with the [M,Hd] hidden activation never
 * leaving the CU (csrc/tr_mlp_fused.hip).  Bit-identical to tr_gemm_bf16(TR_EPI_GELU_BF16) followed by tr_gemm_bf16(TR_EPI_BF16).
 * `packed`: the two weight matrices in fragment-major order and fc2's bias as an accumulator image, tr_mlp_pack_bytes(D,Hd) bytes,
 * written by tr_mlp_pack_bf16 from the bf16 [Hd,D] / [D,Hd] matrices and the fp32 [D] bias (repack whenever they change).  tr_mlp_fused_supported: D == 384, Hd %% 32 == 0 (other widths: the pair). */
int tr_mlp_fused_supported(int D, int Hd);
/* Which Mlp the eval executor runs where tr_block_weights.mlp_pk is given: 1 = the fused launch wherever the shape is supported, 0 = never,
 * -1 (default) = for more blocks of 128 rows than the device has compute units (stream-K schedule) and where a single round of blocks fills
 * at least three quarters of them (one workgroup per CU: hipDeviceAttributeMultiprocessorCount of the current device, 256 on MI355X; the
 * two Mlp forms are bit-identical, so this is a speed choice only).  Process-wide; returns the previous mode. */
int tr_set_mlp_fused(int mode);
size_t tr_mlp_pack_bytes(int D, int Hd);
int tr_mlp_pack_bf16(const uint16_t* fc1_w, const uint16_t* fc2_w, const float* fc2_b, void* packed, int D, int Hd, tr_stream_t s);
/* scratch (nullable; tr_mlp_fused_scratch_bytes(D,Hd) bytes for the CURRENT device, 16-byte aligned): with it a launch of more blocks of
 * 128 rows than the device has compute units deals its steps evenly over the workgroups (stream-K: a block that straddles two workgroups
 * hands its fp32 accumulator over, exactly); without it whole blocks round-robin.  Same bits either way.
 * A scratch belongs to ONE launch at a time: it holds that launch's accumulator slots and hand-over counters (zeroed by a memset node in
 * front of the kernel), so two launches that may overlap -- other streams, other threads -- need a scratch each.
 * A consumer workgroup polls for its predecessor's accumulator (bounded: seconds; tr_set_mlp_poll_max(iterations), negative = the default
 * again, 0 = every hand-over counts as abandoned (tests), returns the previous bound); a poll
 * that runs out does not stop the process: the launch finishes on whatever the slot held and leaves an error record in the scratch, which
 * tr_mlp_fused_status (waits for the stream, reads and clears the record) turns into TR_ERR_LAUNCH. */
size_t tr_mlp_fused_scratch_bytes(int D, int Hd);
int tr_set_mlp_poll_max(int iterations);
int tr_mlp_fused_status(void* scratch, size_t scratch_bytes, int D, int Hd, tr_stream_t s);
int tr_mlp_fused_bf16(const uint16_t* xn, const void* packed, const float* fc1_b, uint16_t* out, void* scratch, size_t scratch_bytes, int M, int D,
                      int Hd, tr_stream_t s);
/* topk.py:95's `self.mlp(self.norm2(x))` in ONE launch: out bf16 [M,D] = fc2(gelu(fc1(LayerNorm(x + delta; g, b, eps)))) with x the fp32
 * residual stream [M,D] and delta the pending bf16 residual of the attention branch [M,D] (neither is written): the kernel's fc1 waves
 * normalise their rows in registers on the way in.  Bit-identical to tr_layernorm2_bf16(x, .., NULL, .., delta, .., NULL, .., g, b, xn, ..)
 * followed by tr_mlp_fused_bf16(xn, ..): the LayerNorm launch (8 B per element through HBM) and the bf16 rows between the two are gone.
 * tr_set_mlp_ln: where the eval executor takes this form in place of a lazy norm2 followed by the fused Mlp -- 1 (default): where that launch
 * is one round of whole blocks (measured faster there, slower under the stream-K schedule, which normalises a block once per workgroup that
 * touches it) and everywhere in a forward marked `concurrent` (those launches run whole blocks), 2: wherever the fused Mlp runs, 0: never;
 * returns the previous setting. */
int tr_set_mlp_ln(int mode);
int tr_mlp_fused_ln_bf16(const float* x, const uint16_t* delta, const float* g, const float* b, float eps, const void* packed,
                         const float* fc1_b, uint16_t* out, void* scratch, size_t scratch_bytes, int M, int D, int Hd, tr_stream_t s);
/* a3/a4, eval forward: the START of a block in one launch -- topk.py:86-87 `self.attn(self.norm1(x))` with :44 `self.qkv(x)`, and the previous
 * block's pending residual adds folded in:  v = (x [+ d1]) [+ d2]  (fp32 stream row [M,D] + pending bf16 residuals [M,D], in that order:
 * d1 = attention branch, d2 = Mlp branch of the previous block; d2 needs d1),  x_out[M,D] = v  (out of place, x_out != x; NULL exactly when
 * d1 is NULL: nothing pending, nothing rewritten),  out bf16 [M,N] = LayerNorm(v; g, b, eps) . W^T + bias.
 * Bit-identical to tr_layernorm_bf16 / tr_layernorm2_bf16 followed by tr_gemm_bf16(TR_EPI_BF16) -- and without the LayerNorm launch's
 * 12-14 bytes per element at the memory roof: four of the kernel's twelve waves normalise the next 128-row block while the other eight
 * multiply the current one (csrc/tr_lnlin.hip).  tr_lnlin_supported: D == 384, N %% 64 == 0, 128 <= N <= 4096.
 * `packed`: W [N,D] (nn.Linear layout, bf16) in fragment-major order, tr_lnlin_pack_bytes(D,N) bytes, written by tr_lnlin_pack_bf16 (repack
 * whenever W changes).  `scratch`: tr_lnlin_scratch_bytes(D,N) bytes for the current device (two 96-KiB row slots per compute unit), one
 * launch at a time like tr_mlp_fused_bf16's. */
int tr_lnlin_supported(int D, int N);
size_t tr_lnlin_pack_bytes(int D, int N);
size_t tr_lnlin_scratch_bytes(int D, int N);
int tr_lnlin_pack_bf16(const uint16_t* W, void* packed, int D, int N, tr_stream_t s);
int tr_lnlin_bf16(const float* x, const uint16_t* d1, const uint16_t* d2, float* x_out, const float* g, const float* b, float eps,
                  const void* packed, const float* bias, uint16_t* out, void* scratch, size_t scratch_bytes, int M, int D, int N, tr_stream_t s);
/* The tail of a block and the head of the next in ONE launch (topk.py:95 `x = x + self.mlp(self.norm2(x))`, then the next block's :87
 * `self.norm1(x)`):  x[M,D] (fp32 stream, already holding the attention branch's residual) += fc2(gelu(fc1(xn))) + fc2_b, IN PLACE, and
 * xn_next[M,D] (bf16, != xn) = LayerNorm(x; next_g, next_b, eps).  The kernel's fc2 wave owns whole rows in registers: its accumulator
 * starts at the stream row, so the fc2 output is never rounded to bf16 on its way into the stream, and the row's mean / variance are taken in
 * registers (two passes, tr_layernorm's formulas).  Replaces fc1, fc2 and the residual-add + LayerNorm launch behind them; not bit-identical
 * to that sequence (one rounding fewer), same tolerance class.  packed / scratch as for tr_mlp_fused_bf16 (fc2_b is passed again: the bias
 * image inside `packed` is not used here). */
/* Whether the eval executor runs that form where it runs the fused Mlp and the next block starts with a plain norm1 (1) or keeps
 * tr_mlp_fused_bf16 + the LayerNorm launch (0 = default: measured, the one-launch form is 4 % slower on the headline forward -- its
 * epilogue stalls the workgroup; profiles/r05_mlp_lab.md).  Process-wide; returns the previous setting. */
int tr_set_mlp_resid_ln(int on);
int tr_mlp_fused_resid_ln_bf16(const uint16_t* xn, const void* packed, const float* fc1_b, const float* fc2_b, float* x, const float* next_g,
                               const float* next_b, float eps, uint16_t* xn_next, void* scratch, size_t scratch_bytes, int M, int D, int Hd,
                               tr_stream_t s);

/* a4 nn.LayerNorm(D, eps) rows of the fp32 residual stream -> bf16 (topk.py:86 norm1, :95 norm2, :201 norm), with the
 * PENDING residual add folded in: if delta != NULL (bf16 rows at stride ldd: the output of attn.proj / mlp.fc2),
 * x[row] += delta[row] is written back first (`x = x + drop_path(...)`, topk.py:87 / :95), then y[row] = LN(x[row]).
 * x fp32 rows at stride ldx (floats); y bf16 [M,D].  D % 4 == 0, D <= 1024. */
int tr_layernorm_bf16(float* x, long ldx, const uint16_t* delta, long ldd, const float* gamma, const float* beta, uint16_t* y,
                      int M, int D, float eps, tr_stream_t s);
int tr_layernorm_f32(float* x, long ldx, const float* delta, long ldd, const float* gamma, const float* beta, float* y, int M,
                     int D, float eps, tr_stream_t s);                                                  /* fp32 validation path */
/* Same, out of place: x_out[row] = x[row] + delta[row] (rows at stride ldxo; x_out == x is the in-place form above).  The training
 * forward uses it so that the input of every norm survives for the backward pass. */
int tr_layernorm_bf16_to(const float* x, long ldx, float* x_out, long ldxo, const uint16_t* delta, long ldd, const float* gamma,
                         const float* beta, uint16_t* y, int M, int D, float eps, tr_stream_t s);
/* y = LayerNorm((x + delta) + delta2) with TWO pending residuals (delta2 nullable), the sum written to x_out -- or, x_out == NULL, not
 * written at all.  The eval executor's "lazy norm2": a norm2 that no reduction follows normalises x + d_attn without storing it, the
 * next norm1 adds d_attn and d_mlp in the reference's order (topk.py:87, :95) and writes the stream once: bit-identical to two
 * tr_layernorm_bf16 calls, 22 instead of 24 bytes per element and block. */
int tr_layernorm2_bf16(const float* x, long ldx, float* x_out, long ldxo, const uint16_t* delta, long ldd, const uint16_t* delta2, long ldd2,
                       const float* gamma, const float* beta, uint16_t* y, int M, int D, float eps, tr_stream_t s);
/* The three bf16-path norms above with the output stored as fp32 rows y [M,D]: y = LayerNorm((x + delta) + delta2), delta and delta2
 * nullable (delta2 needs delta), the sum written to x_out (x_out == x: in place; NULL: not written).  Same statistics, same summation order,
 * same arithmetic -- only the final store differs, so bf16(y) is bit for bit what tr_layernorm_bf16 / _bf16_to / tr_layernorm2_bf16 store.
 * The final norm of a headless model (tr_vit_config.num_classes == 0), whose fp32 CLS features are the output. */
int tr_layernorm_bf16_f32(const float* x, long ldx, float* x_out, long ldxo, const uint16_t* delta, long ldd, const uint16_t* delta2,
                          long ldd2, const float* gamma, const float* beta, float* y, int M, int D, float eps, tr_stream_t s);

/* out[i] = x[i] + delta[i] for n elements (delta nullable; bf16, fp32 when delta_is_f32): the residual stream after a block as
 * the reference's viz_data["Features"] records it (topk.py:197) -- x itself absorbs the pending mlp output only in the next norm. */
int tr_residual_snapshot(const float* x, const void* delta, int delta_is_f32, float* out, size_t n, tr_stream_t s);
/* Output taps (tr_vit_forward_taps; csrc/tr_taps.hip).  The pending operands are bf16 rows, fp32 when delta_is_f32; d1 and d2 nullable (d2
 * needs d1); D % 4 == 0, D <= 1024; every stride in elements, % 4 == 0 and >= D.  The sums are fp32 additions in this order: the value
 * tr_residual_snapshot stores behind a norm that wrote x + d1 back, bit for bit.
 * tr_cls_tap: out[b] = (x[b] + d1[b]) + d2[b] for B rows of D.  x rows at stride ldx (the CLS rows of a [B,N,D] stream: N * D), d1 / d2 at ld1 /
 * ld2 (N * D, or D for the compact buffers of the CLS tail), out rows at ldo (n_blocks * D: the taps of one image are contiguous).
 * tr_final_tokens_f32: y[row] = LayerNorm((x[row] + d1[row]) + d2[row]) over contiguous fp32 rows [M,D] with tr_layernorm_f32's arithmetic:
 * tr_residual_snapshot followed by tr_layernorm_f32 in one launch and one pass; x is not written. */
int tr_cls_tap(const float* x, long ldx, const void* d1, long ld1, const void* d2, long ld2, int delta_is_f32, float* out, long ldo, int B,
               int D, tr_stream_t s);
int tr_final_tokens_f32(const float* x, const void* d1, const void* d2, int delta_is_f32, const float* gamma, const float* beta, float* y,
                        int M, int D, float eps, tr_stream_t s);
/* tr_level_tap_norm: both taps of contiguous rows [M, D] in ONE launch, for the level taps of a training forward: sum[row] = (x + d1) + d2 --
 * the bits of tr_cls_tap at row stride D -- and y[row] = its fp32 LayerNorm -- the bits of tr_final_tokens_f32; x and the pending operands are
 * read once, two rows are stored.  Operands, alignment and refusals are tr_final_tokens_f32's; sum and y are 16-byte aligned. */
int tr_level_tap_norm(const float* x, const void* d1, const void* d2, int delta_is_f32, const float* gamma, const float* beta, float* sum,
                      float* y, int M, int D, float eps, tr_stream_t s);
/* tr_stream_grad_add: g[i] += d[i] in fp32 and gb[i] = bf16(g[i]) (round to nearest even; gb nullable), n % 4 == 0: the gradient of a level's
 * rows taken as they stand joins the stream gradient of tr_vit_backward_levels. */
int tr_stream_grad_add(const float* d, float* g, uint16_t* gb, size_t n, tr_stream_t s);
/* Average-pooled head (tr_vit_config.global_pool == 1; csrc/tr_pool.hip): timm's global_pool='avg' with fc_norm -- the pool runs BEFORE the
 * final norm.  Pending operands as above (bf16, fp32 when delta_is_f32; d1 / d2 nullable, d2 needs d1), contiguous [B,N,D] like x.
 * tr_token_pool: out[b] = sum_n w[b,n] * v[b,n] / sum_n w[b,n] over the patch rows n = 1 .. N-1 (row 0, the CLS token, is left out), v = (x +
 *   d1) + d2 in fp32, out fp32 [B,D].  weight fp32 [B,N] (entry 0 not read): ToMe token sizes / the ATS padding mask; NULL = all ones (the
 *   same bits as a buffer of ones).  A row of weight 0 adds nothing whatever it holds; an image whose weights sum to 0 pools to exact zeros.
 *   One pass, every input byte read once (16-byte loads); fp32 accumulation in an order that depends on N alone -- not on B, not on the
 *   launch geometry: no atomics, two launches give the same bits, an image pools to the same bits in any batch.
 *   N >= 2, D %% 64 == 0, B <= 65535: anything else is TR_ERR_SHAPE before any launch.
 * tr_token_pool_bwd: g[b,0,:] = 0, g[b,n,:] = gpool[b,:] * (w[b,n] * (1 / sum_n w[b,n])) (0 where the sum is 0); g fp32 [B,N,D], EVERY element
 *   written exactly once (no memset in front of it).  No gradient with respect to the weights.  Same shape rules. */
int tr_token_pool(const float* x, const void* d1, const void* d2, int delta_is_f32, const float* weight, float* out, int B, int N, int D,
                  tr_stream_t s);
int tr_token_pool_bwd(const float* gpool, const float* weight, float* g, int B, int N, int D, tr_stream_t s);
/* dst fp32 [B,N] = src fp32 [N] in every row (the Heuristic family's per-block key mask, heuristic.py:247-258). */
int tr_broadcast_rows(const float* src, float* dst, int B, int N, tr_stream_t s);

/* a3 (topk.py:44-51 == deit_viz.py:43-51): softmax(q k^T / sqrt(64)) v for every (image, head).
 * qkv bf16 [B*N, 3*H*64] (columns [q|k|v], head-major), out bf16 [B*N, H*64].
 * cls_rows (nullable) fp32 [B,H,N]: the CLS query's softmax row (attn[:, :, 0, :], topk.py:59) --
 * the only part of the N x N matrix the reduction reads, so the matrix is never materialised.
 * size (nullable) fp32 [B,N]: ToMe's proportional attention (Attention_ToMe.forward tome.py:48-49): log(size[key]) is added
 * to every query's logit for that key; a 1/0 key mask works the same way (ATS, ats.py:117-120: log 0 = -inf -> weight 0).
 * colsum_part (nullable) fp32 [B,H,4,N]: column sums of the softmax matrix, one partial per wave of the workgroup -- summed
 * over (H, 4) they are K-Medoids' token weights sum_h sum_q attn[b,h,q,:] (kmedoids.py:240); partials keep the summation
 * order fixed (no float atomics).
 * Any N: up to 224 tokens a query's whole score row sits in registers (attention16_kernel); beyond (384 x 384 inputs: 577) keys pass
 * through the LDS in chunks of 128 with an online softmax; column sums together with a key bias need N <= 608. */
int tr_attention_bf16(const uint16_t* qkv, uint16_t* out, float* cls_rows, const float* size, float* colsum_part, int B, int N,
                      int H, tr_stream_t s);
/* The same attention where only the CLS query's output is read (the last block of the eval forward): out bf16 [B, H*64] (compact) = row 0
 * of every image of what tr_attention_bf16 writes into [B*N, H*64], bit for bit (same kernels, same instruction sequence for that query
 * block).  K and V of all N rows are read; only the first query block of every (image, head) is computed.  size as above. */
int tr_attention_cls_bf16(const uint16_t* qkv, uint16_t* out, const float* size, int B, int N, int H, tr_stream_t s);
/* CLS tail of the eval executor (bf16): in the LAST block, where nothing reduces from the attention onward and no `Features` are asked for,
 * tr_vit_forward runs tr_attention_cls_bf16 and then proj, norm2, fc1, fc2 on the B CLS rows only -- the only rows the final norm and the
 * head read (topk.py:201-203).  1 (default) / 0: the full-width block; the logits are bit-identical.  TR_PREC_FP32 / TR_PREC_BF16X3
 * always run the full-width block.  Process-wide, read when the launches are enqueued; returns the previous setting. */
int tr_set_cls_tail(int on);
/* fp32 validation path (N <= 640; K/V of a head in LDS up to N = 256, read from L2 beyond): same contract in the reference's
 * arithmetic (expf softmax, fp32 everywhere). */
int tr_attention_f32(const float* qkv, float* out, float* cls_rows, const float* size, float* colsum_part, int B, int N, int H,
                     tr_stream_t s);
/* TR_PREC_BF16X3: same contract, q k^T and P v as split-bf16 products on the matrix cores (fp32 softmax, whole row in registers);
 * N <= 224 on MFMA, longer sequences are forwarded to tr_attention_f32. */
int tr_attention_split(const float* qkv, float* out, float* cls_rows, const float* size, float* colsum_part, int B, int N, int H,
                       tr_stream_t s);
/* a11 (forward only): Policy_Attention.forward dyvit.py:53-67 with softmax_with_policy :39-51 -- the attention of DyViT's
 * TRAINING forward, where pruned tokens stay in the sequence and are masked by policy fp32 [B,N] of 1/0:
 *   attn = (exp(s - max_k s) * pol + eps/N) / (sum_k exp(s - max_k s) * pol + eps),  pol[q][k] = policy[k], 1 for k == q,
 * eps = 1e-6.  bf16: any N (beyond 224 tokens -- 384 x 384 inputs -- an online-softmax kernel over 128-key chunks); fp32: N <= 256.
 * Used by the DyViT training executor (backward: tr_attention_policy_bwd_bf16 / tr_attention_policy_bwd_long_bf16). */
int tr_attention_policy_bf16(const uint16_t* qkv, uint16_t* out, const float* policy, int B, int N, int H, tr_stream_t s);
int tr_attention_policy_f32(const float* qkv, float* out, const float* policy, int B, int N, int H, tr_stream_t s);

/* a6 (topk.py:55-65 == evit.py:77-87) + a8 (evit.py:25-46 complement_idx):
 * scores[b,j] = mean_h cls_rows[b,h,1+j] (j < P = N-1); idx[b,:K] = indices of the K largest scores in
 * DESCENDING score order (ties: lowest index first -- torch.topk's CPU tie order is unspecified);
 * compl (nullable) [B,P-K] = indices not selected, ascending.  scores (nullable) fp32 [B,P]. int32 indices. */
int tr_cls_topk(const float* cls_rows, int32_t* idx, int32_t* compl_idx, float* scores, int B, int H, int N, int K,
                tr_stream_t s);

/* a7 (topk.py:89-93) [+ a9 evit.py:111-123] fused with norm2 (topk.py:95):
 * with x := x + delta when delta != NULL (bf16 [B,N,D], the pending attn.proj output -- topk.py:87 precedes the gather):
 * x_out[b,0]=x[b,0]; x_out[b,1+r]=x[b,1+idx[b,r]] (r<K); if compl_idx: x_out[b,K+1]=sum_j x[b,1+compl[b,j]]*scores[b,compl[b,j]].
 * Also y = LayerNorm(x_out) in bf16.  x fp32 [B,N,D] -> x_out fp32 [B,N_out,D], y bf16 [B,N_out,D],
 * N_out = K+1 (+1 with fuse).  idx == NULL means identity (N_out = N, x_out may be NULL -> only y written). */
int tr_gather_layernorm_bf16(const float* x, const uint16_t* delta, const int32_t* idx, const int32_t* compl_idx, const float* scores,
                             const float* gamma, const float* beta, float* x_out, uint16_t* y, int B, int N, int K,
                             int D, float eps, tr_stream_t s);
int tr_gather_layernorm_f32(const float* x, const float* delta, const int32_t* idx, const int32_t* compl_idx, const float* scores,
                            const float* gamma, const float* beta, float* x_out, float* y, int B, int N, int K, int D,
                            float eps, tr_stream_t s);                                                  /* fp32 validation path */

/* The training forward's Linear + GELU (timm Mlp fc1, the DyViT / SiT predictor layers): pre bf16 [M,N] = A W^T + bias stays for the
 * backward, h bf16 [M,N] = gelu(pre) on the ROUNDED pre-activation -- bitwise tr_gemm_bf16(TR_EPI_BF16) followed by tr_gelu_bf16, in
 * one launch.  K % 64 == 0, N % 8 == 0. */
int tr_gemm_gelu_keep_bf16(const uint16_t* A, const uint16_t* W, const float* bias, uint16_t* pre, uint16_t* h, int M, int N, int K,
                           tr_stream_t s);

/* Backward of Linear -> GELU's second half (timm Mlp fc2 -> act, the DyViT / SiT predictor layers): out bf16 [M,N] =
 * bf16(A W^T) * gelu'(pre) (a data gradient: no bias), pre bf16 [M,N] the pre-activation tr_gemm_gelu_keep_bf16 kept (engine.py:76 loss.backward() through
 * timm Mlp) -- bitwise tr_gemm_bf16(TR_EPI_BF16) followed by tr_gelu_bwd_bf16, in one launch.  K % 64 == 0, N % 8 == 0. */
int tr_gemm_dgelu_bf16(const uint16_t* A, const uint16_t* W, const uint16_t* pre, uint16_t* out, int M, int N, int K, tr_stream_t s);

/* fp32 validation path of the Linear layers: A fp32 [M,K], W fp32 [N,K], out fp32; K % 16 == 0.
 * epilogue: TR_EPI_F32 (bias), TR_EPI_GELU_BF16 (bias + exact-erf GELU, fp32 out), TR_EPI_PATCH_F32. */
int tr_gemm_f32(const float* A, const float* W, const float* bias, float* out, const float* aux, int aux_i, int M, int N, int K,
                int epilogue, tr_stream_t s);
/* TR_PREC_BF16X3: the same Linear (same operands, epilogues and fp32 output) on the matrix cores -- every fp32 operand is split
 * into hi = bf16(v), lo = bf16(v - hi) and a product is taken as hi*hi + hi*lo + lo*hi in the fp32 MFMA accumulator (~2^-17
 * relative per product).  K % 32 == 0 and N % 4 == 0 run on MFMA; other shapes are forwarded to tr_gemm_f32. */
int tr_gemm_split(const float* A, const float* W, const float* bias, float* out, const float* aux, int aux_i, int M, int N, int K,
                  int epilogue, tr_stream_t s);

/* ---- reducers that run before a block (csrc/tr_prune.hip) ------------------------------------------------------------
 * tr_pool_broadcast: PredictorLG.forward dyvit.py:115-118 with policy == 1 (eval): h [B,N,C] (bf16, or fp32 when is_f32), in
 *   place: channels C/2..C-1 of every row become mean over the image's PATCH rows (1..N-1) of that channel + eps.
 * tr_dyvit_score: out_conv.4 + LogSoftmax + [:,:,0] (dyvit.py:108-109,231): h [M,C] -> scores fp32 [M]; w fp32 [2,C], bias [2].
 * tr_sit_merge: TokenSlimmingModule.forward sit.py:37-39: logits fp32 [B,N,ldl] (row 0 of an image = CLS, ignored; first K
 *   columns used), softmax(logits*scale) over the patch-token axis, x_out[b,1+k,:] = sum_p w[b,p,k] x[b,1+p,:]; x_out[b,0] =
 *   x[b,0]; x, x_out fp32 [B,N,D] / [B,K+1,D].  soft (nullable): fp32 [B,K,N-1].
 * tr_rownorm: F.normalize(x, dim=-1) (sinkhorn.py:70): x fp32 [M,D] -> xh fp32 [M,D] and the same rows as a GEMM operand
 *   (bf16, fp32 when lp_is_f32).
 * tr_sinkhorn: log_optimal_transport (sinkhorn.py:41-56) per image on scores fp32 [B,N,ldl] (row 0 = CLS ignored; columns
 *   0..K-1 = token . centre): wt (may alias scores) gets the transport plan token-major [B,N,ldl], soft (nullable) the same
 *   cluster-major [B,K,N-1] (Soft_Assignment_Maps).  K*(N-1) floats stay in LDS when they fit, else in the scores buffer.
 * tr_weighted_merge: x_out[b,1+k,:] = sum_p wt[b,1+p,k] * src[b,1+p,:]; x_out[b,0] = x[b,0]   (sinkhorn.py:83 with
 *   src = unit-norm tokens). */
int tr_pool_broadcast(void* h, int is_f32, int B, int N, int C, float eps, tr_stream_t s);
int tr_rownorm(const float* x, float* xh, void* xh_lp, int lp_is_f32, int M, int D, tr_stream_t s);
int tr_sinkhorn(const float* scores, int ldl, float eps, int iters, float* wt, float* soft, int B, int N, int K, tr_stream_t s);
int tr_weighted_merge(const float* wt, int ldl, const float* x, const float* src, float* x_out, int B, int N, int K, int D,
                      tr_stream_t s);
int tr_dyvit_score(const void* h, int is_f32, const float* w, const float* bias, float* scores, int M, int C, tr_stream_t s);
int tr_sit_merge(const float* logits, int ldl, float scale, const float* x, float* x_out, float* soft, int B, int N, int K,
                 int D, tr_stream_t s);
/* tr_sit_merge with the summed rows taken from `src` fp32 [B,N,D] instead of x (PatchMerger sums the LayerNorm-ed tokens,
 * patchmerger.py:36-39); the CLS row still comes from x. */
int tr_softassign_merge(const float* logits, int ldl, float scale, const float* x, const float* src, float* x_out, float* soft,
                        int B, int N, int K, int D, tr_stream_t s);
/* Same result on MFMA (what the bf16 executor uses; K <= 192): apply_softmax != 0 first turns `logits` IN PLACE into the
 * token-axis softmax of logits*scale (and writes `soft` if given), then x_out[b,1+k,:] = sum_p logits[b,1+p,k] * src[b,1+p,:]
 * with both operands split into bf16 hi + lo (relative error ~2^-16).  apply_softmax == 0: `logits` already holds the
 * weights (Sinkhorn's transport plan). */
int tr_softassign_merge_fast(float* logits, int ldl, float scale, int apply_softmax, const float* x, const float* src, float* x_out,
                             float* soft, int B, int N, int K, int D, tr_stream_t s);
/* ---- DPC-KNN (csrc/tr_cluster.hip) --------------------------------------------------------------------------------------
 * tr_dpcknn_cluster: cluster_dpc_knn dpcknn.py:44-100 (token_mask=None) on the patch rows of x fp32 [B,N,D] (row 0 = CLS,
 *   ignored): centers int32 [B,K] = topk(score, K) in descending-score order (index_down), idx_cluster int32 [B,N-1],
 *   scores fp32 [B,N-1] (distance-to-denser-token * density).  noise (nullable) fp32 [B,N-1]: the uniform [0,1) draws the
 *   reference adds * 1e-6 to the densities (dpcknn.py:71-72); NULL = none.  k = nearest neighbours (args.k_neighbors).
 *   ws: tr_dpcknn_workspace_floats(B,N) floats of scratch.  fast_dist != 0 (also tr_kmedoids): the Gram product of the
 *   distance matrix runs on MFMA with hi/lo-split bf16 operands (relative error ~2^-16) instead of fp32 VALU -- what the bf16
 *   executor uses; 0 = the reference's fp32 arithmetic (validation executor).  For tr_dpcknn_cluster: 1 = the ONE-LAUNCH kernel
 *   below wherever it applies (else the staged launches), 2 = always the staged launches (sqnorm, distances to ws, density,
 *   parent distance, top-K, assignment) -- kept for P > 208 and as the comparison of the tests.
 * tr_dpcknn_cluster_fused (csrc/tr_cluster_fused.hip): the same clustering in one launch, one workgroup per image, the distance
 *   matrix held in LDS as its upper triangle (26 <= N-1 <= 208, D % 32 == 0, D <= 1024, k <= 5: tr_dpcknn_fused_supported);
 *   no workspace.  Identical to the staged launches except that element (i,j) below the diagonal is read from (j,i), which the
 *   staged matrix matches only up to the last bit.
 * tr_cluster_merge_layernorm: merge_tokens dpcknn.py:103-132 with token_weight = exp(x . score_w + score_b) (CTM, :155-157;
 *   score_w NULL = equal weights), then LayerNorm(gamma, beta, eps) of the merged tokens: x_out fp32 [B,K+1,D] (row 0 = CLS
 *   copied), y = LN(x_out) bf16 (fp32 when y_is_f32).  w_ws: [B,N-1] floats of scratch (token weights).
 * tr_kmedoids: k_medoids_fit kmedoids.py:40-85 with token weights (the equal_weight branch draws from the numpy global RNG and
 *   is not built): colsum_part fp32 [B,H,4,N] from the PREVIOUS block's attention -> w = its sum over (H,4) on the patch
 *   columns; initial medoids = topk(w, K); `iters` rounds of {assign to the nearest medoid; medoid k = the member with the
 *   smallest w_i * sum_j dist_ij, index 0 if the cluster is empty (kmedoids.py:74-79)}; final assignment.
 *   centers int32 [B,K] (cluster_idx), assign int32 [B,N-1].  ws: tr_dpcknn_workspace_floats(B,N) floats. */
size_t tr_dpcknn_workspace_floats(int B, int N);
int tr_kmedoids(const float* x, const float* colsum_part, float* ws, int32_t* centers, int32_t* assign, int B, int N, int D, int H,
                int K, int iters, int fast_dist, tr_stream_t s);
/* k_medoids_fit with token_weight = None (args.equal_weight, kmedoids.py:43-58): the first medoid is init_idx for every image -- the
 * reference draws it with np.random.choice on the host, so it is an input --, the others by the farthest-point rule of :47-56,
 * then the same iterations with unit weights. */
int tr_kmedoids_equal(const float* x, int init_idx, float* ws, int32_t* centers, int32_t* assign, int B, int N, int D, int K, int iters,
                      int fast_dist, tr_stream_t s);
int tr_dpcknn_cluster(const float* x, const float* noise, float* ws, int32_t* centers, int32_t* idx_cluster, float* scores,
                      int B, int N, int D, int K, int k, int fast_dist, tr_stream_t s);
int tr_dpcknn_fused_supported(int N, int D, int k);
int tr_dpcknn_cluster_fused(const float* x, const float* noise, int32_t* centers, int32_t* idx_cluster, float* scores, int B, int N,
                            int D, int K, int k, tr_stream_t s);
int tr_cluster_merge_layernorm(const float* x, const float* score_w, const float* score_b, float* w_ws,
                               const int32_t* idx_cluster, const float* gamma, const float* beta, float* x_out, void* y,
                               int y_is_f32, int B, int N, int K, int D, float eps, tr_stream_t s);

/* ---- ATS (csrc/tr_ats.hip) ----------------------------------------------------------------------------------------------
 * tr_ats_sample: AdaptiveTokenSampling.forward ats.py:52-84.  cls_rows fp32 [B,H,N] (softmax row of the CLS query),
 *   qkv [B*N, 3*H*64] (bf16, or fp32 when qkv_is_f32; only V is read), mask (nullable = all valid) fp32 [B,N] of 1/0,
 *   steps fp32 [n_steps] = the module's sample_steps (ats.py:48).  ids int32 [B,K]: id 0 (CLS) first, then the sorted unique
 *   sampled token ids (1-based positions), then 0 padding up to the static bound K; new_mask fp32 [B,K] of 1/0
 *   (ids != 0, CLS 1).  cdf_out (nullable) fp32 [B,N-1]: the cdf the samples were taken on.
 * tr_ats_gather: x_out[b,t] = x[b, ids[b,t]] (fp32 [B,K,D], ats.py:157) and ao_out[b,t] = ao[b, ids[b,t]] (the rows of
 *   attn @ v the sampled queries keep, ats.py:86,129); ao bf16 (fp32 when ao_is_f32). */
int tr_ats_sample(const float* cls_rows, const void* qkv, int qkv_is_f32, const float* mask, const float* steps, int n_steps,
                  int32_t* ids, float* new_mask, float* cdf_out, int B, int N, int H, int K, tr_stream_t s);
int tr_ats_gather(const float* x, const void* ao, int ao_is_f32, const int32_t* ids, float* x_out, void* ao_out, int B, int N,
                  int K, int D, tr_stream_t s);
/* The reference's dynamic width (ats.py:77-78: pad_sequence pads the unique ids to the BATCH maximum, so the token count after a sampling
 * block is 1 + max unique ids, not the static bound K).  tr_ats_width: *width (device int32) = max over the images of their valid ids
 * (row sums of new_mask [B,K]); tr_ats_narrow: the first Kw columns of ids / new_mask as contiguous [B,Kw] arrays, the form tr_ats_gather
 * and the next block's key mask take.  Used by tr_vit_forward when tr_vit_config.ats_dynamic is set. */
int tr_ats_width(const float* new_mask, int32_t* width, int B, int K, tr_stream_t s);
int tr_ats_narrow(const int32_t* ids, const float* new_mask, int32_t* ids_out, float* mask_out, int B, int K, int Kw, tr_stream_t s);

/* a13 bipartite_soft_matching (tome.py:230-277, class_token=True) on metric = k.mean(1) (tome.py:58), read straight from the
 * K third of qkv ([B*N, 3*H*64]; bf16, or fp32 when qkv_is_f32).  Tokens at even positions form set A (CLS = A[0], never
 * merged), odd positions set B.  Outputs (int32): src_idx [B,r] = the r A-tokens with the largest best-match score, in
 * descending order; dst_idx [B,r] = the B-token each is merged into; unm_idx [B, ceil(N/2)-r] = the other A-tokens, ascending.
 * 3 <= N <= 600, 1 <= r <= (N-1)/2 (tome.py:253). */
int tr_tome_match(const void* qkv, int qkv_is_f32, int32_t* unm_idx, int32_t* src_idx, int32_t* dst_idx, int B, int N, int H,
                  int r, tr_stream_t s);

/* a14 merge_wavg (tome.py:309-323) over the merge closure (tome.py:279-289), with the pending residual (delta: bf16, or fp32
 * when f32_path) added first and norm2 (tome.py:101) applied after: x_out [B,N-r,D] = merge((x+delta)*size)/merge(size) in the
 * order [unmerged A-tokens | all B-tokens]; size_out [B,N-r]; y = LayerNorm(x_out) (bf16, or fp32 when f32_path).
 * size_in == NULL means all ones (first merge, tome.py:318-319). */
int tr_tome_merge_layernorm(const float* x, const void* delta, int f32_path, const float* size_in, const int32_t* unm_idx,
                            const int32_t* src_idx, const int32_t* dst_idx, const float* gamma, const float* beta, float* x_out,
                            float* size_out, void* y, int B, int N, int r, int D, float eps, tr_stream_t s);

/* ---- backward kernels (csrc/tr_backward.hip, csrc/tr_attention_bwd.hip) -----------------------------------------------------
 * The reference's training step is `loss.backward()` through the eager forward (engine.py:50-76, mp_scaler.py:10-11); these are
 * the hand-written gradients of the ops above.  Reductions over tokens are two-stage with a fixed order (bitwise reproducible).
 * `accumulate` != 0: the gradient is ADDED to the destination (gradient accumulation, engine.py:41), else it is overwritten.
 * tr_wgrad_bf16: nn.Linear weight gradient dW[N,K] (+)= dY[M,N]^T X[M,K]; dY, X bf16 at row strides ldy, ldx (elements); yskip > 0:
 *   dY row m is row m + m/yskip + 1 of its tensor (the patch rows of a [B, P+1, D] tensor, yskip = P: PatchEmbed's weight gradient).
 *   ws: tr_wgrad_workspace_floats(M,N,K) floats (partials of the token splits).  N, K, ldy, ldx multiples of 8.
 * tr_colsum_bf16: nn.Linear bias gradient db[N] (+)= sum_m dY[m,n]; ws: tr_colsum_workspace_floats(M,N) floats.
 * tr_gelu_bf16 / tr_gelu_bwd_bf16: h = gelu(pre) with the SAME fit as TR_EPI_GELU_BF16 (the training forward stores fc1's
 *   pre-activation, then applies this); dh := dh * gelu'(pre) in place (exact erf form).
 * tr_layernorm_bwd: dy bf16 [M,D] (gradient wrt the LayerNorm output), x fp32 rows (the saved LayerNorm INPUT, row stride ldx),
 *   g_in (nullable) fp32 rows: gradient already flowing in the residual stream at these rows; g_out = g_in + dLN -> fp32 rows
 *   (stride ldgo) and gb_out (nullable) bf16 [rows, D].  d_gamma, d_beta fp32 [D].  idx != NULL: the rows are the gathered rows
 *   [B, n_in] of a Top-K block (n_in = K+1, or K+2 with EViT's fused token); row r of image b is written to row
 *   (r == 0 ? 0 : 1 + idx[b,r-1]) of [B, n_out, D] and the fused row to g_fused fp32 [B, D] (the caller zero-fills g_out/gb_out).
 *   ws: tr_layernorm_bwd_workspace_floats(M, D) floats.
 *   Frozen norm: d_gamma == d_beta == NULL (both, never one: TR_ERR_NULL) computes the data gradient only -- the same bits in g_out /
 *   gb_out / g_fused, no parameter partials, ws (may be NULL) untouched, no reduce launch, nothing added to a deferred reduce; every
 *   form takes it (plain, index scatter with and without g_fused, tr_layernorm_bwd_scatter_add).  Profiler label
 *   "ln_bwd_kernel<no_params>" instead of "ln_bwd_kernel".
 * tr_attention_bwd_bf16: d qkv from d out (see csrc/tr_attention_bwd.hip), N <= 224.
 * tr_head_bwd: dxn bf16 [B,D] = dlogits W; dW (+)= dlogits^T xn; db (+)= colsum(dlogits)   (topk.py:203; W, xn bf16); the weight and
 *   bias gradients run through tr_wgrad_bf16 / tr_colsum_bf16 on dl16, a bf16 copy of dlogits ([B,C] scratch); ws as tr_wgrad_bf16.
 *   Frozen classifier: dW == db == NULL (both) runs the data gradient alone; xn, dl16 and ws are then not read.
 * tr_embed_bwd: d pos_embed [N,D] (+)= sum_b g[b,n,:], d cls_token [D] (+)= sum_b g[b,0,:]   (topk.py:183-186).
 * tr_evit_fuse_bwd: evit.py:117-120: g_out[b,1+c,:] = scores[b,c] g_fused[b] (fp32 + bf16 copy) for the complement tokens c,
 *   dscore[b,1+c] = <x[b,1+c] + delta[b,1+c], g_fused[b]>  (dscore fp32 [B,N], zero-filled by the caller).
 * tr_tome_merge_bwd: merge_wavg (tome.py:309-323): g_out[b,i,:] = size_in[b,i] / size_out[b,o(i)] * g_merged[b,o(i),:];
 *   inv_map int32 [B,N] scratch. */
size_t tr_wgrad_workspace_floats(int M, int N, int K);
int tr_wgrad_bf16(const uint16_t* dY, long ldy, int yskip, const uint16_t* X, long ldx, float* dW, int accumulate, float* ws,
                  size_t ws_floats, int M, int N, int K, tr_stream_t s);
/* Both parameter gradients of an nn.Linear in one pass over dY (the bias sums come out of the weight-gradient kernel's staging
 * registers) and one reduce launch; ws as tr_wgrad_bf16. */
int tr_linear_bwd_params(const uint16_t* dY, long ldy, int yskip, const uint16_t* X, long ldx, float* dW, float* db, int accumulate,
                         float* ws, size_t ws_floats, int M, int N, int K, tr_stream_t s);

/* Parameter gradients of TWO Linear layers at once -- one weight-gradient launch and one reduce launch for both (the backward executor
 * pairs fc2 + fc1 and proj + qkv of a block; engine.py:76).  Each layer as in tr_linear_bwd_params with yskip = 0; results identical to
 * two separate calls up to the (fixed, reproducible) summation order over token ranges. */
/* ... and of up to FOUR (what the backward executor does with fc2, fc1, proj and qkv of a block when nothing rewrites their dY in between):
 * layer i: dW_i [N,K] (+)= dY_i[M, ldy]^T X_i[M, ldx], db_i [N] (+)= column sums of dY_i. */
typedef struct tr_linear_grad {
  const uint16_t* dY; long ldy;
  const uint16_t* X;  long ldx;
  float* dW; float* db;
  int M, N, K;
} tr_linear_grad;
size_t tr_linear_bwd_group_workspace_floats(const tr_linear_grad* layers, int n);      /* only M, N, K of each layer are read */
int tr_linear_bwd_group(const tr_linear_grad* layers, int n, int accumulate, float* ws, size_t ws_floats, tr_stream_t s);
size_t tr_linear_bwd_params2_workspace_floats(int M0, int N0, int K0, int M1, int N1, int K1);
int tr_linear_bwd_params2(const uint16_t* dY0, long ldy0, const uint16_t* X0, long ldx0, float* dW0, float* db0, int M0, int N0, int K0,
                          const uint16_t* dY1, long ldy1, const uint16_t* X1, long ldx1, float* dW1, float* db1, int M1, int N1, int K1,
                          int accumulate, float* ws, size_t ws_floats, tr_stream_t s);
size_t tr_colsum_workspace_floats(int M, int N);
int tr_colsum_bf16(const uint16_t* dY, long ldy, int yskip, float* db, int accumulate, float* ws, size_t ws_floats, int M, int N,
                   tr_stream_t s);
int tr_gelu_bf16(const uint16_t* pre, uint16_t* h, size_t n, tr_stream_t s);
int tr_gelu_bwd_bf16(const uint16_t* pre, uint16_t* dh, size_t n, tr_stream_t s);
size_t tr_layernorm_bwd_workspace_floats(int M, int D);
int tr_layernorm_bwd(const uint16_t* dy, const float* x, long ldx, const float* gamma, const float* g_in, long ldgi, float* g_out,
                     long ldgo, uint16_t* gb_out, const int32_t* idx, int K, int n_in, int n_out, float* g_fused, float* dgamma,
                     float* dbeta, int accumulate, float* ws, size_t ws_floats, int M, int D, float eps, tr_stream_t s);
int tr_layernorm_bwd_scatter_add(const uint16_t* dy, const float* x, const float* gamma, const float* g_in, float* g_out,
                                 const int32_t* idx, int K, int n_out, float* dgamma, float* dbeta, int accumulate, float* ws,
                                 size_t ws_floats, int M, int D, float eps, tr_stream_t s);   /* repeated ids: rows are added (atomics);
                                                                                                 dgamma == dbeta == NULL as above */
int tr_attention_bwd_bf16(const uint16_t* qkv, const uint16_t* dout, const float* size, const float* dcls, uint16_t* dqkv, int B,
                          int N, int H, tr_stream_t s);
/* The same gradient for ANY sequence length (the training executor uses it beyond 224 tokens: 384 x 384 inputs): keys in blocks of 64,
 * three launches per call -- per-query statistics (log-sum-exp and delta = sum_k p dP by online softmax), dQ per query block, dK / dV
 * per key block -- 9 N x N x 64 products per head instead of 5, no float atomics.  ws: tr_attention_bwd_long_workspace_floats floats. */
size_t tr_attention_bwd_long_workspace_floats(int B, int N, int H);
int tr_attention_bwd_long_bf16(const uint16_t* qkv, const uint16_t* dout, const float* size, const float* dcls, uint16_t* dqkv, float* ws,
                               size_t ws_floats, int B, int N, int H, tr_stream_t s);
int tr_head_bwd(const float* dlogits, const uint16_t* W, const uint16_t* xn, uint16_t* dxn, float* dW, float* db, int accumulate,
                uint16_t* dl16, float* ws, size_t ws_floats, int B, int C, int D, tr_stream_t s);
int tr_embed_bwd(const float* g, float* dpos, float* dcls, int accumulate, int B, int N, int D, tr_stream_t s);
int tr_evit_fuse_bwd(const float* x, const uint16_t* delta, const int32_t* compl_idx, const float* scores, const float* g_fused,
                     float* g_out, uint16_t* gb_out, float* dscore, int B, int N, int K, int D, tr_stream_t s);
int tr_tome_merge_bwd(const float* g_merged, const float* size_in, const float* size_out, const int32_t* unm_idx,
                      const int32_t* src_idx, const int32_t* dst_idx, int32_t* inv_map, float* g_out, uint16_t* gb_out, int B, int N,
                      int r, int D, tr_stream_t s);
int tr_f32_to_bf16(const float* src, uint16_t* dst, size_t n, tr_stream_t s);
/* ---- backward of the soft-assignment reducers (csrc/tr_soft_bwd.hip): SiT sit.py:36-40, PatchMerger patchmerger.py:35-39, Sinkhorn
 * sinkhorn.py:41-86.  Forward: out[b,1+k,:] = sum_p wt[b,1+p,k] * src[b,1+p,:] (tr_softassign_merge*), wt token-major fp32 [B,N,ldl], row 0
 * of an image (CLS) unused.  With g = d out fp32 [B,K+1,D]:
 * tr_soft_dweights: dwt[b,1+p,k] = <g[b,1+k,:], src[b,1+p,:]>  (fp32 [B,N,ldl], CLS rows untouched)
 * tr_soft_dsrc:     dsrc[b,1+p,:] = sum_k wt[b,1+p,k] g[b,1+k,:]  (fp32 [B,N,D], CLS rows untouched)
 * tr_token_softmax_bwd: wt = softmax over the tokens of logits*scale: ds[b,1+p,k] = scale * wt (dwt - sum_p' wt dwt) as bf16 at row stride
 *   ldo (CLS rows zero; columns K..ldo-1 untouched: zero them once), the next GEMMs' operand; dscale (nullable, fp32[1]) (+)= d/d scale
 *   (SiT's learnable temperature, sit.py:34) -- needs the raw logits and tr_token_softmax_bwd_workspace_floats(B,K) floats.
 * tr_sinkhorn_bwd: log_optimal_transport backwards: scores = the raw token.centre products, dplan = d of the transport plan (both fp32
 *   [B,N,ldl]); the iterations are recomputed in LDS (K*(N-1) floats must fit: 224x224 inputs); ds bf16 as above.
 * tr_rownorm_bwd: F.normalize backwards: dx = (d xh - xh <xh, d xh>) / |x| with d xh = da (fp32) + db (bf16, nullable).
 * tr_add_into_bf16: y := bf16(a + y). */
int tr_soft_dweights(const float* g, const float* src, float* dwt, int ldl, int B, int N, int K, int D, tr_stream_t s);
int tr_soft_dsrc(const float* g, const float* wt, int ldl, float* dsrc, int B, int N, int K, int D, tr_stream_t s);
size_t tr_token_softmax_bwd_workspace_floats(int B, int K);
int tr_token_softmax_bwd(const float* wt, const float* dwt, const float* logits, int ldl, float scale, uint16_t* ds, int ldo, float* dscale,
                         int accumulate, float* ws, size_t ws_floats, int B, int N, int K, tr_stream_t s);
int tr_sinkhorn_bwd(const float* scores, const float* dplan, int ldl, float eps, int iters, uint16_t* ds, int ldo, int B, int N, int K,
                    tr_stream_t s);
int tr_rownorm_bwd(const float* x, const float* da, const uint16_t* db, float* dx, int M, int D, tr_stream_t s);
int tr_add_into_bf16(const float* a, uint16_t* y, size_t n, tr_stream_t s);

int tr_rowscale_bf16(const uint16_t* src, uint16_t* dst, const float* scale, int B, int rows, int D, tr_stream_t s);   /* dst[b,r,:] = src[b,r,:] * scale[b] */
int tr_reduce_partials_f32(const float* part, int S, size_t count, float* dst, int accumulate, tr_stream_t s);   /* dst (+)= sum_s part[s], in a fixed order that is not sequential in s: four interleaved lanes, see csrc/tr_backward.hip */
/* ---- DyViT training pieces (csrc/tr_dyvit_train.hip, csrc/tr_attention_bwd.hip): see the file headers.  policy / prev / outputs are
 * fp32 [B,N] with entry 0 = the CLS token (always 1); gumbel fp32 [B,N-1,2]. */
int tr_pool_policy(uint16_t* h, const float* policy, int B, int N, int C, float eps, tr_stream_t s);
int tr_pool_policy_bwd(const uint16_t* dcat, const uint16_t* pre0, const uint16_t* cat, const float* policy, uint16_t* dh, float* dpolicy,
                       int B, int N, int C, tr_stream_t s);
int tr_dyvit_decide(const uint16_t* h2, int ldh, const float* w, const float* bias, const float* gumbel, const float* prev,
                    float* policy_out, float* ysoft0, float* sm0, float* hard0, int B, int N, int C, tr_stream_t s);
size_t tr_dyvit_decide_bwd_workspace_floats(int B, int N, int C);
int tr_dyvit_decide_bwd(const float* dkeep, const float* prev, const float* hard0, const float* ysoft0, const float* sm0,
                        const uint16_t* h2, int ldh, const float* w, uint16_t* dh2, float* dprev, float* dw, float* db, int accumulate,
                        float* ws, size_t ws_floats, int B, int N, int C, tr_stream_t s);
int tr_attention_policy_bwd_bf16(const uint16_t* qkv, const uint16_t* dout, const float* policy, uint16_t* dqkv, float* dpol_part, int B,
                                 int N, int H, tr_stream_t s);   /* N <= 224; dpol_part fp32 [B,H,N]: sum the heads with tr_head_sum */
/* The same gradient for any N (the executor uses it beyond 224 tokens: DyViT training at 384 x 384): the key-blocked kernels of
 * tr_attention_bwd_long_bf16 under the keep policy.  ws: tr_attention_bwd_long_workspace_floats(B,N,H) floats. */
int tr_attention_policy_bwd_long_bf16(const uint16_t* qkv, const uint16_t* dout, const float* policy, uint16_t* dqkv, float* dpol_part,
                                      float* ws, size_t ws_floats, int B, int N, int H, tr_stream_t s);
int tr_head_sum(const float* part, float* dst, int B, int H, int N, tr_stream_t s);
int tr_fill_f32(float* p, float v, size_t n, tr_stream_t s);
int tr_add_patch_rows(float* dst, const float* src, int B, int N, tr_stream_t s);
/* DPC-KNN CTM backward (merge_tokens dpcknn.py:103-132 + the score Linear, CTM.forward :155-157): see csrc/tr_backward.hip.
 * ws: at least (B+1)*(D+4) floats; with (8B+1)*(D+4) eight workgroups share an image.  tr_ats_scatter: backward of ATS's row sampling (ats.py:86,157): valid sampled rows t go back to row
 * ids[b,t] of the zero-filled full tensors (g fp32 [B,Ks,D] -> [B,N,D]; d(attn @ v) bf16 likewise). */
int tr_cluster_merge_bwd(const float* g_in, const float* x0, const float* x1, const float* wtok, const int32_t* assign,
                         const float* score_w, float* g_out, uint16_t* gb_out, float* d_sw, float* d_sb, int accumulate, float* ws,
                         size_t ws_floats, int B, int N, int K, int D, tr_stream_t s);
int tr_ats_scatter(const float* g, const uint16_t* dao_s, const int32_t* ids, float* g_full, uint16_t* dao_full, int B, int N, int Ks,
                   int D, tr_stream_t s);

/* ---- whole-model executor: TopKVisionTransformer.forward topk.py:179-212,
 *      EfficientVisionTransformer.forward evit.py:209-244, deit_viz.VisionTransformer.forward :186-212 (eval) ---- */
#define TR_FAMILY_DEIT 0
#define TR_FAMILY_TOPK 1
#define TR_FAMILY_EVIT 2
#define TR_FAMILY_TOME 3   /* keep[blk] = r requested for that block (tome.py:152-155); clamped per call to (N-1)/2 */
#define TR_FAMILY_DYVIT 4  /* eval path of models/dyvit.py: predictor scores -> top-K -> gather BEFORE the block */
#define TR_FAMILY_SIT 5    /* models/sit.py: soft token slimming BEFORE the block */
#define TR_FAMILY_ATS 7    /* models/ats.py: inverse-CDF token sampling inside the attention; keep[blk] = sample_count K (static
                              token bound of the block's output; padded rows are masked keys) */
#define TR_FAMILY_SINKHORN 8 /* models/sinkhorn.py: optimal-transport soft assignment to learned centres BEFORE the block */
#define TR_FAMILY_KMEDOIDS 9 /* models/kmedoids.py: weighted K-Medoids on the patch tokens BEFORE the block, medoids kept */
#define TR_FAMILY_PATCHMERGER 10 /* models/patchmerger.py: K learned queries attend over the normalised tokens BEFORE the block */
#define TR_FAMILY_HEURISTIC 11 /* models/heuristic.py: fixed spatial key/query masks from a block on; no token is removed */
#define TR_FAMILY_DPCKNN 6 /* models/dpcknn.py: DPC-KNN clustering + weighted merge BEFORE the block; keep[blk] = clusters */
#define TR_MAX_DEPTH 32
#define TR_PREC_BF16 0   /* the product path: bf16 MFMA operands, fp32 accumulate / residual / statistics */
#define TR_PREC_FP32 1   /* validation path: the reference's own arithmetic on the GPU (bit-exact indices vs its golden vectors) */
#define TR_PREC_BF16X3 2 /* the fp32 executor with Linears + attention as split-bf16 (hi/lo) products on the matrix cores */

/* Weight MATRICES are bf16 (uint16_t bits) when cfg.precision == TR_PREC_BF16 and fp32 otherwise; vectors are fp32. */
typedef struct {
  const float* ln1_g; const float* ln1_b;
  const void* qkv_w; const float* qkv_b;     /* [3D,D], [3D] */
  const void* proj_w; const float* proj_b;   /* [D,D], [D] */
  const float* ln2_g; const float* ln2_b;
  const void* fc1_w; const float* fc1_b;     /* [Hd,D], [Hd] */
  const void* fc2_w; const float* fc2_b;     /* [D,Hd], [D] */
  const void* mlp_pk;                        /* optional (NULL = none): fc1_w / fc2_w in tr_mlp_pack_bf16's fragment-major order; with it the bf16
                                                EVAL forward may run the block's Mlp as one launch (tr_mlp_fused_bf16: bit-identical to the pair) */
} tr_block_weights;

/* Learned reduction module of one block (families that own one); unused pointers NULL.
 *   DyViT PredictorLG (dyvit.py:96-110): ln = in_conv.0 (eps 1e-5), w0/b0 = in_conv.1 [D,D], w1/b1 = out_conv.0 [D/2,D],
 *     w2/b2 = out_conv.2 [D/4,D/2], w3/b3 = out_conv.4 [2,D/4] (fp32 in both precisions).
 *   SiT TokenSlimmingModule (sit.py:29-34): ln = weight.0 (eps 1e-5), w0/b0 = weight.1 [D/2,D], w1/b1 = weight.3 zero-padded
 *     to n_pad rows ([n_pad, D/2], n_pad = K rounded up to 8), scale = the module's scalar.
 *   PatchMerger (patchmerger.py:32-33): ln = norm (eps 1e-5), w1 = queries zero-padded to n_pad rows [n_pad, D], b1 = zeros,
 *     scale = 1 (embed_dim**-0.5 with scaled_attention).
 *   Sinkhorn (sinkhorn.py:62,73-76): w1 = F.normalize(v) zero-padded to n_pad rows [n_pad, D], b1 = zeros [n_pad].
 *   Heuristic (heuristic.py:247-258): w3 = the block's visibility mask fp32 [N] of 1/0 (CLS 1), n_pad = N; blocks without a
 *     new mask leave w3 NULL and keep the previous one.
 *   ATS (ats.py:48): w3 = sample_steps fp32 [n_pad], n_pad = their count (K-1).
 *   DPC-KNN CTM (dpcknn.py:150-151): w3/b3 = score.weight [1,D] / score.bias [1] (fp32); NULL = args.equal_weight. */
typedef struct {
  const float* ln_g; const float* ln_b;
  const void* w0; const float* b0;
  const void* w1; const float* b1;
  const void* w2; const float* b2;
  const float* w3; const float* b3;
  float scale; int n_pad;
  int h_pad;                   /* DyViT / SiT: width of the D/2 hidden layer as packed (D/2 rounded up to 64 with zero weights, so
                                  the bf16 GEMMs' K %% 64 holds for DeiT-T); 0 = D/2 */
  int reserved_;
} tr_stage_weights;

typedef struct {
  const void* patch_w; const float* patch_b;     /* [D, C*p*p], [D] */
  const float* cls_token; const float* pos_embed;/* [D], [(P+1), D] fp32 */
  const float* norm_g; const float* norm_b;
  const void* head_w; const float* head_b;       /* [classes, D], [classes]; NULL (not read) when num_classes == 0 */
  tr_block_weights blocks[TR_MAX_DEPTH];
  tr_stage_weights stage[TR_MAX_DEPTH];          /* indexed by BLOCK; read only where keep[blk] > 0 (DyViT, SiT) */
} tr_vit_weights;

typedef struct {
  int family;                 /* TR_FAMILY_* */
  short img_size;             /* image height in pixels, a positive multiple of `patch` */
  short img_width;            /* image width in pixels; 0 = square, width = img_size.  Otherwise a positive multiple of `patch`; anything else
                                 is an invalid config.  The grid is gh x gw = (img_size / patch) x (width / patch), P = gh gw patches in row-major
                                 order, patch p = (p / gw, p % gw): every token count, the tape and the workspace follow from P, and images are
                                 [B, C, img_size, width].  (Two 16-bit halves of what was `int img_size`: the struct keeps its 80 x 4 bytes and
                                 every offset, and a caller that wrote the int 224 wrote img_size = 224, img_width = 0.) */
  int patch, in_chans;
  int embed_dim, depth, num_heads, mlp_hidden, num_classes;   /* num_classes == 0: headless (no classifier; the output is the
                                                                  final-normed CLS row, see tr_vit_forward) */
  float ln_eps;
  int keep[TR_MAX_DEPTH];     /* per block, 0 = plain block.  Top-K/EViT/DyViT: K patch tokens kept; ToMe: r tokens merged
                                 away; SiT: K output tokens of the slimming module */
  int precision;              /* TR_PREC_* */
  int knn_k;                  /* DPC-KNN: neighbours of the local density (args.k_neighbors, train.py:221 default 5) */
  int cluster_iters;          /* Sinkhorn / K-Medoids iterations (args.cluster_iters, train.py:232 default 3) */
  float sinkhorn_eps;         /* Sinkhorn temperature (args.sinkhorn_eps, train.py:229 default 1.0) */
  int kmed_init[TR_MAX_DEPTH];/* K-Medoids args.equal_weight: per block, 1 + the first medoid id (the host's np.random.choice draw,
                                 kmedoids.py:45); 0 = the attention-weighted branch */
  int ats_dynamic;            /* ATS, eval forward only: 1 = every sampling block shrinks to the batch maximum of unique ids like the reference
                                 (ats.py:77-78) instead of running the static bound keep[blk] with masked rows.  Same valid tokens and logits (to
                                 the attention kernels' summation order); fewer rows downstream.  tr_vit_forward then reads one int back per
                                 sampling block: it SYNCHRONISES the stream there and cannot be captured in a hipGraph.  0 = static (default). */
  short concurrent;           /* eval forward only, a scheduling hint: 1 = the caller runs other forwards BESIDE this one (other streams, other
                                 workspaces: models.py forward_async), so a launch need not fill the chip on its own -- the other forward's
                                 launches take the compute units it leaves idle.  The executor then runs the fused Mlp wherever it is
                                 supported (also where its blocks fill less than 3/4 of a round) and as whole blocks round-robin (no stream-K
                                 hand-over traffic): measured +2 ... +3 % with two forwards in flight, -2 ... -4 % one at a time.  Same bits
                                 either way.  0 = one forward at a time (default).  (A 16-bit flag since global_pool took the upper half of
                                 what was `int concurrent`: the struct keeps its 80 x 4 bytes and every offset, and a caller that wrote the
                                 int 0 / 1 wrote concurrent = 0 / 1, global_pool = 0.) */
  short global_pool;          /* what the final norm and the classifier see.  0 (default): the CLS row, the reference's head (topk.py:201-203).
                                 1: the average of the patch tokens after the last block, pooled BEFORE the norm (timm's global_pool='avg' with
                                 fc_norm, the MAE fine-tuning head): feat = LayerNorm(sum_n w_n v_n / sum_n w_n), n = 1 .. N_last-1, v = the stream with
                                 its pending residuals; w = ToMe's token sizes after the last merge, the ATS padding mask, 1 for every other
                                 family and before the first merge / sampling stage (tr_token_pool).  The CLS row still runs through every block;
                                 the last block runs at full width (no CLS tail).  Eval in all three precisions, training and backward
                                 (tr_token_pool_bwd; no gradient with respect to w) -- except DyViT in TRAINING mode, which keeps masked tokens
                                 in the stream: TR_ERR_CONFIG.  Any other value: TR_ERR_CONFIG. */
} tr_vit_config;

/* Diagnostics (lab, tools/lab/clock_probe.py): the in-kernel clock probes of a library built with -DTR_DIAG_CLOCK -- {shader cycles, 100-MHz
 * ticks, launches} of workgroup 8 of gemm_bf16_pc / mlp_fused_kernel since the last read (read and reset); all zero in a product build. */
int tr_gemm_clock_probe_read(unsigned long long* out3);
int tr_mlp_clock_probe_read(unsigned long long* out3);

/* Bytes of workspace tr_vit_forward needs for batch B (0 on invalid config). */
size_t tr_vit_workspace_bytes(const tr_vit_config* cfg, int B);
/* Status check of the forwards that ran on `workspace` (the same cfg and B): waits for the stream and reports what only the device can
 * know -- today the fused Mlp's stream-K hand-over (tr_mlp_fused_status on the workspace's scratch).  TR_OK, or TR_ERR_LAUNCH when a
 * forward since the last check produced invalid outputs; the record is cleared.  Not part of the forward itself (it synchronises): call
 * it where the logits are consumed. */
int tr_vit_forward_status(const tr_vit_config* cfg, void* workspace, size_t workspace_bytes, int B, tr_stream_t s);

/* img fp32 [B,C,H,W] (H = cfg->img_size, W = cfg->img_width or, when that is 0, H) -> logits fp32 [B,classes].
 * Headless (num_classes == 0, deit_viz.py:142,182: head = nn.Identity()): `logits` is
 * fp32 [B,D] and receives pre_logits(norm(x)[:, 0]), the final-normed CLS row; no classifier GEMM runs and w->head_w / head_b may be NULL.
 * In bf16 the row is the final norm's output before its bf16 rounding (tr_layernorm_bf16_f32): bf16(features) is the classifier's operand.
 * cfg->global_pool == 1: the norm and the classifier (or, headless, `logits`) read the weighted average of the patch rows after the last block
 * instead of its CLS row (tr_vit_config.global_pool, tr_token_pool); the last block then runs at full width, everything else is unchanged.
 * kept_idx (nullable): device int32 slab of depth*B*(P+1) entries;
 * reduction block blk writes its contiguous [B,K_blk] idx array at offset blk*B*(P+1) (Kept_Tokens, topk.py:196); ToMe
 * writes [unm_idx | src_idx | dst_idx] there ([B,na-r], [B,r], [B,r] back to back).  The slab holds depth*B*(P+1) entries.
 * compl_idx (nullable, EViT): same slab shape, block blk writes [B,P_in-K_blk] at offset blk*B*(P+1)
 * (Fusion_Assign, evit.py:229).  soft_out (nullable, SiT): fp32, the stages' soft assignments [B,K,P_in] back to back in
 * block order (Soft_Assignment_Maps, sit.py:124).  DPC-KNN: kept_idx gets the centres [B,K] (Kept_Tokens), compl_idx the
 * assignment [B,P_in] (Assignment_Maps), K-Medoids likewise (medoid ids, assignment); ATS: kept_idx gets ids [B,K] (CLS id 0 first, 1-based token ids, 0 padding); noise_in (nullable): fp32, the stages' density noise [B,P_in] back to back in block
 * order (dpcknn.py:71-72; NULL = no noise).  features_out (nullable): fp32, the residual stream after EVERY block
 * ([B,N_blk,D] back to back in block order; viz_data["Features"]).  tokens_out (nullable, HOST pointer, int[depth]): token count after each block. */
int tr_vit_forward(const tr_vit_config* cfg, const tr_vit_weights* w, const float* img, float* logits,
                   void* workspace, size_t workspace_bytes, int32_t* kept_idx, int32_t* compl_idx, float* soft_out,
                   const float* noise_in, float* features_out, int* tokens_out, int B, tr_stream_t s);

/* tr_vit_forward / tr_vit_forward_train with the image in another format: input_format TR_INPUT_F32 = fp32 [B,C,H,W] (the calls above),
 * TR_INPUT_U8_NCHW = uint8 [B,C,H,W], TR_INPUT_U8_NHWC = uint8 [B,H,W,C] (NHWC: C = 1 or 3 where the fused patch embedding runs).  For the
 * uint8 formats pixel_lut is the fp32 [C][256] table of tr_patch_embed_u8_bf16 and the patch embedding normalizes on the way in: outputs
 * and the training tape are bitwise those of the fp32 call on the normalized image.  Any other format, or a uint8 format without a LUT,
 * is TR_ERR_CONFIG.  (Separate entry points rather than fields of tr_vit_config / tr_vit_weights: those layouts are part of the ABI.) */
#define TR_INPUT_F32 0
#define TR_INPUT_U8_NCHW 1
#define TR_INPUT_U8_NHWC 2
int tr_vit_forward_pixels(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format, const float* pixel_lut,
                          float* logits, void* workspace, size_t workspace_bytes, int32_t* kept_idx, int32_t* compl_idx, float* soft_out,
                          const float* noise_in, float* features_out, int* tokens_out, int B, tr_stream_t s);

/* Output taps: a caller-chosen subset of the residual stream, written by the eval forward while it runs (fp32, device memory).
 *   cls_blocks        bit i set: the CLS row of the stream after block i -- x plus the residuals still pending there, the value
 *                     features_out holds in row 0 of that block, bit for bit
 *   cls_out           fp32 [B, n, D], n = number of set bits, ascending block order (required when cls_blocks != 0)
 *   final_tokens_out  (nullable) fp32 [B, N_last, D]: the final norm of EVERY row after the last block, in fp32 arithmetic
 *                     (tr_final_tokens_f32) -- norm(x) of the DyViT teacher, dyvit.py:325-334
 * tr_vit_forward_taps / tr_vit_forward_pixels_taps are tr_vit_forward / tr_vit_forward_pixels with that struct.  A CLS tap changes nothing
 * else about the launch sequence: lazy norms and the CLS tail stay (the last block's tap reads the tail's compact buffers).  final_tokens_out
 * needs every row of the last block, so the last block runs full width, as under features_out; nothing else changes.  With no tap asked for
 * (cls_blocks == 0, final_tokens_out == NULL) the launches are those of tr_vit_forward.  A bit at or above depth, cls_blocks without
 * cls_out, or taps together with features_out: TR_ERR_CONFIG.  Eval only. */
typedef struct {
  uint32_t cls_blocks;
  float* cls_out;
  float* final_tokens_out;
} tr_vit_taps;
int tr_vit_forward_taps(const tr_vit_config* cfg, const tr_vit_weights* w, const float* img, float* logits, void* workspace,
                        size_t workspace_bytes, int32_t* kept_idx, int32_t* compl_idx, float* soft_out, const float* noise_in,
                        float* features_out, int* tokens_out, int B, tr_stream_t s, const tr_vit_taps* taps);
int tr_vit_forward_pixels_taps(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format, const float* pixel_lut,
                               float* logits, void* workspace, size_t workspace_bytes, int32_t* kept_idx, int32_t* compl_idx,
                               float* soft_out, const float* noise_in, float* features_out, int* tokens_out, int B, tr_stream_t s,
                               const tr_vit_taps* taps);

/* Level taps: EVERY row of the residual stream after caller-chosen blocks, written by the eval forward while it runs (fp32, device memory) --
 * the tokens of the multi-level dense feature maps below.
 *   blocks        bit i set: the stream after block i -- x plus the residuals still pending there, added in fp32 in the order the next norm
 *                 adds them: (x + attention branch) + mlp branch
 *   norm          0: those rows as they are, the rows features_out holds for that block, bit for bit; 1: the model's final LayerNorm (norm_g,
 *                 norm_b, ln_eps) of those rows in fp32 arithmetic (tr_final_tokens_f32)
 *   tokens_out    fp32: the l-th set block's slab starts at l * B * N0 * D (N0 = patch tokens + 1) and holds [B, N_l, D] contiguous, N_l the
 *                 stream's token count after that block (tokens_out[i] of the forward)
 *   tokens_elems  the length of tokens_out in elements, at least popcount(blocks) * B * N0 * D
 * tr_vit_forward_levels is tr_vit_forward_pixels (any input_format) with that struct and, nullable, a tr_vit_taps.  A tapped block writes its
 * slab with ONE launch where its CLS tap would run; the stream is not written and nothing else about the launch sequence changes: lazy norms,
 * the fused Mlp and the `concurrent` hint stay, and so does the CLS tail unless block depth-1 is tapped -- that needs every row of the last
 * block, which then runs full width, as under final_tokens_out.  blocks == 0: the launches are those of tr_vit_forward.  A bit at or above
 * depth, blocks without tokens_out, norm outside 0 / 1, levels together with features_out or a training tape: TR_ERR_CONFIG; tokens_elems too
 * short: TR_ERR_SHAPE; tokens_out not 16-byte aligned: TR_ERR_ALIGN -- each before any launch.  Eval only. */
typedef struct {
  uint32_t blocks;
  int32_t norm;
  float* tokens_out;
  size_t tokens_elems;
} tr_vit_levels;
int tr_vit_forward_levels(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format, const float* pixel_lut,
                          float* logits, void* workspace, size_t workspace_bytes, int32_t* kept_idx, int32_t* compl_idx, float* soft_out,
                          const float* noise_in, float* features_out, int* tokens_out, int B, tr_stream_t s, const tr_vit_taps* taps,
                          const tr_vit_levels* levels);

/* Decision taps (csrc/tr_decisions.hip): the raw stage slabs of an eval forward -> the per-image decisions of validate.py's `Stage-{loc}`
 * records (validate.py:199-229 on the viz_data of topk.py:196, evit.py:123, tome.py:91-99, sit.py:122, ats.py:78,253, dpcknn.py / kmedoids.py),
 * on the device: ONE launch behind tr_vit_forward* on the same stream, one workgroup per image, the stages walked in block order; no launch
 * for n_stages == 0.  kept_idx / compl_idx / soft are the buffers that forward wrote (idx_elems / soft_elems: their lengths in elements;
 * the slab of block blk starts at blk * B * N0, N0 = patch tokens + 1 <= 1025).  `stages`: HOST table, ascending blocks, at most
 * TR_MAX_DECISION_STAGES entries; n_in = tokens entering the stage (CLS included), 2 <= n_in <= N0, 1 <= k < n_in; P = n_in - 1.
 *   kind     slab                              kept_out [B, W] at kept_off                        assign_out [B, P] at assign_off
 *   PRUNE    kept_idx [B, k] (Top-K, DyViT)    W = k: prev[rel] (first stage: rel)                -
 *   EVIT     kept_idx [B, k]                   W = k + 1: as PRUNE, then one -1; rel == -1 -> -1  -
 *   ATS      kept_idx [B, k] ids: column 0     W = k - 1, rel = id - 1 of columns 1..: first      -
 *            the CLS id, 1-based, 0 = padding  stage as is (padding -1); later stages drop the
 *                                              padding, order kept, then prev[rel], -1 fill
 *   CENTRES  kept_idx [B, k], compl_idx [B, P] W = k: as PRUNE (DPC-KNN, K-Medoids)               the compl_idx rows, copied
 *   TOME     kept_idx (unm [B, na-r], src      -                                                  with pos_a[unm[j]] = j, pos_a[src[j]] = (na-r) + dst[j],
 *            [B, r], dst [B, r]); k = the r                                                       out[0::2] = pos_a, out[1::2] = (na-r) + arange(nb):
 *            asked for, r = min(k, (n_in-1)/2),                                                   (out - 1)[1:]
 *            na = (n_in+1)/2, nb = n_in/2
 *   SOFT     soft [B, k, P] fp32 at soft_off   -                                                  argmax over k, the first maximum wins
 * prev = the kept list of the stage before (its valid entries for a later ATS stage); a stage without a kept list leaves it alone.
 * count_out int32 [n_stages, B]: valid entries of each kept row (W; ATS: the non-zero ids; 0 where the stage has no kept list).  All
 * outputs are stage-relative or composed exactly as the record stores them.  An index is compared with the length of the list it indexes
 * before the read: one that is neither valid nor a padding named above comes out as -2 (a ToMe position nobody claims likewise).
 * n_stages > 32, an unknown kind or blocks not ascending: TR_ERR_CONFIG; n_in / k / an offset outside its buffer: TR_ERR_SHAPE; a pointer
 * not 16-byte aligned: TR_ERR_ALIGN -- each before any launch. */
#define TR_MAX_DECISION_STAGES 32
#define TR_DECISION_PRUNE 0
#define TR_DECISION_EVIT 1
#define TR_DECISION_ATS 2
#define TR_DECISION_CENTRES 3
#define TR_DECISION_TOME 4
#define TR_DECISION_SOFT 5
typedef struct {
  int32_t block;
  int32_t kind;
  int32_t n_in;
  int32_t k;
  int64_t kept_off;     /* elements into kept_out (ignored for TOME / SOFT) */
  int64_t assign_off;   /* elements into assign_out (CENTRES / TOME / SOFT) */
  int64_t soft_off;     /* elements into soft (SOFT) */
} tr_decision_stage;
int tr_stage_decisions(const int32_t* kept_idx, const int32_t* compl_idx, size_t idx_elems, const float* soft, size_t soft_elems,
                       const tr_decision_stage* stages, int n_stages, int B, int N0, int32_t* kept_out, size_t kept_elems,
                       int32_t* count_out, int32_t* assign_out, size_t assign_elems, tr_stream_t s);

/* Dense feature maps (csrc/tr_dense.hip): the final-normed rows of an eval forward (tr_vit_taps.final_tokens_out, fp32 [B, N_last, D]) back
 * on the input's patch grid of P0 = h * w patches.  Two launches behind tr_stage_decisions on the same stream.
 * tr_dense_index: index_out int32 [B, P0] = the row of the last stream (1 ... n_last-1; row 0 is the CLS token) that stands for grid patch
 *   p, -1 where none does.  `kept` / `assign` are tr_stage_decisions' kept_out / assign_out with their lengths, `stages` the same HOST
 *   table (kept_off / assign_off read, soft_off ignored; count_out is not needed: the entries behind a row's count are -1).  One
 *   workgroup per image, P0 <= 1024.  A state cur[p] (patch-relative row, starting at cur[p] = p) walks the stages in block order:
 *     CENTRES, TOME, SOFT   cur[p] = assign[b, cur[p]] where 0 <= cur[p] < n_in - 1 and the result lies in [0, n_out); -1 otherwise
 *                           (SOFT: the hard argmax map; CENTRES: the assignment map, not the centre list)
 *     PRUNE, EVIT, ATS      the list is absolute: cur[p] = the LOWEST j < n_out with kept[b, j] == p, -1 if there is none; entries < 0
 *                           (EViT's fused token, padding, -2) or >= P0 own no patch.  Such a stage behind a stage with a map:
 *                           TR_ERR_CONFIG.
 *   n_out: PRUNE, CENTRES, SOFT k; EVIT k + 1; ATS k - 1; TOME n_in - 1 - min(k, (n_in-1)/2).  index = cur + 1 where cur >= 0.  The last
 *   stage's n_out (P0 for n_stages == 0, which writes the identity 1 ... P0) must equal n_last - 1: TR_ERR_SHAPE.  Patches EViT fused or a
 *   pruning stage dropped come out as -1; the fused token is not followed.  Errors as tr_stage_decisions, each before any launch.
 * tr_dense_gather: out[b, :, p] = tokens[b, index[b, p], :] where 0 <= index[b, p] < n_rows (compared before the read), `fill` elsewhere.
 *   tokens fp32 [B, n_rows, D] contiguous, index int32 [B, P]; out fp32, or bf16 when out_is_bf16 (round to nearest even: the bits of
 *   torch's .to(bfloat16)); layout TR_LAYOUT_NHWC = [B, P, D] (channels last), TR_LAYOUT_NCHW = [B, D, P], anything else TR_ERR_CONFIG.
 *   Every output element is written exactly once (no memset, no atomics).  D % 4 == 0, D <= 1024, 1 <= P <= 1024, n_rows >= 1:
 *   TR_ERR_SHAPE otherwise; pointers 16-byte aligned.  NCHW stores 16 bytes (bf16: 8) along p when P % 4 == 0, single elements otherwise. */
/* The same for L levels -- the streams after L blocks (tr_vit_levels), each behind its own prefix of the stages -- in ONE launch each.
 * tr_dense_index_levels: index_out int32 [L, B, P0].  One workgroup per image walks the stage table once, with tr_dense_index's semantics per
 *   stage kind, and writes level l's index (cur + 1, or -1) behind the last stage whose block is <= level_blocks[l]: a stage reduces in front
 *   of or inside its block, so the stream after block i is behind every stage with block <= i.  A level in front of every stage is the identity
 *   1 ... P0.  level_blocks / level_rows: HOST arrays of L entries (they travel as kernel arguments: a captured graph holds them), the
 *   blocks strictly ascending inside [0, TR_MAX_DEPTH), 1 <= L <= 32 (TR_ERR_CONFIG); level_rows[l] = the token count of the stream after that
 *   block, CLS included: the rows its prefix of stages leaves must equal level_rows[l] - 1 (TR_ERR_SHAPE -- a wrong idea of where a family
 *   reduces does not go unnoticed).  Everything else as tr_dense_index, each refusal before any launch.
 * tr_dense_gather_levels: out[l][b, :, p] = tokens[l * level_stride + (b * level_rows[l] + index[l, b, p]) * D ...] where the index lies in
 *   [0, level_rows[l]), `fill` elsewhere.  tokens: fp32 slabs of level_stride elements (a multiple of 4, at least B * level_rows[l] * D:
 *   tr_vit_levels.tokens_out with level_stride = B * N0 * D), index int32 [L, B, P], out [L, B, P * D] in tr_dense_gather's layouts and
 *   dtypes; per level the bits of tr_dense_gather.  Every element is written exactly once (no memset, no atomics) by one launch whose tile
 *   order has the level as its slowest coordinate. */
int tr_dense_index_levels(const int32_t* kept, size_t kept_elems, const int32_t* assign, size_t assign_elems, const tr_decision_stage* stages,
                          int n_stages, int B, int P0, const int32_t* level_blocks, const int32_t* level_rows, int L, int32_t* index_out,
                          tr_stream_t s);
int tr_dense_gather_levels(const float* tokens, size_t level_stride, const int32_t* level_rows, int L, const int32_t* index, void* out, int layout,
                           int out_is_bf16, float fill, int B, int P, int D, tr_stream_t s);
int tr_dense_index(const int32_t* kept, size_t kept_elems, const int32_t* assign, size_t assign_elems, const tr_decision_stage* stages,
                   int n_stages, int B, int P0, int n_last, int32_t* index_out, tr_stream_t s);
int tr_dense_gather(const float* tokens, const int32_t* index, void* out, int layout, int out_is_bf16, float fill, int B, int P, int n_rows,
                    int D, tr_stream_t s);
/* tr_dense_scatter: the adjoint of tr_dense_gather, the gradient of a map back on the token rows (one launch, no scratch):
 *   dtokens[b, r, :] = sum of dmap[b, :, p] over the patches p with index[b, p] == r, for 0 <= r < n_rows -- row 0 included, as the gather
 *   reads it.  An index entry outside [0, n_rows) (-1, -2, a row too many) owns nothing: it is compared, never used as an address.  dmap in
 *   tr_dense_gather's layouts ([B, D, P] for TR_LAYOUT_NCHW, [B, P, D] for TR_LAYOUT_NHWC; anything else TR_ERR_CONFIG), fp32 or bf16
 *   (dmap_is_bf16); dtokens [B, n_rows, D] fp32, or bf16 when out_is_bf16 (the fp32 sum rounded once, to nearest even) -- the form
 *   tr_vit_backward_dense consumes directly.  The sum is in fp32, one addition after the other in ascending p starting from +0; a row nobody
 *   names is zero; every output element is written exactly once (no memset, no floating-point atomics): the same bits on every launch.
 *   Shapes, alignment and refusals are tr_dense_gather's, each before any launch. */
int tr_dense_scatter(const void* dmap, const int32_t* index, void* dtokens, int layout, int dmap_is_bf16, int out_is_bf16, int B, int P,
                     int n_rows, int D, tr_stream_t s);
/* tr_dense_scatter_levels: the adjoint of tr_dense_gather_levels, the scatter of L levels in ONE launch.  dmaps is a HOST array of L device
 *   pointers (autograd hands over L separate tensors; they travel as kernel arguments, like level_rows), each a map gradient in
 *   tr_dense_scatter's layouts and dtype (one dtype for all).  A NULL entry is a level without a gradient: its slab of dtokens is not touched
 *   and none of its tiles is launched; with every entry NULL nothing is launched.  Level l's index is index + l * B * P, its output
 *   [B, level_rows[l], D] starts at dtokens + l * level_stride elements (fp32, or bf16 when out_is_bf16).  Per level the arithmetic, the
 *   domain check and the bits are tr_dense_scatter's (the same tile bodies); one launch, so L partial last rounds become one.  The
 *   logical order runs through the same XCD remap: channels-last has the level slowest; NCHW has the image slowest and the level next, so
 *   that an XCD's contiguous run holds whole images with all their levels (the levels' tiles do not cost the same under a merge index).  1 <= L <= 32 (TR_ERR_CONFIG); a level's rows must fit level_stride
 *   (TR_ERR_SHAPE); level_stride must keep every slab 16-byte aligned (a multiple of 4 elements, of 8 for bf16 out: TR_ERR_ALIGN); the
 *   other refusals are tr_dense_gather_levels', each before any launch. */
int tr_dense_scatter_levels(const void* const* dmaps, const int32_t* index, void* dtokens, size_t level_stride, const int32_t* level_rows,
                            int L, int layout, int dmap_is_bf16, int out_is_bf16, int B, int P, int D, tr_stream_t s);

/* ---- training: forward that keeps its activations + backward executor (csrc/tr_vit.hip, csrc/tr_train.hip) ----------------------
 * engine.py:50-76: `output = model(samples)` in train mode, `loss.backward()`.  Every family (bf16 operands, fp32 master weights and
 * gradients), up to 640 tokens (224 x 224 and 384 x 384 inputs, or any H x W grid of at most 639 patches).  DyViT (dyvit.py:221-229): noise_in = the Gumbel noise of every stage, fp32 [B,P,2] back to back (torch's
 * -log(Exp(1)) draws); the stages' policies stay on the tape (tr_vit_tape_layout); features_out (nullable) fp32 [B,N0,D]: the final
 * norm of every row (the distillation features, dyvit.py:252-258); tr_vit_backward takes dpred fp32 [stages,B,P] (gradient wrt each
 * stage's out_pred_prob) and dfeat fp32 [B,N0,D] (gradient wrt features_out), both nullable.
 * tr_vit_forward_train: as tr_vit_forward, and every activation the backward needs is written to `tape` (tr_vit_tape_bytes(cfg, B)
 *   bytes, caller-owned; 0 = family / precision without a training path).  drop_scale (nullable, both calls get the same): DropPath
 *   (timm 0.4.12 drop_path, topk.py:78,87,95) as fp32 [2*depth, B]: entry [2i][b] / [2i+1][b] = the scale (0 or 1/keep_prob) of
 *   image b's attention / MLP branch in block i -- the random draw is the caller's.  Dropout: see below.
 * tr_vit_backward: dlogits fp32 [B,classes] -> parameter gradients.  Headless (num_classes == 0): the forward's `logits` are the CLS features
 *   fp32 [B,D], `dlogits` is their gradient fp32 [B,D], no classifier gradient is computed and grads->head_w / head_b may be NULL.
 *   global_pool == 1: the final norm's row gradient is spread over the patch rows by tr_token_pool_bwd (the forward's weights, read from
 *   the tape; no gradient with respect to them); the same units, ranges and frozen-parameter rules.  `w` = the forward's weights; `wt` = same struct with the block
 *   matrices TRANSPOSED (bf16: qkv_w [D,3D], proj_w [D,D], fc1_w [D,Hd], fc2_w [Hd,D]); `grads` = same struct, every pointer an
 *   fp32 buffer of the parameter's shape (written; added to when accumulate != 0).  workspace: tr_vit_backward_workspace_bytes.
 *   [blk_hi .. blk_lo]: the blocks this call walks, in reverse; blk_hi == depth-1 runs the classifier + final norm first, blk_lo == 0
 *   the embedding gradients last; a whole pass is (depth-1, 0) or consecutive ranges in descending order (the stream's gradient
 *   stays in the workspace in between) -- the hook for overlapping the data-parallel gradient reduction (train.py:405-407) with
 *   the backward: reduce one range's gradients on a second stream while the next range runs.
 *   Frozen parameters: a gradient UNIT of `grads` may be NULL -- both pointers, a half-NULL unit is TR_ERR_NULL -- and its work is left
 *   out: {head_w, head_b} (only the classifier's data gradient runs), {norm_g, norm_b} and per block {ln1_g, ln1_b}, {ln2_g, ln2_b} (the
 *   LayerNorm backward without parameter partials), per block {qkv_w, qkv_b}, {proj_w, proj_b}, {fc1_w, fc1_b}, {fc2_w, fc2_b} (left out of
 *   the block's weight-gradient group; what remains is planned as its own group), {pos_embed, cls_token} (no tr_embed_bwd), {patch_w,
 *   patch_b} (no patch weight-gradient product).  The walk stops at the lowest block that takes a gradient: when the embedding unit, the
 *   patch unit and every unit and stage pointer of the blocks below block i are NULL, block i's parameter gradients are the last
 *   launches (its qkv data gradient and a frozen norm1 do not run), the blocks below and the embedding do not run, and a range call
 *   that starts below block i returns TR_OK without a launch; with no block unit at all only the classifier step (and a present final
 *   norm) runs.  A block above the stop block is walked in full whatever is frozen in it.  Stage modules (grads->stage[i]) are not
 *   skipped one by one: a stage the walk reaches needs every pointer its family writes (TR_ERR_NULL otherwise, before any launch); a
 *   stage may be all NULL only at or below the stop block.  With nothing NULL the launch sequence is unchanged.
 * tr_vit_backward_dx: tr_vit_backward plus the gradient with respect to the INPUT image, dx fp32 [B, in_chans, img, img] (nullable: with
 *   dx == NULL the call IS tr_vit_backward).  For the fp32 image of tr_vit_forward_train only (uint8 pixels and augmented batches have no
 *   gradient).  With dx the walk never stops early: it goes down to the embedding whatever is frozen -- every unit may be NULL (a fully
 *   frozen model: an adversarial step on fixed weights), but the stage pointers of EVERY reduction stage are then required (TR_ERR_NULL
 *   otherwise).  wt->patch_w = the patch weight transposed, bf16 [in_chans*patch*patch, D] (TR_ERR_NULL when missing); shapes are those of
 *   tr_patch_embed_dgrad (TR_ERR_SHAPE before any launch otherwise).  The one extra launch, tr_patch_embed_dgrad on the bf16 gradient of
 *   the embedded stream (after pos_drop's mask), runs in the call whose blk_lo == 0, beside the embedding gradients; the other range
 *   calls of a pass take the same dx (so that they walk the same blocks) and do not touch it.  dx is overwritten, never accumulated
 *   into; no workspace beyond tr_vit_backward_workspace_bytes. */
size_t tr_vit_tape_bytes(const tr_vit_config* cfg, int B);
int tr_vit_forward_train(const tr_vit_config* cfg, const tr_vit_weights* w, const float* img, float* logits, void* workspace,
                         size_t workspace_bytes, void* tape, size_t tape_bytes, const float* noise_in, float* features_out,
                         const float* drop_scale, int* tokens_out, int B, tr_stream_t s, const uint8_t* dropout_keep, float drop_rate);
int tr_vit_forward_train_pixels(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format, const float* pixel_lut,
                                float* logits, void* workspace, size_t workspace_bytes, void* tape, size_t tape_bytes, const float* noise_in,
                                float* features_out, const float* drop_scale, int* tokens_out, int B, tr_stream_t s, const uint8_t* dropout_keep,
                                float drop_rate);
/* tr_vit_forward_train_pixels with the device-side augmentation of tr_im2col_u8_aug_bf16: input_format is one of the uint8 formats, B is
 * even, aug / aug_noise / aug_noise_len are that call's table and noise.  The tape's column matrix (the patch GEMM's operand and
 * PatchEmbed's weight-gradient operand) is that of the augmented image, so tr_vit_backward needs nothing else. */
int tr_vit_forward_train_aug(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format, const float* pixel_lut,
                             const tr_augment_rec* aug, const float* aug_noise, long aug_noise_len, float* logits, void* workspace,
                             size_t workspace_bytes, void* tape, size_t tape_bytes, const float* noise_in, float* features_out,
                             const float* drop_scale, int* tokens_out, int B, tr_stream_t s, const uint8_t* dropout_keep, float drop_rate);
/* Dropout (timm's drop_rate, train.py:46 --drop: pos_drop topk.py:186, proj_drop :53, the Mlp's two nn.Dropout): dropout_keep (nullable
 * = drop_rate 0; both calls get the same) is the caller's keep mask, 1 byte per element (non-zero = keep), tr_vit_dropout_mask_bytes()
 * bytes in the order the forward consumes them -- the embedded tokens [B,N0,D], then per block proj's output rows, the Mlp's hidden
 * layer and its output: the order in which the reference module draws them.  Survivors are scaled by 1 / (1 - drop_rate).
 * (attn_drop_rate -- dropout on the attention probabilities, topk.py:49 -- is not built; the reference's CLI cannot set it either.) */
/* Dense feature maps in training: tr_vit_forward_train_dense is the superset training forward -- input_format TR_INPUT_F32 (no LUT), a uint8
 * format (tr_vit_forward_train_pixels) or a uint8 format with aug != NULL (tr_vit_forward_train_aug) -- that also leaves, in caller-owned
 * buffers, what a dense map of the last stream and its gradient need (tr_vit_dense_train):
 *   tokens_out   fp32 [B, N0, D] holding [B, N_last, D]: the final norm of every row, in fp32 arithmetic (the arithmetic of DyViT's
 *                features_out) -- the `tokens` of tr_dense_gather
 *   stream_out   fp32 [B, N0, D] holding [B, N_last, D]: the stream entering the final norm (what DyViT keeps on the tape as xfin_all; the
 *                tape's layout is untouched), the `stream` of tr_vit_backward_dense
 *   kept_idx / compl_idx (int32, depth * B * N0 each: idx_elems) and soft_out (fp32, soft_elems; NULL for a family without soft stages):
 *                the decisions in the eval slab format of tr_stage_decisions, slab of block blk at blk * B * N0 -- device-to-device copies
 *                of the tape's decision slots on the stream, behind the forward; both NULL: no copies
 * No host synchronisation.  The logits, the tape and every launch in front of the final norm are tr_vit_forward_train's.  DyViT (every token
 * stays under a policy; it has features_out): TR_ERR_CONFIG.  A NULL struct, tokens_out or stream_out: TR_ERR_NULL; a buffer too small:
 * TR_ERR_SHAPE; not 16-byte aligned: TR_ERR_ALIGN -- each before any launch.
 * tr_vit_backward_dense: tr_vit_backward_dx (dx nullable) plus dtokens, the gradient with respect to tokens_out [B, N_last, D] -- bf16
 *   (dtokens_is_bf16: tr_dense_scatter's output, read as it is) or fp32 (rounded to bf16 first, as dfeat is) -- and `stream`, the forward's
 *   stream_out.  The call with blk_hi == depth-1 runs a second pass of the final norm's backward over all rows behind the head's (behind
 *   tr_token_pool_bwd's spread with global_pool == 1), adding into the stream gradient and into the norm's parameter gradients; the other
 *   range calls take the same arguments and do not read them.  With dtokens == NULL the call IS tr_vit_backward_dx.  dtokens without stream:
 *   TR_ERR_NULL; DyViT: TR_ERR_CONFIG; not 16-byte aligned: TR_ERR_ALIGN. */
typedef struct {
  float* tokens_out;
  float* stream_out;
  size_t rows_elems;    /* elements of tokens_out and of stream_out: at least B * N0 * D */
  int32_t* kept_idx;
  int32_t* compl_idx;
  size_t idx_elems;     /* elements of kept_idx and of compl_idx: at least depth * B * N0 */
  float* soft_out;
  size_t soft_elems;
} tr_vit_dense_train;
int tr_vit_forward_train_dense(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format, const float* pixel_lut,
                               const tr_augment_rec* aug, const float* aug_noise, long aug_noise_len, float* logits, void* workspace,
                               size_t workspace_bytes, void* tape, size_t tape_bytes, const float* noise_in, const float* drop_scale,
                               int* tokens_out, int B, tr_stream_t s, const uint8_t* dropout_keep, float drop_rate,
                               const tr_vit_dense_train* dense);
int tr_vit_backward_dense(const tr_vit_config* cfg, const tr_vit_weights* w, const tr_vit_weights* wt, const tr_vit_weights* grads,
                          const float* dlogits, const float* dpred, const float* dfeat, const float* drop_scale, const void* tape,
                          size_t tape_bytes, void* workspace, size_t workspace_bytes, int accumulate, int blk_hi, int blk_lo, int B,
                          tr_stream_t s, const uint8_t* dropout_keep, float drop_rate, float* dx, const void* dtokens, int dtokens_is_bf16,
                          const float* stream);
/* Multi-level dense feature maps in training.  tr_vit_forward_train_levels is tr_vit_forward_train_dense plus level taps (tr_vit_train_levels):
 * the one entry where level taps and a training tape go together (tr_vit_forward_levels keeps refusing a tape).  After every block of
 * `blocks` (bit i = block i) the rows of the stream with the residual pending there -- the training forward's DropPath-scaled,
 * dropout-masked branch -- go to the next slab (level l at l * B * N0 * D elements, holding [B, N_l, D]):
 *   norm == 0   tokens_out takes the summed rows (tr_cls_tap at row stride D); stream_out is not read
 *   norm == 1   stream_out takes the summed rows and tokens_out their fp32 final norm, ONE launch per level (tr_level_tap_norm)
 * The taps run where they run in eval and change nothing else: the logits, the tape and every other launch are tr_vit_forward_train's.
 * `dense` carries the decision slabs (kept_idx / compl_idx / soft_out) as in tr_vit_forward_train_dense; its tokens_out / stream_out may both
 * be NULL here (the last block's pair is then not written: a level at block depth-1 serves it).  DyViT: TR_ERR_CONFIG; a NULL struct or
 * buffer: TR_ERR_NULL; a buffer too small: TR_ERR_SHAPE; not 16-byte aligned: TR_ERR_ALIGN; blocks == 0, a block outside the depth or norm
 * outside {0, 1}: TR_ERR_CONFIG -- each before any launch.
 * tr_vit_backward_levels is tr_vit_backward_dense plus the level gradients (tr_vit_level_grads).  `present` has bit l set where level l (the
 * l-th set bit of `blocks`) has a gradient; dtokens holds level l's token gradient at l * level_stride elements -- bf16 for norm == 1 (the
 * gradient of the final-normed rows, tr_dense_scatter_levels' output), fp32 for norm == 0 (of the rows as they stand) -- and stream the
 * forward's stream_out (norm == 1).  A present level at block i < depth-1 is injected in front of block i's Mlp backward, where the stream
 * gradient is that of the summed stream after block i: norm == 1 runs the final norm's backward over all B * N_i rows (adding into the
 * stream gradient, rewriting its bf16 copy, adding into the final norm's parameter gradients, reduced at once); norm == 0 runs
 * tr_stream_grad_add.  The level at block depth-1 enters where tr_vit_backward_dense's dtokens enter (the entry's own dtokens must then be
 * NULL).  A level below the stop block of a partly frozen model adds nothing to the stream gradient (nobody reads it); with norm == 1 and a
 * trainable final norm it still adds to the norm's parameter gradients: these passes run in descending block order behind the walk, in the
 * call whose range holds the stop block (no block walked: in the call with blk_hi == depth-1), so a single call and a pass of range calls
 * add in the same order.  Every range call takes the same arguments; a level is handled by the call whose range holds its block.  With
 * lev == NULL or present == 0 the call IS tr_vit_backward_dense. */
typedef struct {
  uint32_t blocks;
  int32_t norm;
  float* tokens_out;
  float* stream_out;    /* norm == 1 */
  size_t level_elems;   /* elements of tokens_out (and of stream_out): at least popcount(blocks) * B * N0 * D */
} tr_vit_train_levels;
typedef struct {
  uint32_t blocks;
  int32_t norm;
  uint32_t present;
  const void* dtokens;
  const float* stream;
  size_t level_stride;  /* elements between two levels' slabs, at least B * N0 * D */
} tr_vit_level_grads;
int tr_vit_forward_train_levels(const tr_vit_config* cfg, const tr_vit_weights* w, const void* img, int input_format, const float* pixel_lut,
                                const tr_augment_rec* aug, const float* aug_noise, long aug_noise_len, float* logits, void* workspace,
                                size_t workspace_bytes, void* tape, size_t tape_bytes, const float* noise_in, const float* drop_scale,
                                int* tokens_out, int B, tr_stream_t s, const uint8_t* dropout_keep, float drop_rate,
                                const tr_vit_dense_train* dense, const tr_vit_train_levels* levels);
int tr_vit_backward_levels(const tr_vit_config* cfg, const tr_vit_weights* w, const tr_vit_weights* wt, const tr_vit_weights* grads,
                           const float* dlogits, const float* dpred, const float* dfeat, const float* drop_scale, const void* tape,
                           size_t tape_bytes, void* workspace, size_t workspace_bytes, int accumulate, int blk_hi, int blk_lo, int B,
                           tr_stream_t s, const uint8_t* dropout_keep, float drop_rate, float* dx, const void* dtokens, int dtokens_is_bf16,
                           const float* stream, const tr_vit_level_grads* lev);
size_t tr_vit_dropout_mask_bytes(const tr_vit_config* cfg, int B);
/* fp32 master parameters -> the bf16 operand copies of the GEMMs, every matrix of a model in ONE launch (an optimizer step changes them
 * all: engine.py:76-91).  Item i: src fp32 [rows, cols] contiguous -> dst bf16 [rows, cols] (nullable) and dst_t bf16 [cols, rows]
 * (nullable: the transposed copy the data-gradient GEMMs read).  items / first are DEVICE arrays; first[i] = tiles before item i with
 * ceil(rows/64) * ceil(cols/64) tiles per item, total_tiles = first[n_items]. */
typedef struct tr_cast_item { const void* src; void* dst; void* dst_t; int rows, cols; } tr_cast_item;
int tr_cast_pack_bf16(const tr_cast_item* items, const int* first, int n_items, int total_tiles, tr_stream_t s);
/* One launch for the optimizer step of the fine-tune path (csrc/tr_optim.hip): AdamW on every parameter (torch's fused AdamW
 * arithmetic, bit for bit), the gradient zeroed behind it when `zero_grads` != 0, and the bf16 (+ transposed) operand copies rewritten
 * in the same pass.
 * Item i: p, g, m (exp_avg), v (exp_avg_sq) fp32 [rows, cols] contiguous; dst bf16 [rows, cols] / dst_t bf16 [cols, rows] nullable;
 * group selects lr8[group] / wd8[group] (up to 8 parameter groups per launch).  items / first: DEVICE arrays, first[i] = tiles before
 * item i (ceil(rows/64) * ceil(cols/64) per item), total_tiles = first[n_items].  bias_correction1 = 1 - beta1^step,
 * bias_correction2_sqrt = sqrt(1 - beta2^step), computed by the caller in double and rounded to float. */
typedef struct tr_adamw_item { void* p; void* g; void* m; void* v; void* dst; void* dst_t; int rows, cols, group, pad_; } tr_adamw_item;
int tr_adamw_step(const tr_adamw_item* items, const int* first, int n_items, int total_tiles, double beta1, double beta2, double eps,
                  float bias_correction1, float bias_correction2_sqrt, const double* lr8, const double* wd8, int zero_grads,
                  tr_stream_t s);
/* LayerScale (timm's init_values: x + gamma o branch(x); csrc/tr_layerscale.hip).  The executor has no gamma: it reads the FOLDED
 * operands W' = fl32(gamma[d] * W[d,k]), b' = fl32(gamma[d] * b[d]) of the Linear that ends a branch and produces their gradients.
 * items: a DEVICE array, 16-byte aligned.  shapes: a HOST array of n_items (rows, cols) pairs -- the same values as in the items -- from
 * which the grid is sized and which are refused (TR_ERR_SHAPE, before any launch) unless every one is a positive multiple of 64.
 * first: the workgroups before the item -- (rows/64) * (cols/64) per item for the fold, rows/4 for the unfold.  Every pointer 16-byte aligned.
 * tr_layerscale_fold, item i: w fp32 [rows, cols], b fp32 [rows], gamma fp32 [rows] -> dst [rows, cols] (bf16: the fp32 product rounded to
 * nearest-even; fp32 when dst_is_f32; nullable), dst_t bf16 [cols, rows] (nullable), b_dst fp32 [rows] (nullable; b may then be NULL). */
typedef struct tr_ls_fold_item { const void* w; const void* b; const void* gamma; void* dst; void* dst_t; void* b_dst; int rows, cols, first, pad_; } tr_ls_fold_item;
int tr_layerscale_fold(const tr_ls_fold_item* items, const int* shapes, int n_items, int dst_is_f32, tr_stream_t s);
/* The gradients of the real parameters from those of the folded operands.  Item i: dw_f fp32 [rows, cols], db_f fp32 [rows] (the executor's
 * gradients of W', b'); w, b, gamma the fp32 parameters; dw [rows, cols], db [rows], dgamma [rows] fp32, each nullable (a frozen parameter):
 *   dw = fl(gamma * dw_f), db = fl(gamma * db_f) -- under `accumulate` fl(old + fl(gamma * x)), two roundings;
 *   dgamma[d] = sum_k dw_f[d,k] * w[d,k] + db_f[d] * b[d] in fp32 (under `accumulate` added to the old value), summed in an order that
 *   depends on cols alone: the same bits on every launch.  dw_f / db_f are only read. */
typedef struct tr_ls_unfold_item { const void* dw_f; const void* db_f; const void* w; const void* b; const void* gamma; void* dw; void* db; void* dgamma;
                                   int rows, cols, first, pad_; } tr_ls_unfold_item;
int tr_layerscale_unfold_grad(const tr_ls_unfold_item* items, const int* shapes, int n_items, int accumulate, tr_stream_t s);
int tr_dropout_bf16(const uint16_t* src, uint16_t* dst, const uint8_t* keep, float mul, size_t n, tr_stream_t s);
int tr_dropout_f32(const float* src, float* dst, const uint8_t* keep, float mul, size_t n, tr_stream_t s);
/* Byte offsets of block blk's tape slots (x0,x1,xn1,qkv,ao,dattn,x2,xn2,pre,h,idx,idx2,scores,size) followed by its token counts
 * (entering, in attention, in the MLP) and its reduction count: lets a host read the decisions of a training forward. */
int tr_vit_tape_layout(const tr_vit_config* cfg, int B, int blk, size_t* out18);
size_t tr_vit_backward_workspace_bytes(const tr_vit_config* cfg, int B);
int tr_vit_backward(const tr_vit_config* cfg, const tr_vit_weights* w, const tr_vit_weights* wt, const tr_vit_weights* grads,
                    const float* dlogits, const float* dpred, const float* dfeat, const float* drop_scale, const void* tape,
                    size_t tape_bytes, void* workspace, size_t workspace_bytes, int accumulate, int blk_hi, int blk_lo, int B,
                    tr_stream_t s, const uint8_t* dropout_keep, float drop_rate);
int tr_vit_backward_dx(const tr_vit_config* cfg, const tr_vit_weights* w, const tr_vit_weights* wt, const tr_vit_weights* grads,
                       const float* dlogits, const float* dpred, const float* dfeat, const float* drop_scale, const void* tape,
                       size_t tape_bytes, void* workspace, size_t workspace_bytes, int accumulate, int blk_hi, int blk_lo, int B,
                       tr_stream_t s, const uint8_t* dropout_keep, float drop_rate, float* dx);

#ifdef __cplusplus
}
#endif
#endif /* TOKENREDUCTION_HIP_H */
