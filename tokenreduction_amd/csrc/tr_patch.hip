// PatchEmbed + cls_token + pos_embed in ONE launch (timm PatchEmbed, call sites topk.py:181-186; deit_viz.py the same):
//   x[b, 0, :]     = cls_token + pos_embed[0]
//   x[b, 1 + p, :] = W . patch(b, p) + bias + pos_embed[1 + p]          W = proj.weight viewed [D, C*16*16]
// replacing im2col (fp32 image -> bf16 [B*P, 768] columns: 154 MB read + 77 MB written at batch 256) + GEMM (77 MB read again) +
// the cls/pos kernel of the eval forward.  The unfold happens on the way INTO the LDS: a K-step of 64 is four 64-byte runs of one
// image row segment per patch, loaded fp32 into registers, rounded to bf16 and written into the swizzled [rows][64] operand image.
//
// One workgroup (8 waves) per (image, chunk of <= 208 patches, 384 output columns): the image's patches are the tile's rows, so the
// fp32 image is read from HBM exactly once (DeiT-B: once per 384-column half, the second from L2), and the launch has one workgroup per CU
// at batch 256.  Wave w accumulates all 13 row blocks x the column blocks {w, w+8, w+16} (156 accumulator registers): LDS reads per MFMA
// 16 : 39.  W K-slabs arrive by LDS-DMA, double-buffered like A.  The kernel is HBM-bound by design (231 MB per launch at batch 256
// against 29.6 GFLOP: 12 us of matrix time), so what matters is bytes in flight: every thread holds the next K-step's 7 x 16 B.
// Epilogue: three passes over 128 output columns through an LDS staging image, so that every store is a full 128-byte line.
// Summation order: (sum of products + bias) + pos_embed -- the three-launch path adds pos_embed after its first K-step, so the two
// differ in the last bit; the eval executor therefore takes this kernel for EVERY batch size of a supported shape (an image's tokens must
// not depend on its batch), although below ~half a chip of workgroups the three launches are faster (batch 64 DeiT-S: 45 vs 35 us).
#include "tr_common.h"

namespace {

constexpr int PE_RB = 13;                   // 16-row blocks per chunk (196 patches of a 224^2 image -> one chunk)
constexpr int PE_ROWS = PE_RB * 16;
constexpr int PE_NC = 384;                  // output columns per workgroup
constexpr int PE_A_BYTES = PE_ROWS * 128;   // one A slot: [208][64 bf16]
constexpr int PE_W_BYTES = PE_NC * 128;     // one W slot: [384][64 bf16]
constexpr int PE_STAGE_LD = 528;            // epilogue staging row stride (128 fp32 + 16 B)
constexpr int PE_LDS = 2 * (PE_A_BYTES + PE_W_BYTES);
static_assert(PE_LDS >= PE_ROWS * PE_STAGE_LD, "the epilogue staging image reuses the operand ring");
constexpr int PE_ITEMS = 7;                 // float4 loads per thread and K-step (208 rows x 16 / 512 = 6.5)

__device__ __forceinline__ int pswz(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }      // W slabs (written by LDS-DMA)
// The A image (fp32 pixels -> bf16, written by ds_write_b64) has a swizzle of its own.  A 16-lane store group holds four consecutive rows x
// the four float4 of a 16-pixel run, i.e. the 32-byte chunk PAIR {2 r, 2 r + 1} of four rows: with the ring's (row >> 1) & 7 those four rows
// land on one pair of the 128-byte bank window -- 4-way conflicts on every store (27.7 % of the kernel's LDS cycles, r05 SQ counters;
// tools/lds_sim.py: 16 cycles per wave-instruction, 4 without).  XOR 2 (row & 3) moves the four rows to four pairs; the per-quad term
// keeps the fragment reads (16 rows x 4 chunks per ds_read_b128, banks mod 64) conflict-free.  Same bits out: only where a value sits.
__device__ __forceinline__ int aswz(int row, int chunk) {
  return row * 128 + ((chunk ^ ((2 * (row & 3)) ^ ((0x1320 >> (4 * ((row >> 2) & 3))) & 3))) << 4);      // quad term {0, 2, 3, 1}
}

__device__ __forceinline__ void dma_piece(const uint16_t* sbase, unsigned voff, unsigned lds_dst) {
  asm volatile(
      "s_mov_b32 m0, %[ld]\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %[o], %[b]"
      :
      : [o] "v"(voff), [b] "s"(sbase), [ld] "s"(lds_dst)
      : "memory", "m0");
}

// Raw uint8 pixels (tr_patch_embed_u8_bf16): the same kernel with another A loader.  An item is a whole 16-pixel run of one patch row:
// 16 B in NCHW; in NHWC (C = 3) the run's 48 B, all three channels, from which the K-step's channel is picked in registers -- the K order
// stays channel-major, and the two later channels of a run come from L2.  A K-step takes 208 x 4 = 832 items: two per thread.  Every pixel
// goes through lut[c][v] (C x 256 fp32 in LDS, behind the operand ring) and is rounded to bf16 by the same pack_bf16x2 as the fp32 loader:
// the A operand is bitwise the one the fp32 kernel builds from the normalized image, in the same K order, and so are the accumulators.
enum { PE_F32 = 0, PE_U8_NCHW = 1, PE_U8_NHWC3 = 2 };
constexpr int PE_U8_ITEMS = 2;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

__device__ __forceinline__ unsigned byte_of(const u32x4* w, int k) { return (w[k >> 4][(k >> 2) & 3] >> (8 * (k & 3))) & 0xffu; }

// the 16 pixels of one run through the LUT, as bf16 into the run's two 16-byte chunks of its A row.  CH < 0 (NCHW): w[0] holds the run;
// CH = 0..2 (NHWC, C = 3): w[0..2] hold 48 bytes, pixel j of channel CH is byte 3 j + CH.  Byte positions are compile-time constants.
template <int CH>
__device__ __forceinline__ void u8_commit(const u32x4* w, const float* lutc, unsigned char* dst0, unsigned char* dst1) {
  unsigned pk[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k0 = CH < 0 ? 2 * j : 6 * j + CH, k1 = CH < 0 ? 2 * j + 1 : 6 * j + 3 + CH;
    pk[j] = pack_bf16x2(lutc[byte_of(w, k0)], lutc[byte_of(w, k1)]);
  }
  *reinterpret_cast<uint4*>(dst0) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
  *reinterpret_cast<uint4*>(dst1) = make_uint4(pk[4], pk[5], pk[6], pk[7]);
}

template <int FMT>
__global__ __launch_bounds__(512, 1) void patch_embed_kernel(const void* __restrict__ img, const float* __restrict__ lut,
                                                             const uint16_t* __restrict__ W,
                                                             const float* __restrict__ bias, const float* __restrict__ cls,
                                                             const float* __restrict__ pos, float* __restrict__ x, int C, int H, int IW, int gw,
                                                             int P, int D, int nchunk) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.x / nchunk, chunk = blockIdx.x - b * nchunk;
  const int nb = blockIdx.y;                                   // 384-column slab of the output
  const int p0 = chunk * PE_ROWS, rows = min(PE_ROWS, P - p0);
  const int K = C * 256, nk = K / 64;
  unsigned char* sA = smem;
  unsigned char* sW = smem + 2 * PE_A_BYTES;
  float* sL = reinterpret_cast<float*>(smem + PE_LDS);         // uint8 forms: the pixel LUT [C][256], behind the ring
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
  constexpr int NIT = FMT == PE_F32 ? PE_ITEMS : PE_U8_ITEMS;
  constexpr int NV = FMT == PE_U8_NHWC3 ? 3 : 1;               // 16-byte loads per uint8 item

  // ---- per-thread source offsets (floats, without the channel / row-group term) and LDS destinations of the A items
  // item e = tid + 512 it  ->  q = e & 3 (float4 of the 16-pixel run), m = (e >> 2) % rows_pad, r = (e >> 2) / rows_pad (image row of the K-step)
  // ordered (r, m, q): consecutive threads walk along an image row (patches px, px+1, ...: contiguous pixels)
  // uint8: item e -> m = e % rows_pad, r = e / rows_pad, the whole run; offsets in bytes, destination = chunk 2 r (chunk 2 r + 1 is adst ^ 16)
  unsigned aoff[NIT];
  int adst[NIT];
  const float* ibase = static_cast<const float*>(img) + (FMT == PE_F32 ? (size_t)b * C * H * IW : 0);
  const uint8_t* ubase = static_cast<const uint8_t*>(img) + (FMT != PE_F32 ? (size_t)b * C * H * IW : 0);
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int e = tid + 512 * it;
    if constexpr (FMT == PE_F32) {
      const int q = e & 3, mr = e >> 2;
      const int r = mr / PE_ROWS, m = mr - r * PE_ROWS;          // r in 0..3 for e < 4 * 208 * 4 = 3328 (it = 6: e < 3584 -> r may reach 4: masked)
      const bool live = r < 4 && m < rows;
      const int p = min(p0 + m, P - 1);
      const int py = p / gw, px = p - py * gw;
      aoff[it] = (unsigned)((py * 16 + min(r, 3)) * IW + px * 16 + q * 4);
      adst[it] = live ? aswz(m, 2 * r + (q >> 1)) + (q & 1) * 8 : -1;
    } else {
      const int r = e / PE_ROWS, m = e - r * PE_ROWS;            // r in 0..4 for e < 1024: r == 4 masked
      const bool live = r < 4 && m < rows;
      const int p = min(p0 + m, P - 1);
      const int py = p / gw, px = p - py * gw;
      aoff[it] = (unsigned)(((py * 16 + min(r, 3)) * IW + px * 16) * NV);
      adst[it] = live ? aswz(m, 2 * r) : -1;
    }
  }
  if constexpr (FMT != PE_F32)
    for (int i = tid; i < C * 256; i += 512) sL[i] = lut[i];
  // rows of the chunk past the last patch: zero operand rows in both slots (never written again)
  for (int i = tid; i < (PE_ROWS - rows) * 8 * 2; i += 512) {
    const int slot = i & 1, c = (i >> 1) & 7, m = rows + (i >> 4);
    *reinterpret_cast<uint4*>(sA + slot * PE_A_BYTES + m * 128 + c * 16) = make_uint4(0u, 0u, 0u, 0u);
  }
  // W pieces of this wave: rows 48 w + 8 j + l3 of the slab, LDS position (row, pc) holds logical chunk pc ^ ((row >> 1) & 7)
  unsigned woff[6];
  const int l3 = lane >> 3, pc = lane & 7;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int row = wave * 48 + j * 8 + l3;
    woff[j] = (unsigned)(((nb * PE_NC + row) * K + ((pc ^ ((row >> 1) & 7)) << 3)) * 2);
  }
  const unsigned wdst = lds0 + 2 * PE_A_BYTES + wave * 48 * 128;

  f32x4 areg[FMT == PE_F32 ? PE_ITEMS : 1];
  u32x4 ureg[NIT][NV];
  auto issue = [&](int kt, int slot) {
#pragma unroll
    for (int j = 0; j < 6; ++j) dma_piece(W, woff[j] + (unsigned)kt * 128u, wdst + slot * PE_W_BYTES + j * 1024);
    if constexpr (FMT == PE_F32) {
      const float* src = ibase + (size_t)(kt >> 2) * H * IW + (size_t)((kt & 3) * 4) * IW;
#pragma unroll
      for (int it = 0; it < PE_ITEMS; ++it)      // nontemporal: the image is read once -- kept out of the caches the forward lives in (-12 us per forward)
        areg[it] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(src + aoff[it]));
    } else if constexpr (FMT == PE_U8_NCHW) {    // plain loads: measured 62.7 -> 58.2 us against nontemporal at DeiT-S 224, batch 256
      const uint8_t* src = ubase + (size_t)(kt >> 2) * H * IW + (size_t)((kt & 3) * 4) * IW;
#pragma unroll
      for (int it = 0; it < NIT; ++it) ureg[it][0] = *reinterpret_cast<const u32x4*>(src + aoff[it]);
    } else {                                     // NHWC: every channel of the run, 3 x 16 B (the next two channels re-read them from L2)
      const uint8_t* src = ubase + (size_t)((kt & 3) * 4) * IW * 3;
#pragma unroll
      for (int it = 0; it < NIT; ++it)
#pragma unroll
        for (int v = 0; v < NV; ++v) ureg[it][v] = *reinterpret_cast<const u32x4*>(src + aoff[it] + 16 * v);
    }
  };
  auto commit = [&](int kt, int slot) {
    if constexpr (FMT == PE_F32) {
#pragma unroll
      for (int it = 0; it < PE_ITEMS; ++it)
        if (adst[it] >= 0) {
          uint2 v;
          v.x = pack_bf16x2(areg[it][0], areg[it][1]);
          v.y = pack_bf16x2(areg[it][2], areg[it][3]);
          *reinterpret_cast<uint2*>(sA + slot * PE_A_BYTES + adst[it]) = v;
        }
    } else {
      const int c = kt >> 2;                     // the K-step's channel (uniform)
      const float* lutc = sL + c * 256;
#pragma unroll
      for (int it = 0; it < NIT; ++it)
        if (adst[it] >= 0) {
          unsigned char* d0 = sA + slot * PE_A_BYTES + adst[it];
          unsigned char* d1 = sA + slot * PE_A_BYTES + (adst[it] ^ 16);
          if constexpr (FMT == PE_U8_NCHW) u8_commit<-1>(ureg[it], lutc, d0, d1);
          else if (c == 0) u8_commit<0>(ureg[it], lutc, d0, d1);
          else if (c == 1) u8_commit<1>(ureg[it], lutc, d0, d1);
          else u8_commit<2>(ureg[it], lutc, d0, d1);
        }
    }
  };

  f32x4 acc[PE_RB][3];
#pragma unroll
  for (int i = 0; i < PE_RB; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  issue(0, 0);
  if constexpr (FMT != PE_F32) __syncthreads();               // the LUT is in LDS
  commit(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int slot = kt & 1;
    if (kt + 1 < nk) issue(kt + 1, slot ^ 1);
    __builtin_amdgcn_sched_barrier(0);
    const unsigned char* a = sA + slot * PE_A_BYTES;
    const unsigned char* w = sW + slot * PE_W_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 wf[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(w + pswz(16 * (wave + 8 * j) + li, 4 * ks + g));
#pragma unroll
      for (int i = 0; i < PE_RB; ++i) {
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(a + aswz(16 * i + li, 4 * ks + g));
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af, acc[i][j], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < nk) commit(kt + 1, slot ^ 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the W slab of the next step (LDS-DMA: invisible to the compiler's counters)
    __syncthreads();
  }

  // ---- epilogue: pass j stages the columns [128 j, 128 j + 128) of the slab -- wave w holds its columns 16 w .. 16 w + 15
  float* xrow0 = x + ((size_t)b * (P + 1) + 1 + p0) * D + nb * PE_NC;
  const int ch = tid & 31;                                       // this thread's 16-byte column group of a staged row (512 % 32 == 0)
#pragma unroll
  for (int j = 0; j < 3; ++j) {
#pragma unroll
    for (int i = 0; i < PE_RB; ++i)
      *reinterpret_cast<f32x4*>(smem + (16 * i + li) * PE_STAGE_LD + 64 * wave + 16 * g) = acc[i][j];
    __syncthreads();
    const int col = nb * PE_NC + 128 * j + 4 * ch;
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + col);
#pragma unroll
    for (int it = 0; it < PE_RB; ++it) {
      const int m = (tid >> 5) + 16 * it;
      if (m < rows) {
        f32x4 v = *reinterpret_cast<const f32x4*>(smem + m * PE_STAGE_LD + 16 * ch);
        const f32x4 pv = *reinterpret_cast<const f32x4*>(pos + (size_t)(1 + p0 + m) * D + col);
        v = v + bv + pv;
        *reinterpret_cast<f32x4*>(xrow0 + (size_t)m * D + 128 * j + 4 * ch) = v;
      }
    }
    __syncthreads();
  }
  if (chunk == 0 && tid < PE_NC / 4) {                           // the CLS row of this image
    const int col = nb * PE_NC + 4 * tid;
    const f32x4 c = *reinterpret_cast<const f32x4*>(cls + col), pv = *reinterpret_cast<const f32x4*>(pos + col);
    *reinterpret_cast<f32x4*>(x + (size_t)b * (P + 1) * D + col) = c + pv;
  }
}

template <int FMT>
int launch_patch_embed(const void* img, const float* lut, const uint16_t* W, const float* bias, const float* cls, const float* pos, float* x,
                       int B, int C, int H, int IW, int D, tr_stream_t s, const char* what) {
  const int gw = IW / 16, P = (H / 16) * gw, nchunk = (P + PE_ROWS - 1) / PE_ROWS;
  TR_REQUIRE((size_t)D * C * 256 * 2 < ((size_t)1 << 32), TR_ERR_SHAPE, "%s: weight beyond the 32-bit offset range", what);
  const int lds = PE_LDS + (FMT == PE_F32 ? 0 : C * 256 * 4);
  hipStream_t st = static_cast<hipStream_t>(s);
  TR_RESERVE_LDS(reinterpret_cast<const void*>(patch_embed_kernel<FMT>), lds, what);
  tr_prof_note("patch_embed_kernel", 2.0 * B * P * (double)D * C * 256,
               (double)B * C * H * IW * (FMT == PE_F32 ? 4.0 : 1.0) + (double)B * (P + 1) * D * 4.0);
  hipLaunchKernelGGL(patch_embed_kernel<FMT>, dim3(B * nchunk, D / PE_NC), dim3(512), lds, st, img, lut, W, bias, cls, pos, x, C, H, IW, gw, P,
                     D, nchunk);
  TR_CHECK_LAUNCH(what);
  return TR_OK;
}

}  // namespace

// 1 when tr_patch_embed_hw_bf16 takes this shape (else the executor runs im2col + GEMM + cls/pos).  C * H * W < 2^30 keeps the kernel's 32-bit
// per-thread source offsets (aoff: bytes of a uint8 NHWC plane at most) in range.
extern "C" int tr_patch_embed_hw_supported(int C, int H, int W, int patch, int D) {
  return patch == 16 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0 && C >= 1 && D > 0 && D % PE_NC == 0 && (size_t)C * H * W < ((size_t)1 << 30);
}

// the square form: H = W = HW
extern "C" int tr_patch_embed_supported(int C, int HW, int patch, int D) {
  return patch == 16 && HW % 16 == 0 && C >= 1 && D % PE_NC == 0 && (size_t)C * HW * HW < ((size_t)1 << 30);
}

namespace {

// the checks behind the alignment of every fp32 entry, then the launch
int patch_embed_f32(const float* img, const uint16_t* W, const float* bias, const float* cls, const float* pos, float* x, int B, int C, int H,
                    int IW, int D, tr_stream_t s, const char* what) {
  TR_REQUIRE(tr_aligned16(img) && tr_aligned16(W) && tr_aligned16(bias) && tr_aligned16(cls) && tr_aligned16(pos) && tr_aligned16(x), TR_ERR_ALIGN,
             "%s: pointers must be 16-byte aligned", what);
  return launch_patch_embed<PE_F32>(img, nullptr, W, bias, cls, pos, x, B, C, H, IW, D, s, what);
}

int patch_embed_u8(const uint8_t* img, const float* lut, int layout, const uint16_t* W, const float* bias, const float* cls, const float* pos,
                   float* x, int B, int C, int H, int IW, int D, tr_stream_t s, const char* what) {
  TR_REQUIRE(PE_LDS + C * 256 * 4 <= 160 * 1024, TR_ERR_SHAPE, "%s: the pixel LUT of %d channels does not fit beside the ring", what, C);
  TR_REQUIRE(layout == TR_LAYOUT_NCHW || C == 1 || C == 3, TR_ERR_SHAPE, "%s: NHWC needs 1 or 3 channels (C=%d)", what, C);
  TR_REQUIRE(tr_aligned16(img) && tr_aligned16(lut) && tr_aligned16(W) && tr_aligned16(bias) && tr_aligned16(cls) && tr_aligned16(pos) &&
                 tr_aligned16(x),
             TR_ERR_ALIGN, "%s: pointers must be 16-byte aligned", what);
  if (layout == TR_LAYOUT_NCHW || C == 1)        // one channel: NHWC and NCHW are the same bytes
    return launch_patch_embed<PE_U8_NCHW>(img, lut, W, bias, cls, pos, x, B, C, H, IW, D, s, what);
  return launch_patch_embed<PE_U8_NHWC3>(img, lut, W, bias, cls, pos, x, B, C, H, IW, D, s, what);
}

}  // namespace

extern "C" int tr_patch_embed_bf16(const float* img, const uint16_t* W, const float* bias, const float* cls, const float* pos, float* x, int B,
                                   int C, int HW, int patch, int D, tr_stream_t s) {
  TR_REQUIRE(img && W && bias && cls && pos && x, TR_ERR_NULL, "tr_patch_embed_bf16: null pointer");
  TR_REQUIRE(B > 0 && tr_patch_embed_supported(C, HW, patch, D), TR_ERR_SHAPE,
             "tr_patch_embed_bf16: need patch 16, H = W a multiple of 16, embed_dim a multiple of %d (C=%d HW=%d patch=%d D=%d)", PE_NC, C, HW, patch, D);
  return patch_embed_f32(img, W, bias, cls, pos, x, B, C, HW, HW, D, s, "tr_patch_embed_bf16");
}

extern "C" int tr_patch_embed_hw_bf16(const float* img, const uint16_t* W, const float* bias, const float* cls, const float* pos, float* x, int B,
                                      int C, int H, int IW, int patch, int D, tr_stream_t s) {
  TR_REQUIRE(img && W && bias && cls && pos && x, TR_ERR_NULL, "tr_patch_embed_hw_bf16: null pointer");
  TR_REQUIRE(B > 0 && tr_patch_embed_hw_supported(C, H, IW, patch, D), TR_ERR_SHAPE,
             "tr_patch_embed_hw_bf16: need patch 16, H and W multiples of 16, embed_dim a multiple of %d (C=%d H=%d W=%d patch=%d D=%d)", PE_NC, C, H,
             IW, patch, D);
  return patch_embed_f32(img, W, bias, cls, pos, x, B, C, H, IW, D, s, "tr_patch_embed_hw_bf16");
}

extern "C" int tr_patch_embed_u8_bf16(const uint8_t* img, const float* lut, int layout, const uint16_t* W, const float* bias, const float* cls,
                                      const float* pos, float* x, int B, int C, int HW, int patch, int D, tr_stream_t s) {
  TR_REQUIRE(img && lut && W && bias && cls && pos && x, TR_ERR_NULL, "tr_patch_embed_u8_bf16: null pointer");
  TR_REQUIRE(layout == TR_LAYOUT_NCHW || layout == TR_LAYOUT_NHWC, TR_ERR_SHAPE,
             "tr_patch_embed_u8_bf16: layout %d is neither NCHW (0) nor NHWC (1)", layout);
  TR_REQUIRE(B > 0 && tr_patch_embed_supported(C, HW, patch, D), TR_ERR_SHAPE,
             "tr_patch_embed_u8_bf16: need patch 16, H = W a multiple of 16, embed_dim a multiple of %d (C=%d HW=%d patch=%d D=%d)", PE_NC, C, HW,
             patch, D);
  return patch_embed_u8(img, lut, layout, W, bias, cls, pos, x, B, C, HW, HW, D, s, "tr_patch_embed_u8_bf16");
}

extern "C" int tr_patch_embed_u8_hw_bf16(const uint8_t* img, const float* lut, int layout, const uint16_t* W, const float* bias, const float* cls,
                                         const float* pos, float* x, int B, int C, int H, int IW, int patch, int D, tr_stream_t s) {
  TR_REQUIRE(img && lut && W && bias && cls && pos && x, TR_ERR_NULL, "tr_patch_embed_u8_hw_bf16: null pointer");
  TR_REQUIRE(layout == TR_LAYOUT_NCHW || layout == TR_LAYOUT_NHWC, TR_ERR_SHAPE,
             "tr_patch_embed_u8_hw_bf16: layout %d is neither NCHW (0) nor NHWC (1)", layout);
  TR_REQUIRE(B > 0 && tr_patch_embed_hw_supported(C, H, IW, patch, D), TR_ERR_SHAPE,
             "tr_patch_embed_u8_hw_bf16: need patch 16, H and W multiples of 16, embed_dim a multiple of %d (C=%d H=%d W=%d patch=%d D=%d)", PE_NC, C,
             H, IW, patch, D);
  return patch_embed_u8(img, lut, layout, W, bias, cls, pos, x, B, C, H, IW, D, s, "tr_patch_embed_u8_hw_bf16");
}

// ---- PatchEmbed data gradient: d image = fold(dY . W) --------------------------------------------------------------------------------
// The gradient of timm's PatchEmbed (a stride-16 Conv2d, call sites topk.py:181-186) with respect to its input: for patch (b, py, px)
//   dcols[(b, py, px), (c, iy, ix)] = sum_k dY[(b, py, px), k] * W[k, (c, iy, ix)]     ->     dx[b, c, 16 py + iy, 16 px + ix]
// dY = the bf16 gradient of the embedded patch tokens (token rows: the CLS row of every image is skipped and never read), Wt = the patch
// weight transposed [C*256, D], so both MFMA operands are K-contiguous.  Patches do not overlap: every element of dx is written exactly once
// (no memset, no atomics), and the fold is only a choice of store address.
//   The MFMA's A operand is 16 rows of Wt = the 16 ix of one (c, iy); its B operand 16 consecutive patches px of one patch row py.  A lane
// (li, g) then holds ix 4 g .. 4 g + 3 of patch li: one 16-byte store, and the wave's 64 stores are one run of up to 1024 contiguous bytes of
// image row 16 py + iy -- no staging through the LDS.  A workgroup (4 waves) takes one channel and R "units" (a unit = 16 patches of one
// patch row of one image); wave w computes iy = 4 w .. 4 w + 3 for all of them.  The units' dY fragments stay in registers for the whole
// of K (R * D / 8 VGPRs), the Wt fragments stream through L2 / L1 and each feeds R MFMAs.  The launch is bounded by its fp32 output
// (batch 256 at 224 x 224: 154 MB against 30 GFLOP); fp32 accumulation in one fixed K order: the same bits run after run.
namespace {

template <int NK, int R>      // NK = D / 32 K-steps; R units per workgroup
__global__ __launch_bounds__(256) void patch_embed_dgrad_kernel(const uint16_t* __restrict__ dY, long ldy, const uint16_t* __restrict__ Wt,
                                                                float* __restrict__ dx, int C, int H, int IW, int gw, int P, int nb, int units) {
  constexpr int D = NK * 32;
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = blockIdx.y;
  const int u0 = blockIdx.x * R;
  bf16x8 yf[R][NK];
  size_t obase[R];
  bool live[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int u = min(u0 + r, units - 1);                    // past the last unit: reads the last one again, stores nothing
    const int upi = (H >> 4) * nb;                           // units of one image: gh patch rows x nb blocks of 16 patches
    const int b = u / upi, rem = u - b * upi;
    const int py = rem / nb, pb = rem - py * nb;
    const int px = pb * 16 + li;
    const uint16_t* row = dY + ((size_t)b * (P + 1) + 1 + (size_t)py * gw + min(px, gw - 1)) * (size_t)ldy + 8 * g;
#pragma unroll
    for (int k = 0; k < NK; ++k) yf[r][k] = *reinterpret_cast<const bf16x8*>(row + 32 * k);
    live[r] = u0 + r < units && px < gw;
    obase[r] = (((size_t)b * C + c) * H + (size_t)py * 16) * IW + (size_t)px * 16 + 4 * g;
  }
#pragma unroll 1
  for (int j = 0; j < 4; ++j) {
    const int iy = wave * 4 + j;
    const uint16_t* wrow = Wt + ((size_t)c * 256 + iy * 16 + li) * D + 8 * g;
    f32x4 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wrow + 32 * k);
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, yf[r][k], acc[r], 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (live[r]) *reinterpret_cast<f32x4*>(dx + obase[r] + (size_t)iy * IW) = acc[r];
  }
}

template <int NK, int R>
int launch_patch_embed_dgrad(const uint16_t* dY, long ldy, const uint16_t* Wt, float* dx, int B, int C, int H, int IW, tr_stream_t s, const char* what) {
  const int gh = H / 16, gw = IW / 16, P = gh * gw, nb = (gw + 15) / 16, units = B * gh * nb;
  tr_prof_note("patch_embed_dgrad_kernel", 2.0 * B * P * (double)(NK * 32) * C * 256,
               (double)B * C * H * IW * 4.0 + (double)B * P * (NK * 32) * 2.0 + (double)C * 256 * (NK * 32) * 2.0);
  hipLaunchKernelGGL((patch_embed_dgrad_kernel<NK, R>), dim3((units + R - 1) / R, C), dim3(256), 0, static_cast<hipStream_t>(s), dY, ldy, Wt, dx, C,
                     H, IW, gw, P, nb, units);
  TR_CHECK_LAUNCH(what);
  return TR_OK;
}

}  // namespace

// 1 when tr_patch_embed_dgrad_hw takes this shape: patch 16, H and W multiples of 16 (up to 4096), 1 or 3 channels, embed_dim 128 / 192 / 384 / 768
extern "C" int tr_patch_embed_dgrad_hw_supported(int C, int H, int W, int patch, int D) {
  return patch == 16 && H > 0 && H % 16 == 0 && H <= 4096 && W > 0 && W % 16 == 0 && W <= 4096 && (C == 1 || C == 3) &&
         (D == 128 || D == 192 || D == 384 || D == 768);
}

// the square form: H = W = HW
extern "C" int tr_patch_embed_dgrad_supported(int C, int HW, int patch, int D) {
  return patch == 16 && HW > 0 && HW % 16 == 0 && HW <= 4096 && (C == 1 || C == 3) && (D == 128 || D == 192 || D == 384 || D == 768);
}

namespace {

int patch_embed_dgrad(const uint16_t* dY, long ldy, const uint16_t* Wt, float* dx, int B, int C, int H, int IW, int D, tr_stream_t s,
                      const char* what) {
  TR_REQUIRE((size_t)B * (H / 16) * ((IW / 16 + 15) / 16) < ((size_t)1 << 30), TR_ERR_SHAPE, "%s: batch %d beyond the launch grid", what, B);
  TR_REQUIRE(tr_aligned16(dY) && tr_aligned16(Wt) && tr_aligned16(dx) && ldy % 8 == 0, TR_ERR_ALIGN,
             "%s: pointers and the row stride of dY must be 16-byte aligned", what);
  switch (D) {
    case 128: return launch_patch_embed_dgrad<4, 4>(dY, ldy, Wt, dx, B, C, H, IW, s, what);
    case 192: return launch_patch_embed_dgrad<6, 4>(dY, ldy, Wt, dx, B, C, H, IW, s, what);
    case 384: return launch_patch_embed_dgrad<12, 4>(dY, ldy, Wt, dx, B, C, H, IW, s, what);
    default: return launch_patch_embed_dgrad<24, 2>(dY, ldy, Wt, dx, B, C, H, IW, s, what);
  }
}

}  // namespace

extern "C" int tr_patch_embed_dgrad(const uint16_t* dY, long ldy, const uint16_t* Wt, float* dx, int B, int C, int HW, int patch, int D,
                                    tr_stream_t s) {
  TR_REQUIRE(dY && Wt && dx, TR_ERR_NULL, "tr_patch_embed_dgrad: null pointer");
  TR_REQUIRE(B > 0 && tr_patch_embed_dgrad_supported(C, HW, patch, D) && ldy >= D, TR_ERR_SHAPE,
             "tr_patch_embed_dgrad: need patch 16, H = W a multiple of 16, 1 or 3 channels, embed_dim 128 / 192 / 384 / 768, ldy >= embed_dim "
             "(C=%d HW=%d patch=%d D=%d ldy=%ld)", C, HW, patch, D, ldy);
  return patch_embed_dgrad(dY, ldy, Wt, dx, B, C, HW, HW, D, s, "tr_patch_embed_dgrad");
}

extern "C" int tr_patch_embed_dgrad_hw(const uint16_t* dY, long ldy, const uint16_t* Wt, float* dx, int B, int C, int H, int IW, int patch, int D,
                                       tr_stream_t s) {
  TR_REQUIRE(dY && Wt && dx, TR_ERR_NULL, "tr_patch_embed_dgrad_hw: null pointer");
  TR_REQUIRE(B > 0 && tr_patch_embed_dgrad_hw_supported(C, H, IW, patch, D) && ldy >= D, TR_ERR_SHAPE,
             "tr_patch_embed_dgrad_hw: need patch 16, H and W multiples of 16, 1 or 3 channels, embed_dim 128 / 192 / 384 / 768, ldy >= embed_dim "
             "(C=%d H=%d W=%d patch=%d D=%d ldy=%ld)", C, H, IW, patch, D, ldy);
  return patch_embed_dgrad(dY, ldy, Wt, dx, B, C, H, IW, D, s, "tr_patch_embed_dgrad_hw");
}
