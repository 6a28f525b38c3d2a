// Average-pooled head (tr_vit_config.global_pool == 1): the weighted mean of the patch tokens after the last block, and its backward.
//   tr_token_pool       out[b] = sum_n w[b,n] * ((x[b,n] + d1[b,n]) + d2[b,n]) / sum_n w[b,n],  n = 1 .. N-1 (row 0, the CLS token, is left out)
//   tr_token_pool_bwd   g[b,n] = gpool[b] * (w[b,n] / sum_n w[b,n]), g[b,0] = 0: every element of g written once
// timm's global_pool='avg' with fc_norm (the MAE fine-tuning head): the pool runs BEFORE the final norm, on the stream with its pending
// residuals added in the reference's order.  w: ToMe token sizes / the ATS padding mask [B,N] (entry 0 unused); NULL = all ones.
//
// The forward is an HBM-bound column reduction: a workgroup owns one image and one slab of 8 * TX columns, its POOL_RG row groups
// stride through the rows (row n belongs to group (n - 1) % POOL_RG), every lane keeps 8 columns in registers -- two 16-byte loads of the
// stream, one (bf16) or two (fp32) of each pending operand, each byte read once.  The partial sums of the row groups meet in LDS and are
// added in group order by one lane per column.  The order of the additions behind an output element is therefore a function of N alone: not
// of B, not of the slab width the launch picked (small batches take narrower slabs so that B * D / (8 * TX) workgroups still cover the
// chip), not of scheduling.  No atomics.
#include "tr_common.h"
#include "tr_rowops.h"

namespace {

constexpr int POOL_RG = 32;        // row groups of a workgroup: fixed -- it is part of the summation order

// eight consecutive columns of a pending operand
template <bool DF32>
__device__ __forceinline__ void load_delta8(const void* base, size_t elem, float (&t)[8]) {
  if (DF32) {
    const float* p = reinterpret_cast<const float*>(base) + elem;
    const float4 a = ln_nt_load4(p), b = ln_nt_load4(p + 4);
    t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w; t[4] = b.x; t[5] = b.y; t[6] = b.z; t[7] = b.w;
  } else {
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    const u32x4 u = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(base) + elem));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      t[2 * i] = __builtin_bit_cast(float, u[i] << 16);
      t[2 * i + 1] = __builtin_bit_cast(float, u[i] & 0xffff0000u);
    }
  }
}

// the sum of an image's weights over the patch rows, in the order every kernel of this file uses: POOL_RG strided partial sums (lanes
// 0 .. POOL_RG-1 of the workgroup), added in group order.  part: POOL_RG floats of LDS.  The caller's threads all get the sum.
__device__ __forceinline__ float weight_sum(const float* __restrict__ wrow, int N, float* part) {
  if (threadIdx.x < POOL_RG) {
    float a = 0.f;
    for (int n = 1 + threadIdx.x; n < N; n += POOL_RG) a += wrow != nullptr ? wrow[n] : 1.0f;
    part[threadIdx.x] = a;
  }
  __syncthreads();
  float sum = 0.f;
#pragma unroll
  for (int g = 0; g < POOL_RG; ++g) sum += part[g];
  return sum;
}

// grid (D / (8 * TX), B), block POOL_RG * TX: thread = (row group rg, column lane tx)
template <bool DF32, int TX>
__global__ __launch_bounds__(POOL_RG * TX) void token_pool_kernel(const float* __restrict__ x, const void* __restrict__ d1,
                                                                  const void* __restrict__ d2, const float* __restrict__ weight,
                                                                  float* __restrict__ out, int N, int D) {
  __shared__ float part[POOL_RG][8 * TX + 1];
  __shared__ float wpart[POOL_RG];
  const int tx = threadIdx.x % TX, rg = threadIdx.x / TX;
  const int b = blockIdx.y, col = blockIdx.x * 8 * TX + 8 * tx;
  const float* wrow = weight != nullptr ? weight + (size_t)b * N : nullptr;
  float acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] = 0.f;
#pragma unroll 2
  for (int n = 1 + rg; n < N; n += POOL_RG) {
    const size_t off = ((size_t)b * N + n) * D + col;
    const float4 a = ln_nt_load4(x + off), c = ln_nt_load4(x + off + 4);
    float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
    if (d1 != nullptr) {
      float t[8];
      load_delta8<DF32>(d1, off, t);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] += t[i];
    }
    if (d2 != nullptr) {
      float t[8];
      load_delta8<DF32>(d2, off, t);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] += t[i];
    }
    const float w = wrow != nullptr ? wrow[n] : 1.0f;
    if (w != 0.f) {                // a row of weight 0 (ATS padding) adds nothing, whatever it holds
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = fmaf(w, v[i], acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) part[rg][8 * tx + i] = acc[i];
  const float wsum = weight_sum(wrow, N, wpart);        // (its barrier also publishes part)
  if (threadIdx.x < 8 * TX) {
    float sum = 0.f;
#pragma unroll
    for (int g = 0; g < POOL_RG; ++g) sum += part[g][threadIdx.x];
    // an image without weight (every patch row masked) pools to zero
    out[(size_t)b * D + blockIdx.x * 8 * TX + threadIdx.x] = wsum > 0.f ? sum / wsum : 0.f;
  }
}

// grid (ceil(N * D / 4 / 1024), B), block 256: four float4 of g per thread
__global__ __launch_bounds__(256) void token_pool_bwd_kernel(const float* __restrict__ gpool, const float* __restrict__ weight,
                                                             float* __restrict__ g, int N, int D) {
  __shared__ float wpart[POOL_RG];
  const int b = blockIdx.y, dq = D >> 2, total = N * dq;
  const float* wrow = weight != nullptr ? weight + (size_t)b * N : nullptr;
  const float wsum = weight_sum(wrow, N, wpart);
  const float inv = wsum > 0.f ? 1.0f / wsum : 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int e = (blockIdx.x * 4 + k) * 256 + threadIdx.x;
    if (e >= total) break;
    const int n = e / dq, c = e - n * dq;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n > 0) {
      const float coef = (wrow != nullptr ? wrow[n] : 1.0f) * inv;
      const float4 gp = *reinterpret_cast<const float4*>(gpool + (size_t)b * D + 4 * c);
      o = make_float4(gp.x * coef, gp.y * coef, gp.z * coef, gp.w * coef);
    }
    *reinterpret_cast<float4*>(g + ((size_t)b * N + n) * D + 4 * c) = o;
  }
}

template <bool DF32>
void launch_pool(int tx, dim3 grid, hipStream_t st, const float* x, const void* d1, const void* d2, const float* weight, float* out, int N, int D) {
  if (tx == 8) hipLaunchKernelGGL((token_pool_kernel<DF32, 8>), grid, dim3(POOL_RG * 8), 0, st, x, d1, d2, weight, out, N, D);
  else if (tx == 4) hipLaunchKernelGGL((token_pool_kernel<DF32, 4>), grid, dim3(POOL_RG * 4), 0, st, x, d1, d2, weight, out, N, D);
  else hipLaunchKernelGGL((token_pool_kernel<DF32, 2>), grid, dim3(POOL_RG * 2), 0, st, x, d1, d2, weight, out, N, D);
}

}  // namespace

extern "C" int tr_token_pool(const float* x, const void* d1, const void* d2, int delta_is_f32, const float* weight, float* out, int B, int N,
                             int D, tr_stream_t s) {
  TR_REQUIRE(x && out, TR_ERR_NULL, "tr_token_pool: null pointer");
  TR_REQUIRE(d1 != nullptr || d2 == nullptr, TR_ERR_NULL, "tr_token_pool: a second pending operand needs the first");
  TR_REQUIRE(B > 0 && B <= 65535 && N >= 2 && D > 0 && D % 64 == 0, TR_ERR_SHAPE,
             "tr_token_pool: need 1 <= B <= 65535, N >= 2 (CLS + a patch token), D %% 64 == 0 (B=%d N=%d D=%d)", B, N, D);
  TR_REQUIRE(tr_aligned16(x) && tr_aligned16(d1) && tr_aligned16(d2) && tr_aligned16(out), TR_ERR_ALIGN,
             "tr_token_pool: pointers must be 16-byte aligned");
  const bool f32 = delta_is_f32 != 0;
  // slab width: 64 columns where that gives a workgroup to every compute unit, else 32, else 16 (same bits: see the head of the file)
  const long slabs64 = (long)B * (D / 64);
  const int tx = slabs64 >= 256 ? 8 : 2 * slabs64 >= 256 ? 4 : 2;
  const dim3 grid(D / (8 * tx), B);
  hipStream_t st = static_cast<hipStream_t>(s);
  tr_prof_note("tr_token_pool", 2.0 * B * (N - 1) * D,
               (double)B * (N - 1) * D * (4.0 + ((d1 ? 1.0 : 0.0) + (d2 ? 1.0 : 0.0)) * (f32 ? 4.0 : 2.0)) + (double)B * D * 4.0);
  if (f32) launch_pool<true>(tx, grid, st, x, d1, d2, weight, out, N, D);
  else launch_pool<false>(tx, grid, st, x, d1, d2, weight, out, N, D);
  TR_CHECK_LAUNCH("tr_token_pool");
  return TR_OK;
}

extern "C" int tr_token_pool_bwd(const float* gpool, const float* weight, float* g, int B, int N, int D, tr_stream_t s) {
  TR_REQUIRE(gpool && g, TR_ERR_NULL, "tr_token_pool_bwd: null pointer");
  TR_REQUIRE(B > 0 && B <= 65535 && N >= 2 && D > 0 && D % 64 == 0, TR_ERR_SHAPE,
             "tr_token_pool_bwd: need 1 <= B <= 65535, N >= 2, D %% 64 == 0 (B=%d N=%d D=%d)", B, N, D);
  TR_REQUIRE((long)N * (D / 4) < (1L << 31) - 1024, TR_ERR_SHAPE, "tr_token_pool_bwd: N * D too large (N=%d D=%d)", N, D);
  TR_REQUIRE(tr_aligned16(gpool) && tr_aligned16(g), TR_ERR_ALIGN, "tr_token_pool_bwd: pointers must be 16-byte aligned");
  const int total = N * (D / 4);
  tr_prof_note("tr_token_pool_bwd", (double)B * N * D, (double)B * N * D * 4.0 + (double)B * D * 4.0);
  hipLaunchKernelGGL(token_pool_bwd_kernel, dim3((total + 1023) / 1024, B), dim3(256), 0, static_cast<hipStream_t>(s), gpool, weight, g, N, D);
  TR_CHECK_LAUNCH("tr_token_pool_bwd");
  return TR_OK;
}
