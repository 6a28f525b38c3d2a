// Output taps of the eval executor (tr_vit_forward_taps): rows of the residual stream a caller asked for, written while the forward runs.
//   tr_cls_tap            the CLS row of every image after a block: x + the residuals still pending there, fp32, B rows of D
//                         (what viz_data["Features"][blk][:, 0] holds: deit_viz.py:199, topk.py:197)
//   tr_final_tokens_f32   norm(x) of EVERY row after the last block, fp32 (the DyViT teacher's second output, dyvit.py:325-334):
//                         the residual add(s) and the fp32 LayerNorm in one pass
//   tr_level_tap_norm     both of them for one row read: the summed row AND its fp32 final norm, two stores (the level taps of the
//                         training forward, tr_vit_forward_train_levels: the backward of the norm needs the row that entered it)
// All are HBM-bound row kernels in the shape of tr_norm.hip: one wave per row, 16-byte accesses, D <= 1024.  The additions are those of
// tr_residual_snapshot behind an eager norm2 -- (x + first) + second in fp32 -- and the normalisation is tr_layernorm_f32's (ln_row_store<true>),
// so the values equal that two-launch sequence bit for bit.
#include "tr_common.h"
#include "tr_rowops.h"

namespace {

// v[c] += d[row] for the chunks of one row, all loads in one batch (chunk index clamped, like layernorm_kernel)
template <bool DF32, int NCH>
__device__ __forceinline__ void add_pending(float4 (&v)[NCH], const void* __restrict__ d, size_t row_off, int lane, int nchunks) {
  float4 t[NCH];
#pragma unroll
  for (int c = 0; c < NCH; ++c) t[c] = load_delta4<DF32>(d, row_off + 4 * min(lane + 64 * c, nchunks - 1));
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    v[c].x += t[c].x; v[c].y += t[c].y; v[c].z += t[c].z; v[c].w += t[c].w;
  }
}

// (x[row] + d1[row]) + d2[row] in registers: the one summation of every kernel here.  NT: the stream is not read again in this forward
template <bool DF32, int NCH, bool NT>
__device__ __forceinline__ void summed_row(float4 (&v)[NCH], const float* __restrict__ xr, const void* __restrict__ d1, size_t off1,
                                           const void* __restrict__ d2, size_t off2, int lane, int nchunks) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    const float* p = xr + 4 * min(lane + 64 * c, nchunks - 1);
    v[c] = NT ? ln_nt_load4(p) : *reinterpret_cast<const float4*>(p);
  }
  if (d1 != nullptr) add_pending<DF32, NCH>(v, d1, off1, lane, nchunks);
  if (d2 != nullptr) add_pending<DF32, NCH>(v, d2, off2, lane, nchunks);
}
template <int NCH>
__device__ __forceinline__ void store_row(const float4 (&v)[NCH], float* __restrict__ orow, int lane, int nchunks) {
#pragma unroll
  for (int c = 0; c < NCH; ++c)
    if (lane + 64 * c < nchunks) *reinterpret_cast<float4*>(orow + 4 * (lane + 64 * c)) = v[c];
}

// out[b] = (x[b] + d1[b]) + d2[b]: B rows at their own strides (the stream's CLS rows at N * D, compact CLS-tail buffers at D,
// the destination at n_blocks * D); d1 / d2 nullable
template <bool DF32, int NCH>
__global__ __launch_bounds__(256) void cls_tap_kernel(const float* __restrict__ x, long ldx, const void* __restrict__ d1, long ld1,
                                                      const void* __restrict__ d2, long ld2, float* __restrict__ out, long ldo, int B,
                                                      int D) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const int nchunks = D >> 2;
  float4 v[NCH];
  summed_row<DF32, NCH, false>(v, x + (size_t)row * ldx, d1, (size_t)row * ld1, d2, (size_t)row * ld2, lane, nchunks);
  store_row<NCH>(v, out + (size_t)row * ldo, lane, nchunks);
}

// y[row] = LayerNorm_f32((x[row] + d1[row]) + d2[row]) over contiguous rows [M, D]; nothing is written back to x.  The stream and the
// residuals are read once and not again in this forward: nontemporal loads, like the norms
template <bool DF32, int NCH>
__global__ __launch_bounds__(256) void final_tokens_kernel(const float* __restrict__ x, const void* __restrict__ d1,
                                                           const void* __restrict__ d2, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ y, int M, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nchunks = D >> 2;
  float4 v[NCH];
  summed_row<DF32, NCH, true>(v, x + (size_t)row * D, d1, (size_t)row * D, d2, (size_t)row * D, lane, nchunks);
  ln_row_store<true, NCH>(v, nchunks, lane, D, eps, gamma, beta, y + (size_t)row * D);
}

// sum[row] = (x[row] + d1[row]) + d2[row] and y[row] = LayerNorm_f32(sum[row]) over contiguous rows [M, D]: cls_tap_kernel's row at stride D and
// final_tokens_kernel's row from ONE read of x and the pending operands.  x is read again by the next norm of a training forward: plain loads
template <bool DF32, int NCH>
__global__ __launch_bounds__(256) void level_tap_norm_kernel(const float* __restrict__ x, const void* __restrict__ d1,
                                                             const void* __restrict__ d2, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ sum, float* __restrict__ y, int M,
                                                             int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nchunks = D >> 2;
  float4 v[NCH];
  summed_row<DF32, NCH, false>(v, x + (size_t)row * D, d1, (size_t)row * D, d2, (size_t)row * D, lane, nchunks);
  store_row<NCH>(v, sum + (size_t)row * D, lane, nchunks);
  ln_row_store<true, NCH>(v, nchunks, lane, D, eps, gamma, beta, y + (size_t)row * D);
}

// a pending operand: fp32 rows need 16-byte, bf16 rows 8-byte alignment of the base and of every row
inline bool operand_ok(const void* d, long ld, int D, bool f32) {
  if (d == nullptr) return true;
  return ld >= D && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(d) & (f32 ? 15u : 7u)) == 0;
}

}  // namespace

extern "C" int tr_cls_tap(const float* x, long ldx, const void* d1, long ld1, const void* d2, long ld2, int delta_is_f32, float* out, long ldo,
                          int B, int D, tr_stream_t s) {
  TR_REQUIRE(x && out, TR_ERR_NULL, "tr_cls_tap: null pointer");
  TR_REQUIRE(d1 != nullptr || d2 == nullptr, TR_ERR_NULL, "tr_cls_tap: a second pending operand needs the first");
  TR_REQUIRE(B > 0 && D > 0 && D % 4 == 0 && D <= 256 * LN_MAX_CHUNKS && ldx % 4 == 0 && ldx >= D && ldo % 4 == 0 && ldo >= D, TR_ERR_SHAPE,
             "tr_cls_tap: need D %% 4 == 0, D <= 1024, strides %% 4 == 0 and >= D (B=%d D=%d ldx=%ld ldo=%ld)", B, D, ldx, ldo);
  const bool f32 = delta_is_f32 != 0;
  TR_REQUIRE(operand_ok(d1, ld1, D, f32) && operand_ok(d2, ld2, D, f32), TR_ERR_SHAPE, "tr_cls_tap: bad pending operand (ld1=%ld ld2=%ld)", ld1,
             ld2);
  TR_REQUIRE(tr_aligned16(x) && tr_aligned16(out), TR_ERR_ALIGN, "tr_cls_tap: pointers must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(s);
  tr_prof_note("tr_cls_tap", 0.0, (double)B * D * (8.0 + ((d1 ? 1.0 : 0.0) + (d2 ? 1.0 : 0.0)) * (f32 ? 4.0 : 2.0)));
  if (f32) TR_DISPATCH_NCH(D, hipLaunchKernelGGL((cls_tap_kernel<true, NCH>), dim3((B + 3) / 4), dim3(256), 0, st, x, ldx, d1, ld1, d2, ld2, out, ldo, B, D));
  else TR_DISPATCH_NCH(D, hipLaunchKernelGGL((cls_tap_kernel<false, NCH>), dim3((B + 3) / 4), dim3(256), 0, st, x, ldx, d1, ld1, d2, ld2, out, ldo, B, D));
  TR_CHECK_LAUNCH("tr_cls_tap");
  return TR_OK;
}

extern "C" int tr_final_tokens_f32(const float* x, const void* d1, const void* d2, int delta_is_f32, const float* gamma, const float* beta,
                                   float* y, int M, int D, float eps, tr_stream_t s) {
  TR_REQUIRE(x && gamma && beta && y, TR_ERR_NULL, "tr_final_tokens_f32: null pointer");
  TR_REQUIRE(d1 != nullptr || d2 == nullptr, TR_ERR_NULL, "tr_final_tokens_f32: a second pending operand needs the first");
  TR_REQUIRE(M > 0 && D > 0 && D % 4 == 0 && D <= 256 * LN_MAX_CHUNKS, TR_ERR_SHAPE, "tr_final_tokens_f32: need D %% 4 == 0, D <= 1024 (M=%d D=%d)", M,
             D);
  const bool f32 = delta_is_f32 != 0;
  TR_REQUIRE(operand_ok(d1, D, D, f32) && operand_ok(d2, D, D, f32), TR_ERR_ALIGN, "tr_final_tokens_f32: misaligned pending operand");
  TR_REQUIRE(tr_aligned16(x) && tr_aligned16(gamma) && tr_aligned16(beta) && tr_aligned16(y), TR_ERR_ALIGN,
             "tr_final_tokens_f32: pointers must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(s);
  tr_prof_note("tr_final_tokens", 0.0, (double)M * D * (8.0 + ((d1 ? 1.0 : 0.0) + (d2 ? 1.0 : 0.0)) * (f32 ? 4.0 : 2.0)));
  if (f32) TR_DISPATCH_NCH(D, hipLaunchKernelGGL((final_tokens_kernel<true, NCH>), dim3((M + 3) / 4), dim3(256), 0, st, x, d1, d2, gamma, beta, y, M, D, eps));
  else TR_DISPATCH_NCH(D, hipLaunchKernelGGL((final_tokens_kernel<false, NCH>), dim3((M + 3) / 4), dim3(256), 0, st, x, d1, d2, gamma, beta, y, M, D, eps));
  TR_CHECK_LAUNCH("tr_final_tokens_f32");
  return TR_OK;
}

extern "C" int tr_level_tap_norm(const float* x, const void* d1, const void* d2, int delta_is_f32, const float* gamma, const float* beta,
                                 float* sum, float* y, int M, int D, float eps, tr_stream_t s) {
  TR_REQUIRE(x && gamma && beta && sum && y, TR_ERR_NULL, "tr_level_tap_norm: null pointer");
  TR_REQUIRE(d1 != nullptr || d2 == nullptr, TR_ERR_NULL, "tr_level_tap_norm: a second pending operand needs the first");
  TR_REQUIRE(M > 0 && D > 0 && D % 4 == 0 && D <= 256 * LN_MAX_CHUNKS, TR_ERR_SHAPE, "tr_level_tap_norm: need D %% 4 == 0, D <= 1024 (M=%d D=%d)", M, D);
  const bool f32 = delta_is_f32 != 0;
  TR_REQUIRE(operand_ok(d1, D, D, f32) && operand_ok(d2, D, D, f32), TR_ERR_ALIGN, "tr_level_tap_norm: misaligned pending operand");
  TR_REQUIRE(tr_aligned16(x) && tr_aligned16(gamma) && tr_aligned16(beta) && tr_aligned16(sum) && tr_aligned16(y), TR_ERR_ALIGN,
             "tr_level_tap_norm: pointers must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(s);
  tr_prof_note("tr_level_tap_norm", 0.0, (double)M * D * (12.0 + ((d1 ? 1.0 : 0.0) + (d2 ? 1.0 : 0.0)) * (f32 ? 4.0 : 2.0)));
  if (f32) TR_DISPATCH_NCH(D, hipLaunchKernelGGL((level_tap_norm_kernel<true, NCH>), dim3((M + 3) / 4), dim3(256), 0, st, x, d1, d2, gamma, beta, sum, y, M, D, eps));
  else TR_DISPATCH_NCH(D, hipLaunchKernelGGL((level_tap_norm_kernel<false, NCH>), dim3((M + 3) / 4), dim3(256), 0, st, x, d1, d2, gamma, beta, sum, y, M, D, eps));
  TR_CHECK_LAUNCH("tr_level_tap_norm");
  return TR_OK;
}
