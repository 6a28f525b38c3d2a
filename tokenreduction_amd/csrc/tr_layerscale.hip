// LayerScale (timm's init_values; DeiT-III): x = x + gamma_1 * attn(norm1(x)), x = x + gamma_2 * mlp(norm2(x)), one [D] vector per branch.
// The executor has no gamma: the scale folds exactly into the Linear that ends the branch,
//   gamma o (W h + b) = (diag(gamma) W) h + gamma o b
// so it reads FOLDED operands W' = fl32(gamma[d] * W[d,k]), b' = fl32(gamma[d] * b[d]) and produces gradients dW', db' for them, from
// which the gradients of the real parameters follow:
//   dW[d,k] = gamma[d] * dW'[d,k]     db[d] = gamma[d] * db'[d]     dgamma[d] = sum_k dW'[d,k] * W[d,k] + db'[d] * b[d]
//
//   tr_layerscale_fold          every folded matrix of a model in ONE launch: per 64 x 64 tile read W (fp32), scale the rows, write the operand
//                               copy (bf16 -- the product rounded to nearest-even, as tr_cast_pack_bf16 rounds -- or fp32), its transposed bf16
//                               copy through an LDS tile (both global sides coalesced), and the folded bias.
//   tr_layerscale_unfold_grad   every folded gradient of a backward call in ONE launch: a wave owns a row -- its lanes stride the row with 16-byte
//                               accesses (dW' read once, W read once, dW written once), the partial sums of dgamma meet in a butterfly over the
//                               wave.  The order of the additions behind a dgamma is a function of `cols` alone; no atomics.
// Both are memory-bound: 16-byte loads and stores throughout.  rows and cols are multiples of 64 (every model the planner accepts).
//
// The library is built with -ffp-contract=fast, under which the compiler may fuse a product into a following addition whatever intrinsic
// spelled it.  The products here must be ROUNDED fp32 products (the bits of a torch fp32 multiply; two roundings under `accumulate`), so
// each one passes through an empty asm statement that the optimizer cannot look through.
#include "tr_common.h"

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) {
  float t = __fmul_rn(a, b);
  asm volatile("" : "+v"(t));
  return t;
}

// the item a workgroup belongs to: binary search over the items' first workgroup
template <class Item>
__device__ __forceinline__ int find_item(const Item* __restrict__ items, int n_items) {
  int lo = 0, hi = n_items;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (items[mid].first <= (int)blockIdx.x) lo = mid; else hi = mid;
  }
  return lo;
}

// one 64 x 64 tile per workgroup: 8 column groups of 8 x 32 rows, two row passes
template <bool F32>
__global__ __launch_bounds__(256) void ls_fold_kernel(const tr_ls_fold_item* __restrict__ items, int n_items) {
  __shared__ unsigned short tile[64][66];
  const tr_ls_fold_item I = items[find_item(items, n_items)];
  const int tiles_c = I.cols >> 6;
  const int t = blockIdx.x - I.first, r0 = (t / tiles_c) << 6, c0 = (t % tiles_c) << 6;
  const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
  const float* W = static_cast<const float*>(I.w);
  const float* gam = static_cast<const float*>(I.gamma);
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int r = r0 + ty + 32 * p, c = c0 + 8 * tx;
    const size_t o = (size_t)r * I.cols + c;
    const float g = gam[r];
    const float4 a = *reinterpret_cast<const float4*>(W + o), b = *reinterpret_cast<const float4*>(W + o + 4);
    const float v[8] = {mul_rn(g, a.x), mul_rn(g, a.y), mul_rn(g, a.z), mul_rn(g, a.w), mul_rn(g, b.x), mul_rn(g, b.y), mul_rn(g, b.z), mul_rn(g, b.w)};
    if (F32 && I.dst != nullptr) {
      float* d = static_cast<float*>(I.dst) + o;
      *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    if ((!F32 && I.dst != nullptr) || I.dst_t != nullptr) {
      const uint4 q = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
      if (!F32 && I.dst != nullptr) *reinterpret_cast<uint4*>(static_cast<uint16_t*>(I.dst) + o) = q;
      if (I.dst_t != nullptr) {
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          tile[ty + 32 * p][8 * tx + 2 * e] = (unsigned short)(w[e] & 0xffffu);
          tile[ty + 32 * p][8 * tx + 2 * e + 1] = (unsigned short)(w[e] >> 16);
        }
      }
    }
  }
  if (c0 == 0 && I.b_dst != nullptr && threadIdx.x < 64) {        // the folded bias: the first tile of every row band
    const int r = r0 + threadIdx.x;
    static_cast<float*>(I.b_dst)[r] = mul_rn(gam[r], static_cast<const float*>(I.b)[r]);
  }
  if (I.dst_t == nullptr) return;
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int c = ty + 32 * p, r = 8 * tx;                         // transposed: row c0 + c of dst_t, columns r0 + r .. r0 + r + 7
    unsigned w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = (unsigned)tile[r + 2 * e][c] | ((unsigned)tile[r + 2 * e + 1][c] << 16);
    *reinterpret_cast<uint4*>(static_cast<uint16_t*>(I.dst_t) + (size_t)(c0 + c) * I.rows + r0 + r) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// four rows per workgroup, one per wave; lane l takes the float4 at columns 4 l, 4 l + 256, ...
__global__ __launch_bounds__(256) void ls_unfold_kernel(const tr_ls_unfold_item* __restrict__ items, int n_items, int accumulate) {
  const tr_ls_unfold_item I = items[find_item(items, n_items)];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = ((blockIdx.x - I.first) << 2) + wave;
  const size_t o = (size_t)r * I.cols;
  const float g = static_cast<const float*>(I.gamma)[r];
  const float* X = static_cast<const float*>(I.dw_f) + o;
  const float* W = static_cast<const float*>(I.w) + o;
  float* dW = I.dw != nullptr ? static_cast<float*>(I.dw) + o : nullptr;
  const bool want_g = I.dgamma != nullptr;
  float acc = 0.f;
  if (want_g || dW != nullptr) {
    for (int k = 4 * lane; k < I.cols; k += 256) {
      const float4 x = *reinterpret_cast<const float4*>(X + k);
      if (want_g) {
        const float4 w = *reinterpret_cast<const float4*>(W + k);
        acc = fmaf(x.x, w.x, acc); acc = fmaf(x.y, w.y, acc); acc = fmaf(x.z, w.z, acc); acc = fmaf(x.w, w.w, acc);
      }
      if (dW != nullptr) {
        float4 v = make_float4(mul_rn(g, x.x), mul_rn(g, x.y), mul_rn(g, x.z), mul_rn(g, x.w));
        if (accumulate) {
          const float4 old = *reinterpret_cast<const float4*>(dW + k);
          v = make_float4(__fadd_rn(old.x, v.x), __fadd_rn(old.y, v.y), __fadd_rn(old.z, v.z), __fadd_rn(old.w, v.w));
        }
        *reinterpret_cast<float4*>(dW + k) = v;
      }
    }
  }
  if (want_g) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);      // butterfly: the same order in every lane, on every launch
  }
  if (lane != 0) return;
  const float xb = static_cast<const float*>(I.db_f)[r];
  if (I.db != nullptr) {
    float* db = static_cast<float*>(I.db) + r;
    const float v = mul_rn(g, xb);
    *db = accumulate ? __fadd_rn(*db, v) : v;
  }
  if (want_g) {
    float* dg = static_cast<float*>(I.dgamma) + r;
    const float v = fmaf(xb, static_cast<const float*>(I.b)[r], acc);
    *dg = accumulate ? *dg + v : v;
  }
}

// the host's half of a call: the shapes (the item table itself is on the device) -> workgroups, bytes
bool check_shapes(const int* shapes, int n_items) {
  for (int i = 0; i < n_items; ++i)
    if (shapes[2 * i] <= 0 || shapes[2 * i + 1] <= 0 || shapes[2 * i] % 64 != 0 || shapes[2 * i + 1] % 64 != 0) return false;
  return true;
}

}  // namespace

extern "C" int tr_layerscale_fold(const tr_ls_fold_item* items, const int* shapes, int n_items, int dst_is_f32, tr_stream_t s) {
  TR_REQUIRE(items && shapes, TR_ERR_NULL, "tr_layerscale_fold: null pointer");
  TR_REQUIRE(n_items > 0, TR_ERR_SHAPE, "tr_layerscale_fold: nothing to fold (n_items=%d)", n_items);
  TR_REQUIRE(check_shapes(shapes, n_items), TR_ERR_SHAPE, "tr_layerscale_fold: rows and cols must be positive multiples of 64");
  TR_REQUIRE(tr_aligned16(items), TR_ERR_ALIGN, "tr_layerscale_fold: the item table must be 16-byte aligned");
  long tiles = 0;
  double elems = 0.0, rows = 0.0;
  for (int i = 0; i < n_items; ++i) {
    tiles += (long)(shapes[2 * i] / 64) * (shapes[2 * i + 1] / 64);
    elems += (double)shapes[2 * i] * shapes[2 * i + 1];
    rows += shapes[2 * i];
  }
  TR_REQUIRE(tiles < (1L << 31), TR_ERR_SHAPE, "tr_layerscale_fold: too many tiles (%ld)", tiles);
  // (bytes: the fp32 source, the operand copy and -- counted as present -- its transposed bf16 copy)
  tr_prof_note("tr_layerscale_fold", elems, elems * (4.0 + (dst_is_f32 ? 4.0 : 2.0) + 2.0) + rows * 12.0);
  if (dst_is_f32) hipLaunchKernelGGL(ls_fold_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, static_cast<hipStream_t>(s), items, n_items);
  else hipLaunchKernelGGL(ls_fold_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, static_cast<hipStream_t>(s), items, n_items);
  TR_CHECK_LAUNCH("tr_layerscale_fold");
  return TR_OK;
}

extern "C" int tr_layerscale_unfold_grad(const tr_ls_unfold_item* items, const int* shapes, int n_items, int accumulate, tr_stream_t s) {
  TR_REQUIRE(items && shapes, TR_ERR_NULL, "tr_layerscale_unfold_grad: null pointer");
  TR_REQUIRE(n_items > 0, TR_ERR_SHAPE, "tr_layerscale_unfold_grad: nothing to unfold (n_items=%d)", n_items);
  TR_REQUIRE(check_shapes(shapes, n_items), TR_ERR_SHAPE, "tr_layerscale_unfold_grad: rows and cols must be positive multiples of 64");
  TR_REQUIRE(tr_aligned16(items), TR_ERR_ALIGN, "tr_layerscale_unfold_grad: the item table must be 16-byte aligned");
  long groups = 0;
  double elems = 0.0;
  for (int i = 0; i < n_items; ++i) {
    groups += shapes[2 * i] / 4;
    elems += (double)shapes[2 * i] * shapes[2 * i + 1];
  }
  TR_REQUIRE(groups < (1L << 31), TR_ERR_SHAPE, "tr_layerscale_unfold_grad: too many rows (%ld groups)", groups);
  // (bytes with every output present: dW' and W read, dW written -- and read under accumulate)
  tr_prof_note("tr_layerscale_unfold_grad", 3.0 * elems, elems * (accumulate ? 16.0 : 12.0));
  hipLaunchKernelGGL(ls_unfold_kernel, dim3((unsigned)groups), dim3(256), 0, static_cast<hipStream_t>(s), items, n_items, accumulate ? 1 : 0);
  TR_CHECK_LAUNCH("tr_layerscale_unfold_grad");
  return TR_OK;
}
