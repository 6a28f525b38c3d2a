// Dense feature maps from the reduced token stream: the final-normed rows of an eval forward (the final_tokens tap, fp32 [B, N_last, D]) put
// back on the input's patch grid.
//   tr_dense_index    the record-form decisions of tr_stage_decisions composed across the stages into index[b, p]: the row of the last
//                     stream (1 ... N_last-1, row 0 is the CLS token) that stands for grid patch p, -1 where none does.  One workgroup of
//                     256 threads per image; the state cur[p] (patch-relative row, -1 = lost) and the inverse table of a kept list live in
//                     LDS.  Pure index shuffling; every value is compared with the length of what it is about to index BEFORE the read.
//   tr_dense_gather   features[b, :, p] = tokens[b, index[b, p], :] where 0 <= index < n_rows, `fill` elsewhere; fp32 or bf16 (round to
//                     nearest even) output, channels-last [B, P, D] or NCHW [B, D, P].  Every output element is written exactly once: no
//                     memset in front of it, no atomics.
//   tr_dense_index_levels / tr_dense_gather_levels   the same two steps for L levels (the streams after L chosen blocks, each behind its own
//                     prefix of the stages) in ONE launch each: the index kernel walks the stage table once and writes a level's index where
//                     its prefix ends; the gather's tile order has the level as its slowest coordinate.
//   tr_dense_scatter  the gather's adjoint, for the map's gradient in training: dtokens[b, r, :] = the sum of dmap[b, :, p] over the patches
//                     with index[b, p] == r, fp32 additions in ascending p, every output element written exactly once, no scratch.
//   tr_dense_scatter_levels   the scatter for L levels (the adjoint of tr_dense_gather_levels) in ONE launch: the maps' gradients arrive as L
//                     separate tensors, a NULL one is a level without a gradient and owns no tile; the tile bodies are tr_dense_scatter's.
// The gather is the hot path: it writes the largest tensor of the forward once and reads at most as much.  Channels-last is a row copy in
// the shape of tr_taps.hip (a wave per output row, 16-byte loads).  NCHW transposes a tile of 64 patches x 64 channels through LDS: rows
// come in with 16-byte loads (a 256-byte piece of each gathered row), leave along p with 16-byte stores (8-byte for bf16) when P % 4 == 0,
// 4-byte (2-byte) ones otherwise.  The tile's leading dimension is 65 floats -- one 4-byte access width of padding -- so a column read
// (32 lanes of a half wave on 32 banks) is conflict-free; the row writes rotate each lane's four elements so that they are too.
#include "tr_common.h"

#include <climits>

namespace {

constexpr int DI_THREADS = 256;
constexpr int DI_MAX_P = 1024;

struct dense_table {
  tr_decision_stage st[TR_MAX_DECISION_STAGES];
  int n_out[TR_MAX_DECISION_STAGES];
  int n;
};

__host__ __device__ inline bool stage_has_map(int kind) {
  return kind == TR_DECISION_CENTRES || kind == TR_DECISION_TOME || kind == TR_DECISION_SOFT;
}

// the levels of tr_dense_index_levels: level l's index is the state behind the first after[l] stages (ascending; 0 = in front of every stage)
struct level_table {
  int after[TR_MAX_DEPTH];
  int n;
};

// one stage applied to the state cur[] of image b (every thread of the workgroup calls it)
__device__ __forceinline__ void dense_index_stage(const int32_t* __restrict__ kept, const int32_t* __restrict__ assign, const tr_decision_stage& st,
                                                  int n_out, int b, int P0, int tid, int* cur, int* inv) {
  if (stage_has_map(st.kind)) {
    // cur[p] = assign[cur[p]]: a thread touches its own entries of cur only, no barrier needed between map stages
    const int P_in = st.n_in - 1;
    const int32_t* a = assign + st.assign_off + (size_t)b * P_in;
    for (int p = tid; p < P0; p += DI_THREADS) {
      const int c = cur[p];
      int v = -1;
      if (c >= 0 && c < P_in) {
        v = a[c];
        if (v < 0 || v >= n_out) v = -1;
      }
      cur[p] = v;
    }
  } else {
    // the kept list is absolute: cur[p] = the lowest j with kept[j] == p (an LDS atomicMin: deterministic whatever the order)
    const int W = n_out;
    const int32_t* kp = kept + st.kept_off + (size_t)b * W;
    for (int p = tid; p < P0; p += DI_THREADS) inv[p] = INT_MAX;
    __syncthreads();
    for (int j = tid; j < W; j += DI_THREADS) {
      const int v = kp[j];
      if (v >= 0 && v < P0) atomicMin(&inv[v], j);
    }
    __syncthreads();
    for (int p = tid; p < P0; p += DI_THREADS) {
      const int j = inv[p];
      cur[p] = j == INT_MAX ? -1 : j;
    }
    __syncthreads();                                     // (inv is filled again by the next kept stage)
  }
}

// index = cur + 1 where a row stands for the patch (a thread reads the entries of cur it wrote itself)
__device__ __forceinline__ void dense_index_store(const int* cur, int32_t* __restrict__ out, int P0, int tid) {
  for (int p = tid; p < P0; p += DI_THREADS) {
    const int c = cur[p];
    out[p] = c >= 0 ? c + 1 : -1;
  }
}

__global__ __launch_bounds__(DI_THREADS) void dense_index_kernel(const int32_t* __restrict__ kept, const int32_t* __restrict__ assign,
                                                                 dense_table tab, int B, int P0, int32_t* __restrict__ index_out) {
  __shared__ int cur[DI_MAX_P];
  __shared__ int inv[DI_MAX_P];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int p = tid; p < P0; p += DI_THREADS) cur[p] = p;
  for (int s = 0; s < tab.n; ++s) dense_index_stage(kept, assign, tab.st[s], tab.n_out[s], b, P0, tid, cur, inv);
  dense_index_store(cur, index_out + (size_t)b * P0, P0, tid);
}

// L levels in one walk: before stage s is applied, every level whose prefix is the first s stages takes the state as it stands
__global__ __launch_bounds__(DI_THREADS) void dense_index_levels_kernel(const int32_t* __restrict__ kept, const int32_t* __restrict__ assign,
                                                                        dense_table tab, level_table lev, int B, int P0,
                                                                        int32_t* __restrict__ index_out) {
  __shared__ int cur[DI_MAX_P];
  __shared__ int inv[DI_MAX_P];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int p = tid; p < P0; p += DI_THREADS) cur[p] = p;
  int l = 0;
  for (int s = 0; s <= tab.n; ++s) {
    for (; l < lev.n && lev.after[l] == s; ++l) dense_index_store(cur, index_out + ((size_t)l * B + b) * P0, P0, tid);
    if (s < tab.n) dense_index_stage(kept, assign, tab.st[s], tab.n_out[s], b, P0, tid, cur, inv);
  }
}

// ---- the gather ------------------------------------------------------------------------------------------------------------------------
// fp32 -> bf16 bits, round to nearest even in integer arithmetic (the bits of tensor.to(torch.bfloat16): denormals are rounded like any
// other value whatever the wave's denormal mode, a NaN becomes the quiet NaN 0x7fc0)
__device__ __forceinline__ unsigned int bf16_rne_bits(float f) {
  const unsigned int u = __builtin_bit_cast(unsigned int, f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// Channels-last: one wave per output row (b, p), lane l on the 16-byte chunks l, l + 64, ...
template <bool BF16>
__device__ __forceinline__ void gather_row_nhwc(const float* __restrict__ tokens, const int32_t* __restrict__ index, void* __restrict__ out,
                                                float fill, long row, int P, int n_rows, int D) {
  const int lane = threadIdx.x & 63;
  const long b = row / P;
  const int idx = index[row];
  const bool ok = idx >= 0 && idx < n_rows;
  const float* src = tokens + ((size_t)b * n_rows + (ok ? idx : 0)) * D;
  for (int c = 4 * lane; c < D; c += 256) {
    float4 v = make_float4(fill, fill, fill, fill);
    if (ok) v = *reinterpret_cast<const float4*>(src + c);
    if (BF16) {
      uint2 o;
      o.x = bf16_rne_bits(v.x) | (bf16_rne_bits(v.y) << 16);
      o.y = bf16_rne_bits(v.z) | (bf16_rne_bits(v.w) << 16);
      *reinterpret_cast<uint2*>(static_cast<uint16_t*>(out) + (size_t)row * D + c) = o;
    } else {
      *reinterpret_cast<float4*>(static_cast<float*>(out) + (size_t)row * D + c) = v;
    }
  }
}

template <bool BF16>
__global__ __launch_bounds__(256) void dense_gather_nhwc_kernel(const float* __restrict__ tokens, const int32_t* __restrict__ index,
                                                                void* __restrict__ out, float fill, long rows, int P, int n_rows, int D) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  gather_row_nhwc<BF16>(tokens, index, out, fill, row, P, n_rows, D);
}

// the rows of a level, per level of tr_dense_gather_levels (a kernel argument: a captured graph holds it)
struct level_rows_table {
  int rows[TR_MAX_DEPTH];
};

// ... for L levels: the rows of level l are l * B * P ... (l + 1) * B * P - 1 of one launch; a level's tokens, index and map are slabs of
// level_stride, B * P and B * P * D elements
template <bool BF16>
__global__ __launch_bounds__(256) void dense_gather_levels_nhwc_kernel(const float* __restrict__ tokens, size_t level_stride, level_rows_table lr,
                                                                       const int32_t* __restrict__ index, void* __restrict__ out, float fill,
                                                                       long rows_per_level, long rows, int P, int D) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int l = (int)(row / rows_per_level);
  const size_t o = (size_t)l * rows_per_level * D;
  void* out_l = BF16 ? static_cast<void*>(static_cast<uint16_t*>(out) + o) : static_cast<void*>(static_cast<float*>(out) + o);
  gather_row_nhwc<BF16>(tokens + l * level_stride, index + (size_t)l * rows_per_level, out_l, fill, row - l * rows_per_level, P, lr.rows[l], D);
}

constexpr int DG_TP = 64;            // patches per tile
constexpr int DG_TC = 64;            // channels per tile
constexpr int DG_LD = DG_TC + 1;     // one 4-byte access width of padding: column reads hit 32 different banks

// NCHW: tile (image b, patches p0 ... p0+63, channels c0 ... c0+63).  The tiles of one image are consecutive logical ids, and xcd_remap gives
// each XCD a contiguous run of them: the rows of an image that many patches share (the merge families) are then read through one L2.
template <bool BF16, bool VEC>
__device__ __forceinline__ void gather_tile_nchw(const float* __restrict__ tokens, const int32_t* __restrict__ index, void* __restrict__ out,
                                                 float fill, int P, int n_rows, int D, int b, int p0, int c0, float* tile) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  // rows in: a wave instruction takes 4 rows x 64 channels, 16 lanes per row; all four loads of a wave are issued before the first write
  const int l16 = lane & 15, c = c0 + 4 * l16;
  float4 v[4];
  int rr[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    rr[it] = wave * 16 + it * 4 + (lane >> 4);
    const int p = p0 + rr[it];
    int idx = -1;
    if (p < P) idx = index[(size_t)b * P + p];
    v[it] = make_float4(fill, fill, fill, fill);
    if (idx >= 0 && idx < n_rows && c < D) v[it] = *reinterpret_cast<const float4*>(tokens + ((size_t)b * n_rows + idx) * D + c);
  }
  // a half wave writes rows r and r + 1 (65 floats apart: one bank on), 16 lanes each, lane l16 on elements 4 * l16 ... + 3.  With step i
  // writing element (i + rot) % 4, rot = 0, 1, 1, 2 for the four groups of 8 lanes, the 32 lanes of a ds_write_b32 hit 32 different banks
  const int rot = (((lane >> 3) & 3) + 1) >> 1;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const float e[4] = {v[it].x, v[it].y, v[it].z, v[it].w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = (i + rot) & 3;
      const float val = j == 0 ? e[0] : j == 1 ? e[1] : j == 2 ? e[2] : e[3];
      tile[rr[it] * DG_LD + 4 * l16 + j] = val;
    }
  }
  __syncthreads();

  if (VEC) {
    // columns out: a half wave takes 32 patches x 4 channels -- lane = (8 groups of 4 patches) x (4 channels): step j reads
    // tile[4 * lp + j][cc], banks 4 * lp + j + cc -- and the two halves of a wave store the two 128-byte halves of the same channel rows
    const int lp = lane & 7, cc = (lane >> 3) & 3, half = lane >> 5;
    const int pr = 32 * half + 4 * lp, p = p0 + pr;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int cr = wave * 16 + it * 4 + cc, ch = c0 + cr;
      float o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = tile[(pr + j) * DG_LD + cr];
      if (ch < D && p < P) {                             // (P % 4 == 0: p < P means p + 3 < P)
        const size_t at = ((size_t)b * D + ch) * P + p;
        if (BF16) {
          uint2 w;
          w.x = bf16_rne_bits(o[0]) | (bf16_rne_bits(o[1]) << 16);
          w.y = bf16_rne_bits(o[2]) | (bf16_rne_bits(o[3]) << 16);
          *reinterpret_cast<uint2*>(static_cast<uint16_t*>(out) + at) = w;
        } else {
          *reinterpret_cast<float4*>(static_cast<float*>(out) + at) = make_float4(o[0], o[1], o[2], o[3]);
        }
      }
    }
  } else {
    // P % 4 != 0: the channel rows of the output are not 16-byte aligned -- one element per lane, a wave on 64 patches of one channel
    const int p = p0 + lane;
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int cr = wave * 16 + it, ch = c0 + cr;
      const float o = tile[lane * DG_LD + cr];
      if (ch < D && p < P) {
        const size_t at = ((size_t)b * D + ch) * P + p;
        if (BF16) static_cast<uint16_t*>(out)[at] = (uint16_t)bf16_rne_bits(o);
        else static_cast<float*>(out)[at] = o;
      }
    }
  }
}

template <bool BF16, bool VEC>
__global__ __launch_bounds__(256) void dense_gather_nchw_kernel(const float* __restrict__ tokens, const int32_t* __restrict__ index,
                                                                void* __restrict__ out, float fill, int P, int n_rows, int D, int ptiles,
                                                                int ctiles) {
  __shared__ float tile[DG_TP * DG_LD];
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int ct = id % ctiles, pt = (id / ctiles) % ptiles, b = id / (ctiles * ptiles);
  gather_tile_nchw<BF16, VEC>(tokens, index, out, fill, P, n_rows, D, b, pt * DG_TP, ct * DG_TC, tile);
}

// ... for L levels in one launch: the logical tile order is (level, image, patch tile, channel tile), the level slowest, and xcd_remap gives
// each XCD a contiguous run of it -- inside a level the tiles of an image stay neighbours on one L2, as in the single-level kernel
template <bool BF16, bool VEC>
__global__ __launch_bounds__(256) void dense_gather_levels_nchw_kernel(const float* __restrict__ tokens, size_t level_stride, level_rows_table lr,
                                                                       const int32_t* __restrict__ index, void* __restrict__ out, float fill,
                                                                       int B, int P, int D, int ptiles, int ctiles) {
  __shared__ float tile[DG_TP * DG_LD];
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int per_image = ctiles * ptiles;
  const int ct = id % ctiles, pt = (id / ctiles) % ptiles, b = (id / per_image) % B, l = id / (per_image * B);
  const size_t o = (size_t)l * B * P * D;
  void* out_l = BF16 ? static_cast<void*>(static_cast<uint16_t*>(out) + o) : static_cast<void*>(static_cast<float*>(out) + o);
  gather_tile_nchw<BF16, VEC>(tokens + l * level_stride, index + (size_t)l * B * P, out_l, fill, P, lr.rows[l], D, b, pt * DG_TP, ct * DG_TC, tile);
}

// ---- the scatter: the gather's adjoint -------------------------------------------------------------------------------------------------
// dtokens[b, r, :] = the sum of dmap[b, :, p] over the patches p with index[b, p] == r, in fp32, one addition after the other in ascending p
// starting from +0.  An output row is owned by one wave (channels-last) or by one lane per channel (NCHW) that walks the row's patches in
// order, so there is nothing to clear, nothing atomic and one set of bits whatever the launch.  The row's patches come from a ballot over the
// image's index, 64 entries a step: the set bits, lowest first, ARE the ascending list -- no inverse table in memory, no scratch.
// `index == r` with 0 <= r < n_rows is the whole domain check: -1, -2 and anything >= n_rows equal no row and are never used as an address.
__device__ __forceinline__ float bf16_bits_to_f32(unsigned int h) { return __builtin_bit_cast(float, h << 16); }

// Channels-last: a wave per output row (b, r), lane l on the 16-byte (bf16 input: 8-byte) chunks l, l + 64, ... of every patch row it sums
template <bool IN_BF16, bool OUT_BF16>
__device__ __forceinline__ void scatter_row_nhwc(const void* __restrict__ dmap, const int32_t* __restrict__ index, void* __restrict__ out,
                                                 long row, int P, int n_rows, int D) {
  const int lane = threadIdx.x & 63;
  const long b = row / n_rows;
  const int r = (int)(row - b * n_rows);
  const int32_t* idx = index + (size_t)b * P;
  float4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int p0 = 0; p0 < P; p0 += 64) {
    const int pl = p0 + lane;
    unsigned long long mask = __ballot(pl < P && idx[pl] == r);
    while (mask) {
      const int p = p0 + __ffsll((long long)mask) - 1;     // p < P: only lanes with pl < P vote
      mask &= mask - 1;
      const size_t at = ((size_t)b * P + p) * D;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * lane + 256 * j;
        if (c < D) {
          float4 v;
          if (IN_BF16) {
            const uint2 u = *reinterpret_cast<const uint2*>(static_cast<const uint16_t*>(dmap) + at + c);
            v = make_float4(bf16_bits_to_f32(u.x & 0xffffu), bf16_bits_to_f32(u.x >> 16), bf16_bits_to_f32(u.y & 0xffffu), bf16_bits_to_f32(u.y >> 16));
          } else {
            v = *reinterpret_cast<const float4*>(static_cast<const float*>(dmap) + at + c);
          }
          acc[j].x += v.x;
          acc[j].y += v.y;
          acc[j].z += v.z;
          acc[j].w += v.w;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = 4 * lane + 256 * j;
    if (c < D) {
      if (OUT_BF16) {
        uint2 o;
        o.x = bf16_rne_bits(acc[j].x) | (bf16_rne_bits(acc[j].y) << 16);
        o.y = bf16_rne_bits(acc[j].z) | (bf16_rne_bits(acc[j].w) << 16);
        *reinterpret_cast<uint2*>(static_cast<uint16_t*>(out) + (size_t)row * D + c) = o;
      } else {
        *reinterpret_cast<float4*>(static_cast<float*>(out) + (size_t)row * D + c) = acc[j];
      }
    }
  }
}

template <bool IN_BF16, bool OUT_BF16>
__global__ __launch_bounds__(256) void dense_scatter_nhwc_kernel(const void* __restrict__ dmap, const int32_t* __restrict__ index,
                                                                 void* __restrict__ out, long rows, int P, int n_rows, int D) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                 // (wave-uniform)
  scatter_row_nhwc<IN_BF16, OUT_BF16>(dmap, index, out, row, P, n_rows, D);
}

// The levels of tr_dense_scatter_levels (a kernel argument): a level's map gradient (NULL: no gradient, no workgroup), its rows, and where
// its workgroups start -- channels-last: in the launch, the level slowest; NCHW: among the tiles of one image; a level without a gradient
// has start[l] == start[l + 1]
struct level_scatter_table {
  const void* dmap[TR_MAX_DEPTH];
  int rows[TR_MAX_DEPTH];
  int start[TR_MAX_DEPTH + 1];
};
__device__ __forceinline__ int scatter_level_of(const level_scatter_table& lt, int L, int id) {
  int l = 0;
  while (l + 1 < L && id >= lt.start[l + 1]) ++l;          // (uniform over the workgroup; an empty level is stepped over)
  return l;
}
template <bool OUT_BF16>
__device__ __forceinline__ void* scatter_level_out(void* out, size_t elems) {
  return OUT_BF16 ? static_cast<void*>(static_cast<uint16_t*>(out) + elems) : static_cast<void*>(static_cast<float*>(out) + elems);
}

// ... for L levels: workgroup id -> (level, four rows of it); a level's index and output are slabs of B * P and level_stride elements
template <bool IN_BF16, bool OUT_BF16>
__global__ __launch_bounds__(256) void dense_scatter_levels_nhwc_kernel(level_scatter_table lt, int L, const int32_t* __restrict__ index,
                                                                        void* __restrict__ out, size_t level_stride, int B, int P, int D) {
  const int l = scatter_level_of(lt, L, (int)blockIdx.x);
  const int n_rows = lt.rows[l];
  const long row = (long)((int)blockIdx.x - lt.start[l]) * 4 + (threadIdx.x >> 6);
  if (row >= (long)B * n_rows) return;                     // (wave-uniform)
  scatter_row_nhwc<IN_BF16, OUT_BF16>(lt.dmap[l], index + (size_t)l * B * P, scatter_level_out<OUT_BF16>(out, l * level_stride), row, P, n_rows, D);
}

constexpr int DS_TR = 32;            // output rows per tile (8 per wave)
constexpr int DS_TC = 64;            // channels per tile: a lane per channel

// NCHW: tile (image b, rows r0 ... r0+31, channels c0 ... c0+63); lane l owns channel c0 + l of the rows of its wave and reads the single
// elements dmap[b, c, p] of the row's patches (stride P between lanes), stores along c.  The image's index sits in LDS.  Wave w takes the rows
// r0 + w, r0 + w + 4, ...: the four waves work on neighbouring rows -- with a pruning family's index neighbouring patches, the same lines of
// the map -- at the same time.  The tiles of one image are consecutive logical ids (channel tile fastest) and xcd_remap gives an XCD a
// contiguous run of them, as in the gather: a line of the image's D x P slab is fetched from HBM once and served by one L2 afterwards.
template <bool IN_BF16, bool OUT_BF16>
__device__ __forceinline__ void scatter_tile_nchw(const void* __restrict__ dmap, const int32_t* __restrict__ index, void* __restrict__ out, int P,
                                                  int n_rows, int D, int b, int rt, int ct, int* sidx) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int p = threadIdx.x; p < P; p += 256) sidx[p] = index[(size_t)b * P + p];
  __syncthreads();
  const int c = ct * DS_TC + lane;
  const bool mine = c < D;
  const size_t col = ((size_t)b * D + (mine ? c : 0)) * P;  // channel c's P elements
  for (int k = 0; k < DS_TR / 4; ++k) {
    const int r = rt * DS_TR + wave + 4 * k;
    if (r >= n_rows) break;                                // (wave-uniform)
    float acc = 0.f;
    for (int p0 = 0; p0 < P; p0 += 64) {
      const int pl = p0 + lane;
      unsigned long long mask = __ballot(pl < P && sidx[pl] == r);
      while (mask) {
        const int p = p0 + __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        if (mine) {
          if (IN_BF16) acc += bf16_bits_to_f32(static_cast<const uint16_t*>(dmap)[col + p]);
          else acc += static_cast<const float*>(dmap)[col + p];
        }
      }
    }
    if (mine) {
      const size_t at = ((size_t)b * n_rows + r) * D + c;
      if (OUT_BF16) static_cast<uint16_t*>(out)[at] = (uint16_t)bf16_rne_bits(acc);
      else static_cast<float*>(out)[at] = acc;
    }
  }
}

template <bool IN_BF16, bool OUT_BF16>
__global__ __launch_bounds__(256) void dense_scatter_nchw_kernel(const void* __restrict__ dmap, const int32_t* __restrict__ index,
                                                                 void* __restrict__ out, int P, int n_rows, int D, int rtiles, int ctiles) {
  __shared__ int sidx[DI_MAX_P];
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int ct = id % ctiles, rt = (id / ctiles) % rtiles, b = id / (ctiles * rtiles);
  scatter_tile_nchw<IN_BF16, OUT_BF16>(dmap, index, out, P, n_rows, D, b, rt, ct, sidx);
}

// ... for L levels in one launch.  The logical tile order is (image, level, row tile, channel tile) through the same xcd_remap: inside a level
// the tiles of an image stay neighbours on one L2, as in the single-level kernel, and an XCD's contiguous run holds whole images with ALL
// their levels.  With the level slowest an XCD's run would be (part of) one level, and the levels' tiles do not cost the same: under a
// merge index every level sums all P patches of an image into fewer and fewer rows, so the last level's few tiles carry a quarter of the
// work on an eighth of the chip (measured: 0.58 ms against 0.33 ms for four launches under ToMe's index; profiles/dense_train_levels_lab.md).
// A level has its own number of row tiles; lt.start[l] is its first tile inside an image, per_image the tiles of one image
template <bool IN_BF16, bool OUT_BF16>
__global__ __launch_bounds__(256) void dense_scatter_levels_nchw_kernel(level_scatter_table lt, int L, const int32_t* __restrict__ index,
                                                                        void* __restrict__ out, size_t level_stride, int B, int P, int D,
                                                                        int ctiles, int per_image) {
  __shared__ int sidx[DI_MAX_P];
  const int id = xcd_remap(blockIdx.x, gridDim.x);
  const int b = id / per_image, ti = id - b * per_image;
  const int l = scatter_level_of(lt, L, ti);
  const int t = ti - lt.start[l];
  const int ct = t % ctiles, rt = t / ctiles;
  scatter_tile_nchw<IN_BF16, OUT_BF16>(lt.dmap[l], index + (size_t)l * B * P, scatter_level_out<OUT_BF16>(out, l * level_stride), P, lt.rows[l], D,
                                       b, rt, ct, sidx);
}

}  // namespace

// the stage table checked and copied into `tab` with every stage's n_out (tr_dense_index's rules, for both index entry points)
static int dense_build_table(const char* who, const int32_t* kept, size_t kept_elems, const int32_t* assign, size_t assign_elems,
                             const tr_decision_stage* stages, int n_stages, int B, int P0, dense_table* tab_out) {
  dense_table& tab = *tab_out;
  tab.n = n_stages;
  int last_block = -1, n_out = P0;
  bool seen_map = false;
  for (int i = 0; i < n_stages; ++i) {
    const tr_decision_stage& st = stages[i];
    TR_REQUIRE(st.kind >= TR_DECISION_PRUNE && st.kind <= TR_DECISION_SOFT, TR_ERR_CONFIG, "%s: stage %d has kind %d", who, i, st.kind);
    TR_REQUIRE(st.block > last_block && st.block < TR_MAX_DEPTH, TR_ERR_CONFIG, "%s: stage %d names block %d (ascending blocks below %d)", who, i,
               st.block, TR_MAX_DEPTH);
    last_block = st.block;
    TR_REQUIRE(st.n_in >= 2 && st.n_in <= P0 + 1 && st.k >= 1 && st.k < st.n_in, TR_ERR_SHAPE,
               "%s: stage %d needs 2 <= n_in <= P0 + 1 and 1 <= k < n_in (n_in=%d k=%d P0=%d)", who, i, st.n_in, st.k, P0);
    TR_REQUIRE(st.kind != TR_DECISION_ATS || st.k >= 2, TR_ERR_SHAPE, "%s: stage %d: an ATS stage needs k >= 2", who, i);
    if (stage_has_map(st.kind)) {
      seen_map = true;
      n_out = st.kind == TR_DECISION_TOME ? st.n_in - 1 - (st.k < (st.n_in - 1) / 2 ? st.k : (st.n_in - 1) / 2) : st.k;
      const size_t P_in = (size_t)st.n_in - 1;
      TR_REQUIRE(assign, TR_ERR_NULL, "%s: stage %d reads an assignment map, assign is NULL", who, i);
      TR_REQUIRE(st.assign_off >= 0 && (size_t)st.assign_off + (size_t)B * P_in <= assign_elems, TR_ERR_SHAPE,
                 "%s: stage %d: map [%d, %zu] at %lld leaves assign (%zu elements)", who, i, B, P_in, (long long)st.assign_off, assign_elems);
    } else {
      // an absolute kept list overrides the state: behind a map stage the rows it names are no grid patches any more
      TR_REQUIRE(!seen_map, TR_ERR_CONFIG, "%s: stage %d has only a kept list and stands behind a stage with an assignment map", who, i);
      n_out = st.kind == TR_DECISION_EVIT ? st.k + 1 : st.kind == TR_DECISION_ATS ? st.k - 1 : st.k;
      TR_REQUIRE(kept, TR_ERR_NULL, "%s: stage %d reads a kept list, kept is NULL", who, i);
      TR_REQUIRE(st.kept_off >= 0 && (size_t)st.kept_off + (size_t)B * n_out <= kept_elems, TR_ERR_SHAPE,
                 "%s: stage %d: kept list [%d, %d] at %lld leaves kept (%zu elements)", who, i, B, n_out, (long long)st.kept_off, kept_elems);
    }
    tab.st[i] = st;
    tab.n_out[i] = n_out;
  }
  return TR_OK;
}

extern "C" int tr_dense_index(const int32_t* kept, size_t kept_elems, const int32_t* assign, size_t assign_elems, const tr_decision_stage* stages,
                              int n_stages, int B, int P0, int n_last, int32_t* index_out, tr_stream_t s) {
  TR_REQUIRE(n_stages >= 0 && n_stages <= TR_MAX_DECISION_STAGES, TR_ERR_CONFIG, "tr_dense_index: %d stages (at most %d)", n_stages,
             TR_MAX_DECISION_STAGES);
  TR_REQUIRE(index_out && (n_stages == 0 || stages), TR_ERR_NULL, "tr_dense_index: null pointer");
  TR_REQUIRE(B > 0 && P0 >= 1 && P0 <= DI_MAX_P && n_last >= 2, TR_ERR_SHAPE, "tr_dense_index: need B > 0, 1 <= P0 <= 1024, n_last >= 2 (B=%d P0=%d n_last=%d)",
             B, P0, n_last);
  dense_table tab;
  const int rc = dense_build_table("tr_dense_index", kept, kept_elems, assign, assign_elems, stages, n_stages, B, P0, &tab);
  if (rc != TR_OK) return rc;
  const int n_out = n_stages > 0 ? tab.n_out[n_stages - 1] : P0;
  TR_REQUIRE(n_out == n_last - 1, TR_ERR_SHAPE, "tr_dense_index: the stages end at %d patch rows, the last stream has %d", n_out, n_last - 1);
  TR_REQUIRE(tr_aligned16(kept) && tr_aligned16(assign) && tr_aligned16(index_out), TR_ERR_ALIGN, "tr_dense_index: pointers must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(s);
  tr_prof_note("tr_dense_index", 0.0, 4.0 * B * P0 * (n_stages + 1));
  hipLaunchKernelGGL(dense_index_kernel, dim3(B), dim3(DI_THREADS), 0, st, kept, assign, tab, B, P0, index_out);
  TR_CHECK_LAUNCH("tr_dense_index");
  return TR_OK;
}

extern "C" int tr_dense_index_levels(const int32_t* kept, size_t kept_elems, const int32_t* assign, size_t assign_elems,
                                     const tr_decision_stage* stages, int n_stages, int B, int P0, const int32_t* level_blocks,
                                     const int32_t* level_rows, int L, int32_t* index_out, tr_stream_t s) {
  TR_REQUIRE(n_stages >= 0 && n_stages <= TR_MAX_DECISION_STAGES, TR_ERR_CONFIG, "tr_dense_index_levels: %d stages (at most %d)", n_stages,
             TR_MAX_DECISION_STAGES);
  TR_REQUIRE(L >= 1 && L <= TR_MAX_DEPTH, TR_ERR_CONFIG, "tr_dense_index_levels: %d levels (1 ... %d)", L, TR_MAX_DEPTH);
  TR_REQUIRE(index_out && level_blocks && level_rows && (n_stages == 0 || stages), TR_ERR_NULL, "tr_dense_index_levels: null pointer");
  TR_REQUIRE(B > 0 && P0 >= 1 && P0 <= DI_MAX_P, TR_ERR_SHAPE, "tr_dense_index_levels: need B > 0, 1 <= P0 <= 1024 (B=%d P0=%d)", B, P0);
  for (int l = 0; l < L; ++l)
    TR_REQUIRE(level_blocks[l] >= 0 && level_blocks[l] < TR_MAX_DEPTH && (l == 0 || level_blocks[l] > level_blocks[l - 1]), TR_ERR_CONFIG,
               "tr_dense_index_levels: level %d names block %d (strictly ascending blocks in 0 ... %d)", l, level_blocks[l], TR_MAX_DEPTH - 1);
  dense_table tab;
  const int rc = dense_build_table("tr_dense_index_levels", kept, kept_elems, assign, assign_elems, stages, n_stages, B, P0, &tab);
  if (rc != TR_OK) return rc;
  // a level's prefix: the stages at or before its block.  What that prefix leaves must be the rows the caller saw in the stream there
  level_table lev;
  lev.n = L;
  for (int l = 0, after = 0; l < L; ++l) {
    while (after < n_stages && stages[after].block <= level_blocks[l]) ++after;
    lev.after[l] = after;
    const int n_out = after > 0 ? tab.n_out[after - 1] : P0;
    TR_REQUIRE(n_out == level_rows[l] - 1, TR_ERR_SHAPE, "tr_dense_index_levels: the stages up to block %d leave %d patch rows, level %d has %d",
               level_blocks[l], n_out, l, level_rows[l] - 1);
  }
  TR_REQUIRE(tr_aligned16(kept) && tr_aligned16(assign) && tr_aligned16(index_out), TR_ERR_ALIGN,
             "tr_dense_index_levels: pointers must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(s);
  tr_prof_note("tr_dense_index_levels", 0.0, 4.0 * B * P0 * (n_stages + L));
  hipLaunchKernelGGL(dense_index_levels_kernel, dim3(B), dim3(DI_THREADS), 0, st, kept, assign, tab, lev, B, P0, index_out);
  TR_CHECK_LAUNCH("tr_dense_index_levels");
  return TR_OK;
}

extern "C" int tr_dense_gather(const float* tokens, const int32_t* index, void* out, int layout, int out_is_bf16, float fill, int B, int P,
                               int n_rows, int D, tr_stream_t s) {
  TR_REQUIRE(tokens && index && out, TR_ERR_NULL, "tr_dense_gather: null pointer");
  TR_REQUIRE(layout == TR_LAYOUT_NCHW || layout == TR_LAYOUT_NHWC, TR_ERR_CONFIG, "tr_dense_gather: layout %d (TR_LAYOUT_NCHW or TR_LAYOUT_NHWC)", layout);
  TR_REQUIRE(B > 0 && P >= 1 && P <= DI_MAX_P && n_rows >= 1 && D > 0 && D % 4 == 0 && D <= 1024, TR_ERR_SHAPE,
             "tr_dense_gather: need B > 0, 1 <= P <= 1024, n_rows >= 1, D %% 4 == 0, D <= 1024 (B=%d P=%d n_rows=%d D=%d)", B, P, n_rows, D);
  TR_REQUIRE(tr_aligned16(tokens) && tr_aligned16(index) && tr_aligned16(out), TR_ERR_ALIGN, "tr_dense_gather: pointers must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(s);
  const bool bf = out_is_bf16 != 0;
  // required traffic: every output element once, at most as many token bytes, the index
  tr_prof_note("tr_dense_gather", 0.0, (double)B * P * D * (4.0 + (bf ? 2.0 : 4.0)) + 4.0 * B * P);
  if (layout == TR_LAYOUT_NHWC) {
    const long rows = (long)B * P;
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (bf) hipLaunchKernelGGL((dense_gather_nhwc_kernel<true>), grid, dim3(256), 0, st, tokens, index, out, fill, rows, P, n_rows, D);
    else hipLaunchKernelGGL((dense_gather_nhwc_kernel<false>), grid, dim3(256), 0, st, tokens, index, out, fill, rows, P, n_rows, D);
  } else {
    const int ptiles = (P + DG_TP - 1) / DG_TP, ctiles = (D + DG_TC - 1) / DG_TC;
    const long blocks = (long)B * ptiles * ctiles;
    TR_REQUIRE(blocks <= INT_MAX, TR_ERR_SHAPE, "tr_dense_gather: %ld tiles", blocks);
    const dim3 grid((unsigned)blocks);
    const bool vec = P % 4 == 0;
#define DG_LAUNCH(BF, VEC) \
  hipLaunchKernelGGL((dense_gather_nchw_kernel<BF, VEC>), grid, dim3(256), 0, st, tokens, index, out, fill, P, n_rows, D, ptiles, ctiles)
    if (bf && vec) DG_LAUNCH(true, true);
    else if (bf) DG_LAUNCH(true, false);
    else if (vec) DG_LAUNCH(false, true);
    else DG_LAUNCH(false, false);
#undef DG_LAUNCH
  }
  TR_CHECK_LAUNCH("tr_dense_gather");
  return TR_OK;
}

extern "C" int tr_dense_gather_levels(const float* tokens, size_t level_stride, const int32_t* level_rows, int L, const int32_t* index, void* out,
                                      int layout, int out_is_bf16, float fill, int B, int P, int D, tr_stream_t s) {
  TR_REQUIRE(tokens && level_rows && index && out, TR_ERR_NULL, "tr_dense_gather_levels: null pointer");
  TR_REQUIRE(layout == TR_LAYOUT_NCHW || layout == TR_LAYOUT_NHWC, TR_ERR_CONFIG, "tr_dense_gather_levels: layout %d (TR_LAYOUT_NCHW or TR_LAYOUT_NHWC)",
             layout);
  TR_REQUIRE(L >= 1 && L <= TR_MAX_DEPTH, TR_ERR_CONFIG, "tr_dense_gather_levels: %d levels (1 ... %d)", L, TR_MAX_DEPTH);
  TR_REQUIRE(B > 0 && P >= 1 && P <= DI_MAX_P && D > 0 && D % 4 == 0 && D <= 1024, TR_ERR_SHAPE,
             "tr_dense_gather_levels: need B > 0, 1 <= P <= 1024, D %% 4 == 0, D <= 1024 (B=%d P=%d D=%d)", B, P, D);
  level_rows_table lr;
  for (int l = 0; l < L; ++l) {
    // a level's rows [B, n_rows, D] lie inside its slab; slabs start 16-byte aligned
    TR_REQUIRE(level_rows[l] >= 1 && (size_t)B * level_rows[l] * D <= level_stride, TR_ERR_SHAPE,
               "tr_dense_gather_levels: level %d has %d rows: [%d, %d, %d] does not fit a slab of %zu elements", l, level_rows[l], B, level_rows[l],
               D, level_stride);
    lr.rows[l] = level_rows[l];
  }
  TR_REQUIRE(level_stride % 4 == 0, TR_ERR_ALIGN, "tr_dense_gather_levels: level_stride %zu is not a multiple of 4 elements", level_stride);
  TR_REQUIRE(tr_aligned16(tokens) && tr_aligned16(index) && tr_aligned16(out), TR_ERR_ALIGN,
             "tr_dense_gather_levels: pointers must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(s);
  const bool bf = out_is_bf16 != 0;
  tr_prof_note("tr_dense_gather_levels", 0.0, (double)L * ((double)B * P * D * (4.0 + (bf ? 2.0 : 4.0)) + 4.0 * B * P));
  if (layout == TR_LAYOUT_NHWC) {
    const long per_level = (long)B * P, rows = per_level * L;
    TR_REQUIRE((rows + 3) / 4 <= INT_MAX, TR_ERR_SHAPE, "tr_dense_gather_levels: %ld rows", rows);
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (bf) hipLaunchKernelGGL((dense_gather_levels_nhwc_kernel<true>), grid, dim3(256), 0, st, tokens, level_stride, lr, index, out, fill, per_level, rows, P, D);
    else hipLaunchKernelGGL((dense_gather_levels_nhwc_kernel<false>), grid, dim3(256), 0, st, tokens, level_stride, lr, index, out, fill, per_level, rows, P, D);
  } else {
    const int ptiles = (P + DG_TP - 1) / DG_TP, ctiles = (D + DG_TC - 1) / DG_TC;
    const long blocks = (long)L * B * ptiles * ctiles;
    TR_REQUIRE(blocks <= INT_MAX, TR_ERR_SHAPE, "tr_dense_gather_levels: %ld tiles", blocks);
    const dim3 grid((unsigned)blocks);
    const bool vec = P % 4 == 0;
#define DG_LAUNCH(BF, VEC)                                                                                                                   \
  hipLaunchKernelGGL((dense_gather_levels_nchw_kernel<BF, VEC>), grid, dim3(256), 0, st, tokens, level_stride, lr, index, out, fill, B, P, D, \
                     ptiles, ctiles)
    if (bf && vec) DG_LAUNCH(true, true);
    else if (bf) DG_LAUNCH(true, false);
    else if (vec) DG_LAUNCH(false, true);
    else DG_LAUNCH(false, false);
#undef DG_LAUNCH
  }
  TR_CHECK_LAUNCH("tr_dense_gather_levels");
  return TR_OK;
}

extern "C" int tr_dense_scatter(const void* dmap, const int32_t* index, void* dtokens, int layout, int dmap_is_bf16, int out_is_bf16, int B, int P,
                                int n_rows, int D, tr_stream_t s) {
  TR_REQUIRE(dmap && index && dtokens, TR_ERR_NULL, "tr_dense_scatter: null pointer");
  TR_REQUIRE(layout == TR_LAYOUT_NCHW || layout == TR_LAYOUT_NHWC, TR_ERR_CONFIG, "tr_dense_scatter: layout %d (TR_LAYOUT_NCHW or TR_LAYOUT_NHWC)", layout);
  TR_REQUIRE(B > 0 && P >= 1 && P <= DI_MAX_P && n_rows >= 1 && D > 0 && D % 4 == 0 && D <= 1024, TR_ERR_SHAPE,
             "tr_dense_scatter: need B > 0, 1 <= P <= 1024, n_rows >= 1, D %% 4 == 0, D <= 1024 (B=%d P=%d n_rows=%d D=%d)", B, P, n_rows, D);
  TR_REQUIRE(tr_aligned16(dmap) && tr_aligned16(index) && tr_aligned16(dtokens), TR_ERR_ALIGN, "tr_dense_scatter: pointers must be 16-byte aligned");
  const bool ib = dmap_is_bf16 != 0, ob = out_is_bf16 != 0;
  const long rows = (long)B * n_rows;
  const int rtiles = (n_rows + DS_TR - 1) / DS_TR, ctiles = (D + DS_TC - 1) / DS_TC;
  const long blocks = layout == TR_LAYOUT_NHWC ? (rows + 3) / 4 : (long)B * rtiles * ctiles;
  TR_REQUIRE(blocks <= INT_MAX, TR_ERR_SHAPE, "tr_dense_scatter: %ld workgroups", blocks);
  hipStream_t st = static_cast<hipStream_t>(s);
  // required traffic: every element of the map once at most, every output element once, the index
  tr_prof_note("tr_dense_scatter", 0.0, (double)B * P * D * (ib ? 2.0 : 4.0) + (double)rows * D * (ob ? 2.0 : 4.0) + 4.0 * B * P);
  const dim3 grid((unsigned)blocks);
#define DS_LAUNCH(IB, OB)                                                                                                          \
  do {                                                                                                                             \
    if (layout == TR_LAYOUT_NHWC)                                                                                                  \
      hipLaunchKernelGGL((dense_scatter_nhwc_kernel<IB, OB>), grid, dim3(256), 0, st, dmap, index, dtokens, rows, P, n_rows, D);   \
    else                                                                                                                           \
      hipLaunchKernelGGL((dense_scatter_nchw_kernel<IB, OB>), grid, dim3(256), 0, st, dmap, index, dtokens, P, n_rows, D, rtiles, ctiles); \
  } while (0)
  if (ib && ob) DS_LAUNCH(true, true);
  else if (ib) DS_LAUNCH(true, false);
  else if (ob) DS_LAUNCH(false, true);
  else DS_LAUNCH(false, false);
#undef DS_LAUNCH
  TR_CHECK_LAUNCH("tr_dense_scatter");
  return TR_OK;
}

extern "C" int tr_dense_scatter_levels(const void* const* dmaps, const int32_t* index, void* dtokens, size_t level_stride,
                                       const int32_t* level_rows, int L, int layout, int dmap_is_bf16, int out_is_bf16, int B, int P, int D,
                                       tr_stream_t s) {
  TR_REQUIRE(dmaps && level_rows && index && dtokens, TR_ERR_NULL, "tr_dense_scatter_levels: null pointer");
  TR_REQUIRE(layout == TR_LAYOUT_NCHW || layout == TR_LAYOUT_NHWC, TR_ERR_CONFIG, "tr_dense_scatter_levels: layout %d (TR_LAYOUT_NCHW or TR_LAYOUT_NHWC)",
             layout);
  TR_REQUIRE(L >= 1 && L <= TR_MAX_DEPTH, TR_ERR_CONFIG, "tr_dense_scatter_levels: %d levels (1 ... %d)", L, TR_MAX_DEPTH);
  TR_REQUIRE(B > 0 && P >= 1 && P <= DI_MAX_P && D > 0 && D % 4 == 0 && D <= 1024, TR_ERR_SHAPE,
             "tr_dense_scatter_levels: need B > 0, 1 <= P <= 1024, D %% 4 == 0, D <= 1024 (B=%d P=%d D=%d)", B, P, D);
  const bool ib = dmap_is_bf16 != 0, ob = out_is_bf16 != 0, nhwc = layout == TR_LAYOUT_NHWC;
  const int ctiles = (D + DS_TC - 1) / DS_TC;
  level_scatter_table lt;
  long blocks = 0;
  bool aligned = true;
  double bytes = 0.0;
  for (int l = 0; l < L; ++l) {
    // a level's rows [B, n_rows, D] lie inside its slab, present or not; slabs start 16-byte aligned
    TR_REQUIRE(level_rows[l] >= 1 && (size_t)B * level_rows[l] * D <= level_stride, TR_ERR_SHAPE,
               "tr_dense_scatter_levels: level %d has %d rows: [%d, %d, %d] does not fit a slab of %zu elements", l, level_rows[l], B,
               level_rows[l], D, level_stride);
    lt.dmap[l] = dmaps[l];
    lt.rows[l] = level_rows[l];
    lt.start[l] = (int)blocks;
    if (dmaps[l] == nullptr) continue;
    aligned = aligned && tr_aligned16(dmaps[l]);
    const long rows = (long)B * level_rows[l];
    // channels-last: the level's first workgroup in the launch; NCHW: its first tile inside an image
    blocks += nhwc ? (rows + 3) / 4 : (long)((level_rows[l] + DS_TR - 1) / DS_TR) * ctiles;
    TR_REQUIRE(blocks * (nhwc ? 1 : B) <= INT_MAX, TR_ERR_SHAPE, "tr_dense_scatter_levels: %ld workgroups", blocks * (nhwc ? 1 : B));
    bytes += (double)B * P * D * (ib ? 2.0 : 4.0) + (double)rows * D * (ob ? 2.0 : 4.0) + 4.0 * B * P;
  }
  for (int l = L; l <= TR_MAX_DEPTH; ++l) lt.start[l] = (int)blocks;
  for (int l = L; l < TR_MAX_DEPTH; ++l) {
    lt.dmap[l] = nullptr;
    lt.rows[l] = 1;
  }
  TR_REQUIRE(level_stride % (ob ? 8 : 4) == 0, TR_ERR_ALIGN, "tr_dense_scatter_levels: level_stride %zu does not keep the slabs 16-byte aligned",
             level_stride);
  TR_REQUIRE(aligned && tr_aligned16(index) && tr_aligned16(dtokens), TR_ERR_ALIGN, "tr_dense_scatter_levels: pointers must be 16-byte aligned");
  if (blocks == 0) return TR_OK;                            // no level has a gradient: nothing to write
  hipStream_t st = static_cast<hipStream_t>(s);
  // required traffic of the present levels: every element of a map once at most, every output element once, the index
  tr_prof_note("tr_dense_scatter_levels", 0.0, bytes);
  const int per_image = (int)blocks;                        // (NCHW)
  const dim3 grid((unsigned)(nhwc ? blocks : blocks * B));
#define DS_LAUNCH(IB, OB)                                                                                                                   \
  do {                                                                                                                                      \
    if (nhwc)                                                                                                                               \
      hipLaunchKernelGGL((dense_scatter_levels_nhwc_kernel<IB, OB>), grid, dim3(256), 0, st, lt, L, index, dtokens, level_stride, B, P, D); \
    else                                                                                                                                    \
      hipLaunchKernelGGL((dense_scatter_levels_nchw_kernel<IB, OB>), grid, dim3(256), 0, st, lt, L, index, dtokens, level_stride, B, P, D,  \
                         ctiles, per_image);                                                                                                \
  } while (0)
  if (ib && ob) DS_LAUNCH(true, true);
  else if (ib) DS_LAUNCH(true, false);
  else if (ob) DS_LAUNCH(false, true);
  else DS_LAUNCH(false, false);
#undef DS_LAUNCH
  TR_CHECK_LAUNCH("tr_dense_scatter_levels");
  return TR_OK;
}
