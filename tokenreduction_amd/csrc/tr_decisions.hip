// Decision taps (tr_stage_decisions): the raw per-stage index slabs of an eval forward (kept_idx / compl_idx / soft_out of tr_vit_forward)
// turned into what the reference's validate.py stores per image in its `Stage-{loc}` records (validate.py:199-229):
//   kept     the composed ABSOLUTE patch indices of the input grid after every stage (Kept_Token): stage-relative indices pushed through
//            the previous stage's list
//   assign   the stage's Assignment_Maps row, stage-relative as the reference stores it: copied (DPC-KNN, K-Medoids), rebuilt from
//            ToMe's (unm, src, dst) (tome.py:91-99), or the argmax over a written soft matrix (sit.py:122)
// One launch per forward, one workgroup of 256 threads per image, the stages walked in block order.  The previous stage's composed list
// stays in LDS (two lists of at most 1024 entries), ToMe's position table in a third.  Pure index shuffling: 4-byte loads and stores,
// consecutive lanes on consecutive elements.  Every index is compared with the length of the list it is about to index BEFORE the read; one
// that is neither valid nor a documented padding value comes out as -2, never as an access out of range.
#include "tr_common.h"

namespace {

constexpr int DEC_THREADS = 256;
constexpr int DEC_MAX_LIST = 1024;       // N0 <= 1025: at most 1024 patch tokens enter a stage
constexpr int DEC_BAD = -2;

struct dec_table {
  tr_decision_stage st[TR_MAX_DECISION_STAGES];
  int n;
};

// exclusive prefix count of `flag` over the workgroup's 256 threads, in thread order, and the total: ballots inside a wave, four
// wave totals through LDS
__device__ __forceinline__ int block_prefix_count(bool flag, int* wave_tot, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b = __ballot(flag);
  const int before = __popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();                                   // (wave_tot of the previous round has been read)
  if (lane == 0) wave_tot[wave] = __popcll(b);
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < DEC_THREADS / 64; ++w) {
    const int t = wave_tot[w];
    if (w < wave) base += t;
    tot += t;
  }
  total = tot;
  return base + before;
}

__global__ __launch_bounds__(DEC_THREADS) void stage_decisions_kernel(const int32_t* __restrict__ kept_idx, const int32_t* __restrict__ compl_idx,
                                                                      const float* __restrict__ soft, dec_table tab, int B, int N0,
                                                                      int32_t* __restrict__ kept_out, int32_t* __restrict__ count_out,
                                                                      int32_t* __restrict__ assign_out) {
  __shared__ int list[2][DEC_MAX_LIST + 1];        // (EViT: k + 1 <= n_in entries)
  __shared__ int pos_a[DEC_MAX_LIST / 2 + 1];
  __shared__ int wave_tot[DEC_THREADS / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  int cur = 0;             // list[cur]: the previous stage's composed list
  int prev_len = -1;       // its length; -1: no stage yet, the list is the input grid itself (0 ... n_in-2)
  for (int s = 0; s < tab.n; ++s) {
    const tr_decision_stage st = tab.st[s];
    const size_t slab = (size_t)st.block * B * N0;
    const int n_in = st.n_in, k = st.k, kind = st.kind;
    if (kind == TR_DECISION_PRUNE || kind == TR_DECISION_EVIT || kind == TR_DECISION_CENTRES) {
      // rel [B, k] -> prev[rel]; EViT: one trailing -1 (the fused token, evit.py:123), and -1 indexes it (numpy's last element)
      const int len = prev_len < 0 ? n_in - 1 : prev_len;
      const int* prev = list[cur];
      int* next = list[cur ^ 1];
      const int W = kind == TR_DECISION_EVIT ? k + 1 : k;
      int32_t* out = kept_out + st.kept_off + (size_t)b * W;
      for (int j = tid; j < W; j += DEC_THREADS) {
        int v = -1;
        if (j < k) {
          const int rel = kept_idx[slab + (size_t)b * k + j];
          if (rel >= 0 && rel < len) v = prev_len < 0 ? rel : prev[rel];
          else v = (kind == TR_DECISION_EVIT && rel == -1) ? -1 : DEC_BAD;
        }
        next[j] = v;
        out[j] = v;
      }
      if (tid == 0) count_out[(size_t)s * B + b] = W;
      if (kind == TR_DECISION_CENTRES) {
        const int P = n_in - 1;
        int32_t* a = assign_out + st.assign_off + (size_t)b * P;
        for (int p = tid; p < P; p += DEC_THREADS) a[p] = compl_idx[slab + (size_t)b * P + p];
      }
      __syncthreads();
      cur ^= 1;
      prev_len = W;
    } else if (kind == TR_DECISION_ATS) {
      // ids [B, k]: column 0 the CLS id, 1-based ids behind it, 0 = padding
      const int W = k - 1;
      const int* prev = list[cur];
      int* next = list[cur ^ 1];
      int32_t* out = kept_out + st.kept_off + (size_t)b * W;
      const int32_t* ids = kept_idx + slab + (size_t)b * k + 1;
      if (prev_len < 0) {
        // first stage: rel as is, padding as -1 (the record keeps its padding: validate.py:205)
        int count = 0;
        for (int j0 = 0; j0 < W; j0 += DEC_THREADS) {
          const int j = j0 + tid;
          const int id = j < W ? ids[j] : 0;
          int v = -1;
          if (id != 0) v = (id >= 1 && id - 1 < n_in - 1) ? id - 1 : DEC_BAD;
          if (j < W) {
            next[j] = v;
            out[j] = v;
          }
          int tot;
          block_prefix_count(id != 0, wave_tot, tot);
          count += tot;
        }
        if (tid == 0) count_out[(size_t)s * B + b] = count;
        __syncthreads();
        prev_len = W;
      } else {
        // later stages: the padding is dropped, order preserved (validate.py:213-214), then prev[rel]
        int count = 0;
        for (int j0 = 0; j0 < W; j0 += DEC_THREADS) {
          const int j = j0 + tid;
          const int id = j < W ? ids[j] : 0;
          int tot;
          const int pos = count + block_prefix_count(id != 0, wave_tot, tot);
          if (id != 0) next[pos] = (id >= 1 && id - 1 < prev_len) ? prev[id - 1] : DEC_BAD;
          count += tot;
        }
        __syncthreads();
        for (int j = tid; j < W; j += DEC_THREADS) out[j] = j < count ? next[j] : -1;
        if (tid == 0) count_out[(size_t)s * B + b] = count;
        prev_len = count;
      }
      cur ^= 1;
    } else if (kind == TR_DECISION_TOME) {
      // (unm [B, na-r], src [B, r], dst [B, r]) -> the output token of every input patch token, minus 1 (tome.py:91-99)
      const int na = (n_in + 1) / 2, nb = n_in / 2;
      const int r = min(k, (n_in - 1) / 2);
      const int32_t* unm = kept_idx + slab + (size_t)b * (na - r);
      const int32_t* src = kept_idx + slab + (size_t)B * (na - r) + (size_t)b * r;
      const int32_t* dst = kept_idx + slab + (size_t)B * na + (size_t)b * r;
      for (int j = tid; j < na; j += DEC_THREADS) pos_a[j] = DEC_BAD + 1;          // an entry nobody claims: -2 in the map
      __syncthreads();
      for (int j = tid; j < na - r; j += DEC_THREADS) {
        const int u = unm[j];
        if (u >= 0 && u < na) pos_a[u] = j;
      }
      for (int j = tid; j < r; j += DEC_THREADS) {
        const int u = src[j], d = dst[j];
        if (u >= 0 && u < na) pos_a[u] = (d >= 0 && d < nb) ? (na - r) + d : DEC_BAD + 1;
      }
      __syncthreads();
      int32_t* a = assign_out + st.assign_off + (size_t)b * (n_in - 1);
      for (int p = 1 + tid; p < n_in; p += DEC_THREADS) a[p - 1] = ((p & 1) ? (na - r) + (p >> 1) : pos_a[p >> 1]) - 1;
      if (tid == 0) count_out[(size_t)s * B + b] = 0;
      __syncthreads();                                  // (pos_a is reused by the next ToMe stage)
    } else {
      // TR_DECISION_SOFT: argmax over the k rows of soft[b] ([k, P] fp32), the first maximum wins and a NaN counts as one (numpy)
      const int P = n_in - 1;
      const float* sm = soft + st.soft_off + (size_t)b * k * P;
      int32_t* a = assign_out + st.assign_off + (size_t)b * P;
      for (int p = tid; p < P; p += DEC_THREADS) {
        float best = sm[p];
        int arg = 0;
        for (int c = 1; c < k; ++c) {
          const float v = sm[(size_t)c * P + p];
          if (v > best || (v != v && best == best)) {
            best = v;
            arg = c;
          }
        }
        a[p] = arg;
      }
      if (tid == 0) count_out[(size_t)s * B + b] = 0;
    }
  }
}

}  // namespace

extern "C" int tr_stage_decisions(const int32_t* kept_idx, const int32_t* compl_idx, size_t idx_elems, const float* soft, size_t soft_elems,
                                  const tr_decision_stage* stages, int n_stages, int B, int N0, int32_t* kept_out, size_t kept_elems,
                                  int32_t* count_out, int32_t* assign_out, size_t assign_elems, tr_stream_t s) {
  TR_REQUIRE(n_stages >= 0 && n_stages <= TR_MAX_DECISION_STAGES, TR_ERR_CONFIG, "tr_stage_decisions: %d stages (at most %d)", n_stages,
             TR_MAX_DECISION_STAGES);
  if (n_stages == 0) return TR_OK;                                       // a model without a device-side stage: no launch
  TR_REQUIRE(stages && kept_idx && count_out, TR_ERR_NULL, "tr_stage_decisions: null pointer");
  TR_REQUIRE(B > 0 && N0 >= 2 && N0 <= DEC_MAX_LIST + 1, TR_ERR_SHAPE, "tr_stage_decisions: need B > 0 and 2 <= N0 <= 1025 (B=%d N0=%d)", B, N0);
  dec_table tab;
  tab.n = n_stages;
  int last_block = -1;
  for (int i = 0; i < n_stages; ++i) {
    const tr_decision_stage& st = stages[i];
    TR_REQUIRE(st.kind >= TR_DECISION_PRUNE && st.kind <= TR_DECISION_SOFT, TR_ERR_CONFIG, "tr_stage_decisions: stage %d has kind %d", i, st.kind);
    TR_REQUIRE(st.block > last_block && st.block < TR_MAX_DEPTH, TR_ERR_CONFIG,
               "tr_stage_decisions: stage %d names block %d (ascending blocks below %d)", i, st.block, TR_MAX_DEPTH);
    last_block = st.block;
    TR_REQUIRE(((size_t)st.block + 1) * B * N0 <= idx_elems, TR_ERR_SHAPE, "tr_stage_decisions: stage %d: the slab of block %d leaves the index buffers (%zu elements)",
               i, st.block, idx_elems);
    TR_REQUIRE(st.n_in >= 2 && st.n_in <= N0 && st.k >= 1 && st.k < st.n_in, TR_ERR_SHAPE,
               "tr_stage_decisions: stage %d needs 2 <= n_in <= N0 and 1 <= k < n_in (n_in=%d k=%d N0=%d)", i, st.n_in, st.k, N0);
    const size_t P = (size_t)st.n_in - 1;
    size_t kept_w = 0, assign_w = 0;
    if (st.kind == TR_DECISION_PRUNE || st.kind == TR_DECISION_CENTRES) kept_w = st.k;
    else if (st.kind == TR_DECISION_EVIT) kept_w = (size_t)st.k + 1;
    else if (st.kind == TR_DECISION_ATS) kept_w = (size_t)st.k - 1;
    if (st.kind == TR_DECISION_CENTRES || st.kind == TR_DECISION_TOME || st.kind == TR_DECISION_SOFT) assign_w = P;
    TR_REQUIRE(st.kind != TR_DECISION_ATS || st.k >= 2, TR_ERR_SHAPE, "tr_stage_decisions: stage %d: an ATS stage needs k >= 2", i);
    if (kept_w) {
      TR_REQUIRE(kept_out, TR_ERR_NULL, "tr_stage_decisions: stage %d writes a kept list, kept_out is NULL", i);
      TR_REQUIRE(st.kept_off >= 0 && (size_t)st.kept_off + (size_t)B * kept_w <= kept_elems, TR_ERR_SHAPE,
                 "tr_stage_decisions: stage %d: kept list [%d, %zu] at %lld leaves kept_out (%zu elements)", i, B, kept_w,
                 (long long)st.kept_off, kept_elems);
    }
    if (assign_w) {
      TR_REQUIRE(assign_out, TR_ERR_NULL, "tr_stage_decisions: stage %d writes an assignment map, assign_out is NULL", i);
      TR_REQUIRE(st.assign_off >= 0 && (size_t)st.assign_off + (size_t)B * assign_w <= assign_elems, TR_ERR_SHAPE,
                 "tr_stage_decisions: stage %d: map [%d, %zu] at %lld leaves assign_out (%zu elements)", i, B, assign_w,
                 (long long)st.assign_off, assign_elems);
    }
    if (st.kind == TR_DECISION_CENTRES) TR_REQUIRE(compl_idx, TR_ERR_NULL, "tr_stage_decisions: stage %d needs compl_idx", i);
    if (st.kind == TR_DECISION_SOFT) {
      TR_REQUIRE(soft, TR_ERR_NULL, "tr_stage_decisions: stage %d needs the soft-assignment buffer", i);
      TR_REQUIRE(st.soft_off >= 0 && (size_t)st.soft_off + (size_t)B * st.k * P <= soft_elems, TR_ERR_SHAPE,
                 "tr_stage_decisions: stage %d: soft block [%d, %d, %zu] at %lld leaves the buffer (%zu elements)", i, B, st.k, P,
                 (long long)st.soft_off, soft_elems);
    }
    tab.st[i] = st;
  }
  TR_REQUIRE(tr_aligned16(kept_idx) && tr_aligned16(compl_idx) && tr_aligned16(soft) && tr_aligned16(kept_out) && tr_aligned16(count_out) &&
                 tr_aligned16(assign_out),
             TR_ERR_ALIGN, "tr_stage_decisions: pointers must be 16-byte aligned");
  hipStream_t st = static_cast<hipStream_t>(s);
  tr_prof_note("tr_stage_decisions", 0.0, 8.0 * B * N0 * n_stages);
  hipLaunchKernelGGL(stage_decisions_kernel, dim3(B), dim3(DEC_THREADS), 0, st, kept_idx, compl_idx, soft, tab, B, N0, kept_out, count_out,
                     assign_out);
  TR_CHECK_LAUNCH("tr_stage_decisions");
  return TR_OK;
}
