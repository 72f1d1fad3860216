// topk.hip -- the nearest neighbours of the critic-feature probe (utils/probe.py), by identity:
//   * otgan_topk_dot_f64: for every query row q_i and the columns y_j with j != self0 + i,
//       index[i][0 .. k) = the columns of the k largest s(q_i, y_j) = q_i . y_j,
//       score[i][0 .. k) = those values,
//     sorted by score descending, equal scores by the smaller column first (-1 and -inf where fewer were counted).
// The third epilogue on the block product of gram64.h, after kid.hip's kernel sums and knn.hip's k smallest distances
// (whose lists are values only: a vote needs to know WHICH columns are nearest): a workgroup of four waves keeps its 64
// query rows, walks the column blocks of its share of the columns, and after each block every lane offers its 8 rows x 2
// columns of dot products to the 8 lists it holds.  The selection -- lists, merges over the 32 lanes that share a row (16
// lanes x the 2 waves of a block row), column split, second launch -- is selectk.h's.
// Order: (score, column) PAIRS,
//       (s, j) before (s', j')  <=>  s > s'  or  (s == s' and j < j'),
// total on the pairs of a row (a column occurs once).  An exchange is two compares and six selects against the
// v_min_f64 / v_max_f64 of knn.hip; 16 values x KL steps per block and lane stay far below the C / 4 x 4 MFMAs per block
// and wave.  A pair is 3 registers: 12 and 24 per row, 96 and 192 per lane for lists of 4 and 8.
// One bit pattern per pair: a.b depends on (a, b, C) only and a.b == b.a, because this kernel runs the one loop of
// gram64.h and nothing else (the order of additions: there).
// Masks: ragged rows, ragged columns and the excluded column are offered as (-inf, kTopkNone): a real column has a finite
// score, and a real column whose score were -inf still has the smaller column number, so a masked entry never displaces
// one (a column number is an int below ny <= 2^31 - 1 = kTopkNone).  kTopkNone leaves as index -1 with score -inf.  A NaN
// score compares false on both legs of the order and is never inserted: inputs must be finite (the header says so).
// Memory: a pair lives in registers only; LDS and the workspace hold scores and columns as two arrays, so the merge of
// the two waves and of the splits are written out here on sel_insert instead of calling sel_merge_waves / sel_merge_splits
// (with pairs stored whole, 12 or 16 bytes, the lists-of-8 kernel came out of the register allocator 5 % slower: 16.6 ->
// 17.5 ms at 1000 x 5000 x 32768, profiles/selectk_ab.txt).
// Workspace: [splits][nq][k] doubles, then [splits][nq][k] int32.
#include <limits>

#include "gram64.h"
#include "selectk.h"
#include "../../include/otgan.h"

namespace {

constexpr int kTopkNone = 0x7fffffff;   // the column of a masked entry: after every real column

// (score, column) pairs: score descending, equal scores by the smaller column
struct TopkPair {
  double s;
  int j;
};

struct TopkOrder {
  typedef TopkPair Entry;
  static __device__ __forceinline__ TopkPair none() { return {-std::numeric_limits<double>::infinity(), kTopkNone}; }
  static __device__ __forceinline__ void exchange(TopkPair& slot, TopkPair& v) {
    const bool first = v.s > slot.s || (v.s == slot.s && v.j < slot.j);
    const double s = slot.s;
    const int j = slot.j;
    slot.s = first ? v.s : s;
    slot.j = first ? v.j : j;
    v.s = first ? s : v.s;
    v.j = first ? j : v.j;
  }
  static __device__ __forceinline__ TopkPair shfl_xor(TopkPair e, int o) {
    return {__shfl_xor(e.s, o, 64), __shfl_xor(e.j, o, 64)};
  }
};

// grid (query blocks, splits), 256 threads.  part_s, part_j: [splits][nq][k].  KL >= k: the length of the lists
template <int KL>
__global__ __launch_bounds__(256, KL <= 4 ? 2 : 1) void topk_block_kernel(int nq, int ny, int C, const float* __restrict__ q, long ldq,
                                                         const float* __restrict__ y, long ldy, int k, int self0, int per,
                                                         double* __restrict__ part_s, int* __restrict__ part_j) {
  __shared__ __attribute__((aligned(16))) Gram64Lds lds;
  __shared__ double wave_s[2][kGramBlock][KL];     // [wj][row of the block][entry]
  __shared__ int wave_j[2][kGramBlock][KL];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int wi = wave >> 1, wj = wave & 1;
  const int bi = blockIdx.x, nbc = (ny + kGramBlock - 1) / kGramBlock;
  const int jb0 = blockIdx.y * per, jb1 = min(jb0 + per, nbc);
  const double ninf = -std::numeric_limits<double>::infinity();

  const float* pa[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) pa[u] = q + (long)gram64_fetch_row(bi, u, nq) * ldq;

  // slot s = 4 ti + r of this lane is row 32 wi + 16 ti + g + 4 r of the block
  TopkPair list[8][KL];
  // the guards as two ints per row, not lane masks (masks live in SGPR pairs and spilled): the columns of a row end at
  // jend (0 for a row past nq: none is counted) and selfj is the excluded one (-1: none; a number >= ny excludes nothing)
  int selfj[8], jend[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int i = bi * kGramBlock + 32 * wi + 16 * (s >> 2) + g + 4 * (s & 3);
    jend[s] = i < nq ? ny : 0;
    selfj[s] = (self0 >= 0 && (long)self0 + i < ny) ? self0 + i : -1;
    sel_fill<TopkOrder>(list[s]);
  }

  for (int jb = jb0; jb < jb1; ++jb) {
    const float* pb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) pb[u] = y + (long)gram64_fetch_row(jb, u, ny) * ldy;
    f64x4 acc[2][2];
    gram64_block_product(C, pa, pb, lds, acc);
    int j[2];
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) j[tj] = jb * kGramBlock + 32 * wj + 16 * tj + c;
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        const bool counted = j[tj] < jend[s] && j[tj] != selfj[s];
        sel_insert<TopkOrder>(list[s], TopkPair{counted ? acc[s >> 2][tj][s & 3] : ninf, counted ? j[tj] : kTopkNone});
      }
  }

  // the 16 lanes c of a wave hold different columns of the same 8 rows
#pragma unroll
  for (int s = 0; s < 8; ++s) sel_merge_lanes<TopkOrder>(list[s], 1, 16);
  if (c == 0) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int row = 32 * wi + 16 * (s >> 2) + g + 4 * (s & 3);
#pragma unroll
      for (int t = 0; t < KL; ++t) {
        wave_s[wj][row][t] = list[s][t].s;
        wave_j[wj][row][t] = list[s][t].j;
      }
    }
  }
  __syncthreads();
  // the two waves of a block row, one thread per row
  const int i = bi * kGramBlock + tid;
  if (tid < kGramBlock && i < nq) {
    TopkPair m[KL];
#pragma unroll
    for (int t = 0; t < KL; ++t) m[t] = TopkPair{wave_s[0][tid][t], wave_j[0][tid][t]};
#pragma unroll
    for (int t = 0; t < KL; ++t) sel_insert<TopkOrder>(m, TopkPair{wave_s[1][tid][t], wave_j[1][tid][t]});
    const long at = ((long)blockIdx.y * nq + i) * k;
#pragma unroll
    for (int t = 0; t < KL; ++t)
      if (t < k) {
        part_s[at + t] = m[t].s;
        part_j[at + t] = m[t].j;
      }
  }
}

// one thread per query row: the first k pairs of its splits' lists (splits == 0: every slot empty); an empty slot
// leaves as (-1, -inf)
__global__ __launch_bounds__(256) void topk_merge_kernel(int nq, int k, int splits, const double* __restrict__ part_s,
                                                         const int* __restrict__ part_j, int* __restrict__ index,
                                                         double* __restrict__ score) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  const double ninf = -std::numeric_limits<double>::infinity();
  TopkPair m[kSelMaxK];
  sel_fill<TopkOrder>(m);
  for (int s = 0; s < splits; ++s) {
    const long at = ((long)s * nq + i) * k;
#pragma unroll
    for (int t = 0; t < kSelMaxK; ++t)
      if (t < k) sel_insert<TopkOrder>(m, TopkPair{part_s[at + t], part_j[at + t]});
  }
#pragma unroll
  for (int t = 0; t < kSelMaxK; ++t)
    if (t < k) {
      const bool none = m[t].j == kTopkNone;
      index[i * k + t] = none ? -1 : m[t].j;
      if (score) score[i * k + t] = none ? ninf : m[t].s;
    }
}

}  // namespace

extern "C" {

size_t otgan_topk_dot_workspace_bytes(int nq, int ny, int k) {
  if (nq <= 0 || ny <= 0 || k < 1 || k > kSelMaxK) return 0;
  const SelPlan p = sel_plan(nq, ny, kGramBlock);
  const size_t slots = (size_t)p.splits * (size_t)nq * (size_t)k;
  const size_t bytes = slots * (sizeof(double) + sizeof(int32_t));
  return (bytes + 7) & ~(size_t)7;
}

int otgan_topk_dot_f64(int nq, int ny, int C, const float* q, int ldq, const float* y, int ldy, int k, int self0,
                       int32_t* index, double* score, void* workspace, size_t workspace_bytes, void* stream) {
  OTGAN_CHECK_ARG(nq >= 0 && ny >= 0 && C > 0 && C % 4 == 0 && ldq >= C && ldy >= C && ldq % 4 == 0 && ldy % 4 == 0,
                  "otgan_topk_dot_f64: nq %d >= 0, ny %d >= 0, C %d a positive multiple of 4, ldq %d and ldy %d >= C and "
                  "multiples of 4", nq, ny, C, ldq, ldy);
  OTGAN_CHECK_ARG(k >= 1 && k <= kSelMaxK && self0 >= -1, "otgan_topk_dot_f64: k %d in 1 ... %d, self0 %d >= -1", k, kSelMaxK, self0);
  OTGAN_CHECK_ARG((index || nq == 0) && (q || nq == 0) && (y || ny == 0), "otgan_topk_dot_f64: null argument");
  OTGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(q) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(index) & 3) == 0 && (reinterpret_cast<uintptr_t>(score) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                  "otgan_topk_dot_f64: misaligned pointer (rows 16 bytes, score and workspace 8, index 4)");
  if (nq == 0) return OTGAN_OK;
  const SelPlan p = sel_plan(nq, ny, kGramBlock);
  if (ny > 0 && (!workspace || workspace_bytes < otgan_topk_dot_workspace_bytes(nq, ny, k))) {
    otgan_set_error("otgan_topk_dot_f64: workspace of %zu bytes, otgan_topk_dot_workspace_bytes(%d, %d, %d) = %zu",
                    workspace_bytes, nq, ny, k, otgan_topk_dot_workspace_bytes(nq, ny, k));
    return OTGAN_ERR_WORKSPACE;
  }
  double* part_s = nullptr;
  int* part_j = nullptr;
  if (ny > 0) {
    part_s = static_cast<double*>(workspace);
    part_j = reinterpret_cast<int*>(part_s + (size_t)p.splits * (size_t)nq * (size_t)k);
    auto kernel = k <= 4 ? topk_block_kernel<4> : topk_block_kernel<kSelMaxK>;
    hipLaunchKernelGGL(kernel, dim3(p.nbq, p.splits), dim3(256), 0, (hipStream_t)stream, nq, ny, C, q, (long)ldq, y,
                       (long)ldy, k, self0, p.per, part_s, part_j);
    OTGAN_CHECK_LAUNCH("otgan_topk_dot_f64");
  }
  hipLaunchKernelGGL(topk_merge_kernel, dim3((nq + 255) / 256), dim3(256), 0, (hipStream_t)stream, nq, k, p.splits,
                     (const double*)part_s, (const int*)part_j, (int*)index, score);
  OTGAN_CHECK_LAUNCH("otgan_topk_dot_f64 (merge)");
  return OTGAN_OK;
}

}  // extern "C"
