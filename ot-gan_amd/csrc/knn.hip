// knn.hip -- fused nearest-neighbour passes for precision, recall, density and coverage (utils/pr.py):
//   * otgan_knn_f64: for every query row q_i and the columns y_j with j != self0 + i,
//       nearest[i][0 .. k) = the k smallest d2(q_i, y_j), ascending (+inf where fewer were counted),
//       inside[i]          = #{ j : d2(q_i, y_j) <= thresh[j] },
//     with d2(a, b) = max(0, (n_a + n_b) - 2 a.b) and n_x = x.x.
// The distance matrix is never written: as in kid.hip a workgroup of four waves forms a 64 x 64 block of the Gram matrix
// with the block product of gram64.h (exact fp32 x fp32 products on the fp64 MFMA) and the epilogue differs: a workgroup
// keeps its 64 query rows, walks the column blocks of its share of the columns, and after each block every lane offers
// its 8 rows x 2 columns of distances to the 8 lists and 8 counters it holds.  The selection -- lists, merges over the 32
// lanes that share a row (16 lanes x the 2 waves of a block row), column split, second launch -- is selectk.h's.
// Order: doubles ascending, an exchange is v_min_f64 / v_max_f64 (16 values x KL steps per block and lane against 2048
// MFMAs per block and wave at C = 2048).  Lists of 8 doubles for 8 rows are 128 registers, which with the 32 of the
// accumulators leave one workgroup per CU; lists of 4 leave two, as the usual k = 3 wants.
// Masks: a masked element (ragged row, ragged column, the excluded column) is offered as +inf and not counted; rows past
// the end read the last row (gram64.h).
// The counts ride along: summed over the lanes beside the tree, over the two waves in LDS, over the splits in the second
// launch.
// One bit pattern per pair: a.b depends on (a, b, C) only and a.b == b.a, because every kernel here and in kid.hip runs
// the one loop of gram64.h (the order of additions: there); the norms are the DIAGONAL of the same block product
// (knn_norm_kernel), so n_x == x.x of that order and d2(a, a) == 0 exactly; n_a + n_b commutes.  Equal distances are
// interchangeable in a list of values and a count is an integer, so the outputs depend neither on the order of the
// columns nor on their split over workgroups.
// Workspace: the norms of q and y, then [splits][nq][k] doubles, then [splits][nq] counts.
#include <limits>

#include "gram64.h"
#include "selectk.h"
#include "../../include/otgan.h"

namespace {

// doubles ascending
struct KnnOrder {
  typedef double Entry;
  static __device__ __forceinline__ double none() { return std::numeric_limits<double>::infinity(); }
  static __device__ __forceinline__ void exchange(double& slot, double& v) {
    const double lo = fmin(slot, v);
    v = fmax(slot, v);
    slot = lo;
  }
  static __device__ __forceinline__ double shfl_xor(double e, int o) { return __shfl_xor(e, o, 64); }
};

// grid (blocks of q + blocks of y), 256 threads: norm[i] = x_i . x_i as the diagonal of the block product of 64 rows with
// themselves -- the bits the distance kernel gets for a row against a copy of itself
__global__ __launch_bounds__(256) void knn_norm_kernel(int nq, int ny, int C, const float* __restrict__ q, long ldq,
                                                       const float* __restrict__ y, long ldy, double* __restrict__ normq,
                                                       double* __restrict__ normy) {
  __shared__ __attribute__((aligned(16))) Gram64Lds lds;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int wi = wave >> 1, wj = wave & 1;
  const int nbq = (nq + kGramBlock - 1) / kGramBlock;
  const bool second = (int)blockIdx.x >= nbq;
  const int b = second ? blockIdx.x - nbq : blockIdx.x, n = second ? ny : nq;
  const float* x = second ? y : q;
  const long ld = second ? ldy : ldq;
  double* norm = second ? normy : normq;
  const float* p[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) p[u] = x + (long)gram64_fetch_row(b, u, n) * ld;
  f64x4 acc[2][2];
  gram64_block_product(C, p, p, lds, acc);
  if (wi != wj) return;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = b * kGramBlock + 32 * wi + 16 * ti + g + 4 * r;
      if (g + 4 * r == c && i < n) norm[i] = acc[ti][ti][r];
    }
}

// grid (query blocks, splits), 256 threads.  part: [splits][nq][k], cnt: [splits][nq].  KL >= k: the length of the lists
template <int KL>
__global__ __launch_bounds__(256, KL <= 4 ? 2 : 1) void knn_block_kernel(int nq, int ny, int C, const float* __restrict__ q, long ldq,
                                                        const float* __restrict__ y, long ldy, int k, int self0,
                                                        const double* __restrict__ normq, const double* __restrict__ normy,
                                                        const double* __restrict__ thresh, int per,
                                                        double* __restrict__ part, int* __restrict__ cnt) {
  __shared__ __attribute__((aligned(16))) Gram64Lds lds;
  __shared__ double wave_list[2][kGramBlock][KL];     // [wj][row of the block][entry]
  __shared__ int wave_cnt[2][kGramBlock];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int wi = wave >> 1, wj = wave & 1;
  const int bi = blockIdx.x, nbc = (ny + kGramBlock - 1) / kGramBlock;
  const int jb0 = blockIdx.y * per, jb1 = min(jb0 + per, nbc);

  const float* pa[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) pa[u] = q + (long)gram64_fetch_row(bi, u, nq) * ldq;

  // slot s = 4 ti + r of this lane is row 32 wi + 16 ti + g + 4 r of the block
  double list[8][KL], nrow[8];
  int count[8];
  long selfj[8];
  bool rowok[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int i = bi * kGramBlock + 32 * wi + 16 * (s >> 2) + g + 4 * (s & 3);
    rowok[s] = i < nq;
    nrow[s] = normq[min(i, nq - 1)];
    selfj[s] = self0 >= 0 ? (long)self0 + i : -1L;          // (no column has number -1)
    count[s] = 0;
    sel_fill<KnnOrder>(list[s]);
  }

  for (int jb = jb0; jb < jb1; ++jb) {
    const float* pb[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) pb[u] = y + (long)gram64_fetch_row(jb, u, ny) * ldy;
    f64x4 acc[2][2];
    gram64_block_product(C, pa, pb, lds, acc);
    int j[2];
    double ncol[2], th[2];
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      j[tj] = jb * kGramBlock + 32 * wj + 16 * tj + c;
      const int jc = min(j[tj], ny - 1);
      ncol[tj] = normy[jc];
      th[tj] = thresh ? thresh[jc] : 0.0;
    }
#pragma unroll
    for (int s = 0; s < 8; ++s)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        const double d2 = fmax(0.0, (nrow[s] + ncol[tj]) - 2.0 * acc[s >> 2][tj][s & 3]);
        const bool counted = rowok[s] && j[tj] < ny && (long)j[tj] != selfj[s];
        sel_insert<KnnOrder>(list[s], counted ? d2 : KnnOrder::none());
        count[s] += (thresh != nullptr && counted && d2 <= th[tj]) ? 1 : 0;
      }
  }

  // the 16 lanes c of a wave hold different columns of the same 8 rows
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    sel_merge_lanes<KnnOrder>(list[s], 1, 16);
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) count[s] += __shfl_xor(count[s], o, 64);
  }
  if (c == 0) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int row = 32 * wi + 16 * (s >> 2) + g + 4 * (s & 3);
#pragma unroll
      for (int t = 0; t < KL; ++t) wave_list[wj][row][t] = list[s][t];
      wave_cnt[wj][row] = count[s];
    }
  }
  __syncthreads();
  // the two waves of a block row, one thread per row
  const int i = bi * kGramBlock + tid;
  if (tid < kGramBlock && i < nq) {
    const long at = (long)blockIdx.y * nq + i;
    sel_merge_waves<KnnOrder>(wave_list[0][tid], wave_list[1][tid], k, part + at * k);
    cnt[at] = wave_cnt[0][tid] + wave_cnt[1][tid];
  }
}

// one thread per query row: the k smallest of its splits' lists and the sum of their counts (splits == 0: +inf and 0)
__global__ __launch_bounds__(256) void knn_merge_kernel(int nq, int k, int splits, const double* __restrict__ part,
                                                        const int* __restrict__ cnt, double* __restrict__ nearest,
                                                        int* __restrict__ inside) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  double m[kSelMaxK];
  sel_merge_splits<KnnOrder>(m, part, i, nq, k, splits);
  int total = 0;
  for (int s = 0; s < splits; ++s) total += cnt[(long)s * nq + i];
#pragma unroll
  for (int t = 0; t < kSelMaxK; ++t)
    if (t < k) nearest[i * k + t] = m[t];
  if (inside) inside[i] = total;
}

inline size_t knn_norm_doubles(int nq, int ny) { return (size_t)nq + (size_t)ny; }

}  // namespace

extern "C" {

size_t otgan_knn_workspace_bytes(int nq, int ny, int k) {
  if (nq <= 0 || ny <= 0 || k < 0 || k > kSelMaxK) return 0;
  const SelPlan p = sel_plan(nq, ny, kGramBlock);
  const size_t rows = (size_t)p.splits * (size_t)nq;
  const size_t bytes = (knn_norm_doubles(nq, ny) + rows * (size_t)k) * sizeof(double) + rows * sizeof(int32_t);
  return (bytes + 7) & ~(size_t)7;
}

int otgan_knn_f64(int nq, int ny, int C, const float* q, int ldq, const float* y, int ldy, int k, int self0,
                  const double* thresh, double* nearest, int32_t* inside, void* workspace, size_t workspace_bytes,
                  void* stream) {
  OTGAN_CHECK_ARG(nq >= 0 && ny >= 0 && C > 0 && C % 4 == 0 && ldq >= C && ldy >= C && ldq % 4 == 0 && ldy % 4 == 0,
                  "otgan_knn_f64: nq %d >= 0, ny %d >= 0, C %d a positive multiple of 4, ldq %d and ldy %d >= C and "
                  "multiples of 4", nq, ny, C, ldq, ldy);
  OTGAN_CHECK_ARG(k >= 0 && k <= kSelMaxK && self0 >= -1, "otgan_knn_f64: k %d in 0 ... %d, self0 %d >= -1", k, kSelMaxK, self0);
  OTGAN_CHECK_ARG((thresh == nullptr) == (inside == nullptr) || (ny == 0 && !thresh),      // (no column: no threshold to point at)
                  "otgan_knn_f64: thresh and inside go together");
  OTGAN_CHECK_ARG((nearest || k == 0 || nq == 0) && (q || nq == 0) && (y || ny == 0), "otgan_knn_f64: null argument");
  OTGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(q) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(thresh) & 7) == 0 && (reinterpret_cast<uintptr_t>(nearest) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(inside) & 3) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                  "otgan_knn_f64: misaligned pointer (rows 16 bytes, thresh, nearest and workspace 8, inside 4)");
  if (nq == 0 || (k == 0 && !inside)) return OTGAN_OK;
  const SelPlan p = sel_plan(nq, ny, kGramBlock);
  if (ny > 0 && (!workspace || workspace_bytes < otgan_knn_workspace_bytes(nq, ny, k))) {
    otgan_set_error("otgan_knn_f64: workspace of %zu bytes, otgan_knn_workspace_bytes(%d, %d, %d) = %zu", workspace_bytes,
                    nq, ny, k, otgan_knn_workspace_bytes(nq, ny, k));
    return OTGAN_ERR_WORKSPACE;
  }
  double* part = nullptr;
  int* cnt = nullptr;
  if (ny > 0) {
    double* normq = static_cast<double*>(workspace);
    double* normy = normq + nq;
    part = normy + ny;
    cnt = reinterpret_cast<int*>(part + (size_t)p.splits * (size_t)nq * (size_t)k);
    hipLaunchKernelGGL(knn_norm_kernel, dim3(p.nbq + p.nbc), dim3(256), 0, (hipStream_t)stream, nq, ny, C, q, (long)ldq, y,
                       (long)ldy, normq, normy);
    OTGAN_CHECK_LAUNCH("otgan_knn_f64 (norms)");
    auto kernel = k <= 4 ? knn_block_kernel<4> : knn_block_kernel<kSelMaxK>;
    hipLaunchKernelGGL(kernel, dim3(p.nbq, p.splits), dim3(256), 0, (hipStream_t)stream, nq, ny, C, q, (long)ldq, y,
                       (long)ldy, k, self0, (const double*)normq, (const double*)normy, thresh, p.per, part, cnt);
    OTGAN_CHECK_LAUNCH("otgan_knn_f64");
  }
  hipLaunchKernelGGL(knn_merge_kernel, dim3((nq + 255) / 256), dim3(256), 0, (hipStream_t)stream, nq, k, p.splits,
                     (const double*)part, (const int*)cnt, nearest, (int*)inside);
  OTGAN_CHECK_LAUNCH("otgan_knn_f64 (merge)");
  return OTGAN_OK;
}

}  // extern "C"
