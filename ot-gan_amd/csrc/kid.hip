// kid.hip -- fused kernel sums for the Kernel Inception Distance (utils/kid.py):
//   * otgan_kid_sums_f64: for every subset s, with X_i = x[xi[s][i]], Y_j = y[yi[s][j]] (m rows each, fp32, C channels) and the
//     cubic kernel k(a, b) = (a.b / C + 1)^3,
//       out[s][0] = sum_{i != j} k(X_i, X_j),   out[s][1] = sum_{i != j} k(Y_i, Y_j),   out[s][2] = sum_{i, j} k(X_i, Y_j).
// The three Gram matrices are only ever summed, so none is written: a workgroup of four waves owns a 64 x 64 block of one
// Gram -- the block product of gram64.h (exact fp32 x fp32 products on the fp64 MFMA, operands through LDS) -- applies the
// affine map and the cube to its accumulators in registers and leaves ONE double; the map, the cube and all sums are fp64.
// Blocks: of the two symmetric Grams only the blocks on or above the diagonal exist.  A strictly upper block counts twice
// (its mirror image is never computed); a diagonal block is computed whole -- both (i, j) and (j, i) of its pairs, once each
// -- and drops i == j, BY POSITION in the index list: a row number that occurs twice is two rows.  The cross Gram has all
// nb x nb blocks and no excluded diagonal.
// Ragged edges: rows past m read row m - 1 of the list (gram64.h) and are masked where the kernel value is summed.
// Deterministic: no atomics.  Lanes, waves and workgroups are added in a fixed order: the per-workgroup doubles go to
// workspace[s][block] and a second launch adds the blocks of each (subset, output) in a fixed order.  A subset's value
// does not depend on nsub or on its place in the call.
#include "gram64.h"
#include "../../include/otgan.h"

namespace {

// blocks per subset: nb (nb + 1) / 2 of each symmetric Gram and nb^2 of the cross Gram
__host__ __device__ inline long kid_blocks(int m) {
  const long nb = (m + kGramBlock - 1) / kGramBlock;
  return nb * (nb + 1) + nb * nb;
}

// grid (kid_blocks(m), nsub), 256 threads.  blockIdx.x: first the upper blocks of X X^T row by row, then those of Y Y^T,
// then the blocks of X Y^T.
__global__ __launch_bounds__(256) void kid_block_kernel(int m, int C, const float* __restrict__ x, long ldx,
                                                        const int* __restrict__ xi, const float* __restrict__ y, long ldy,
                                                        const int* __restrict__ yi, double* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) Gram64Lds lds;
  __shared__ double wave_part[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int s = blockIdx.y;
  const int nb = (m + kGramBlock - 1) / kGramBlock, tri = nb * (nb + 1) / 2;
  int t = blockIdx.x, which, bi, bj;
  if (t < 2 * tri) {
    which = t < tri ? 0 : 1;
    t -= which * tri;
    bi = 0;
    while (t >= nb - bi) {
      t -= nb - bi;
      ++bi;
    }
    bj = bi + t;
  } else {
    which = 2;
    t -= 2 * tri;
    bi = t / nb;
    bj = t - bi * nb;
  }
  const float* abase = which == 1 ? y : x;
  const float* bbase = which == 0 ? x : y;
  const long lda = which == 1 ? ldy : ldx, ldb = which == 0 ? ldx : ldy;
  const int* aidx = (which == 1 ? yi : xi) + (long)s * m;
  const int* bidx = (which == 0 ? xi : yi) + (long)s * m;

  const float* pa[2];
  const float* pb[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    pa[u] = abase + (long)aidx[gram64_fetch_row(bi, u, m)] * lda;
    pb[u] = bbase + (long)bidx[gram64_fetch_row(bj, u, m)] * ldb;
  }
  f64x4 acc[2][2];
  gram64_block_product(C, pa, pb, lds, acc);

  // k = (g / C + 1)^3 of the counted pairs, added in a fixed order: registers, lanes (xor tree), waves; tile (ti, tj)
  // register r of this lane is the element (32 wi + 16 ti + g + 4 r, 32 wj + 16 tj + c) of the block
  const int wi = wave >> 1, wj = wave & 1;
  const double dC = (double)C;
  const bool drop_diag = which < 2;        // (i == j occurs in diagonal blocks only)
  double sum = 0.0;
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = bi * kGramBlock + 32 * wi + 16 * ti + g + 4 * r, j = bj * kGramBlock + 32 * wj + 16 * tj + c;
        const double v = acc[ti][tj][r] / dC + 1.0;
        const bool counted = i < m && j < m && !(drop_diag && i == j);
        sum += counted ? v * v * v : 0.0;
      }
  sum = wave_sum_d(sum);
  if (lane == 0) wave_part[wave] = sum;
  __syncthreads();
  if (tid == 0) {
    const double v = ((wave_part[0] + wave_part[1]) + wave_part[2]) + wave_part[3];
    partial[(long)s * gridDim.x + blockIdx.x] = (which < 2 && bj > bi) ? 2.0 * v : v;
  }
}

// grid (nsub), 192 threads: wave w adds the blocks of output w of its subset -- each lane every 64th block in rising
// order, then the xor tree over the lanes
__global__ __launch_bounds__(192) void kid_reduce_kernel(int m, const double* __restrict__ partial, double* __restrict__ out) {
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long nb = (m + kGramBlock - 1) / kGramBlock, tri = nb * (nb + 1) / 2, total = 2 * tri + nb * nb;
  const long lo = w * tri, hi = w == 2 ? total : lo + tri;
  const double* p = partial + (long)blockIdx.x * total;
  double sum = 0.0;
  for (long b = lo + lane; b < hi; b += 64) sum += p[b];
  sum = wave_sum_d(sum);
  if (lane == 0) out[(long)blockIdx.x * 3 + w] = sum;
}

}  // namespace

extern "C" {

size_t otgan_kid_workspace_bytes(int nsub, int m) {
  if (nsub <= 0 || m < 2) return 0;
  return (size_t)nsub * (size_t)kid_blocks(m) * sizeof(double);
}

int otgan_kid_sums_f64(int nsub, int m, int C, const float* x, int ldx, const int32_t* xi, const float* y, int ldy,
                       const int32_t* yi, double* out, void* workspace, size_t workspace_bytes, void* stream) {
  OTGAN_CHECK_ARG(nsub >= 0 && m >= 2 && C > 0 && C % 4 == 0 && ldx >= C && ldy >= C && ldx % 4 == 0 && ldy % 4 == 0,
                  "otgan_kid_sums_f64: nsub %d >= 0, m %d >= 2, C %d a positive multiple of 4, ldx %d and ldy %d >= C and "
                  "multiples of 4", nsub, m, C, ldx, ldy);
  OTGAN_CHECK_ARG(out && ((x && xi && y && yi) || nsub == 0), "otgan_kid_sums_f64: null argument");
  OTGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 7) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(y) & 15) == 0 && (reinterpret_cast<uintptr_t>(xi) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(yi) & 3) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                  "otgan_kid_sums_f64: misaligned pointer (rows 16 bytes, out and workspace 8, indices 4)");
  if (nsub == 0) return OTGAN_OK;
  const long blocks = kid_blocks(m);
  OTGAN_CHECK_ARG(nsub <= 65535 && blocks <= 2147483647L,
                  "otgan_kid_sums_f64: nsub %d (at most 65535 per call) or m %d too large for one grid", nsub, m);
  if (!workspace || workspace_bytes < otgan_kid_workspace_bytes(nsub, m)) {
    otgan_set_error("otgan_kid_sums_f64: workspace of %zu bytes, otgan_kid_workspace_bytes(%d, %d) = %zu", workspace_bytes,
                    nsub, m, otgan_kid_workspace_bytes(nsub, m));
    return OTGAN_ERR_WORKSPACE;
  }
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(kid_block_kernel, dim3((unsigned)blocks, nsub), dim3(256), 0, (hipStream_t)stream, m, C, x, (long)ldx,
                     (const int*)xi, y, (long)ldy, (const int*)yi, partial);
  OTGAN_CHECK_LAUNCH("otgan_kid_sums_f64");
  hipLaunchKernelGGL(kid_reduce_kernel, dim3(nsub), dim3(192), 0, (hipStream_t)stream, m, (const double*)partial, out);
  OTGAN_CHECK_LAUNCH("otgan_kid_sums_f64 (reduce)");
  return OTGAN_OK;
}

}  // extern "C"
