// moments.hip -- additive fp64 feature moments for the Frechet Inception Distance (utils/fid.py):
//   * otgan_moments_update_f64: sum[i] += sum_k x[k][i], outer[i][j] += sum_k x[k][i] x[k][j] for a batch x [n][C] of fp32
//     rows (pool_3 of csrc/inception.hip), in place, so batches stream through it and ranks SUM-reduce the result.
// X^T X on v_mfma_f64_16x16x4_f64.  The inputs are converted to fp64 BEFORE the multiply: a product of two fp32 values
// has 48 significant bits and is exact in fp64, so the only rounding is the fp64 summation over the rows.
// One wave owns a 32 x 32 block of `outer` on or above the diagonal (2 x 2 MFMA tiles; the tile below the diagonal of a
// diagonal block is not computed).  Its accumulators START from the values in memory, the rows run in a fixed order and
// nothing is an atomic: the same sequence of calls gives the same bits.  Every element on or above the diagonal is
// stored to [i][j] and to [j][i], and of a diagonal tile only the elements with i <= j are: `outer` is exactly symmetric.
// The waves of the diagonal blocks also own the column sums of their 32 columns.
// Operand layout of the f64 MFMA: gram64.h, which also has the f64x4 type (its LDS-staged block product is another
// algorithm: here the lanes of a tile are adjacent columns of x and nothing goes through LDS).
#include "gram64.h"
#include "../../include/otgan.h"

namespace {

constexpr int kMomBlock = 32;   // columns of `outer` per wave and side

// One wave's block.  DIAG: bi == bj -- B is A, the tile (1, 0) below the diagonal is skipped, the column sums are kept.
// Loads are unconditional from clamped (always valid) addresses and masked afterwards, so that the compiler can keep
// the loads of several row groups in flight.
template <bool DIAG>
__device__ __forceinline__ void moments_block(int n, int C, long ldx, const float* __restrict__ x, double* __restrict__ sum,
                                              double* __restrict__ outer, int bi, int bj) {
  const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
  int ci[2], cj[2];     // this lane's column of x in the A tiles (rows of outer) and in the B tiles (columns of outer)
  bool oki[2], okj[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    ci[t] = bi * kMomBlock + 16 * t + c;
    cj[t] = bj * kMomBlock + 16 * t + c;
    oki[t] = ci[t] < C;
    okj[t] = cj[t] < C;
  }

  // tile (ti, tj) covers rows i0 = 32 bi + 16 ti, columns j0 = 32 bj + 16 tj; register r of this lane is the element
  // (i0 + g + 4 r, j0 + c)
  f64x4 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = bi * kMomBlock + 16 * ti + g + 4 * r, j = bj * kMomBlock + 16 * tj + c;
        const bool below = DIAG && ti > tj;
        acc[ti][tj][r] = (!below && i < C && j < C) ? outer[(long)i * C + j] : 0.0;
      }

  const float* pa[2] = {x + (oki[0] ? ci[0] : 0), x + (oki[1] ? ci[1] : 0)};
  const float* pb[2] = {x + (okj[0] ? cj[0] : 0), x + (okj[1] ? cj[1] : 0)};
  double colsum[2] = {0.0, 0.0};   // rows g, g + 4, g + 8 ... of columns ci[t]
  // rows k0 + g of x; `masked`: the last, partial group of four (rows past n read row n - 1 and count as zero)
  auto step = [&](int k0, bool masked) {
    const int row = k0 + g;
    const bool rok = !masked || row < n;
    const long off = (long)(rok ? row : n - 1) * ldx;
    double a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float va = pa[t][off];
      a[t] = (rok && oki[t]) ? (double)va : 0.0;
      if (DIAG) {
        b[t] = a[t];
        colsum[t] += a[t];
      } else {
        const float vb = pb[t][off];
        b[t] = (rok && okj[t]) ? (double)vb : 0.0;
      }
    }
    acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[0], acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b[1], acc[0][1], 0, 0, 0);
    if (!DIAG) acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], b[0], acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], b[1], acc[1][1], 0, 0, 0);
  };
  int k0 = 0;
  for (; k0 + 16 <= n; k0 += 16) {
#pragma unroll
    for (int u = 0; u < 4; ++u) step(k0 + 4 * u, false);
  }
  for (; k0 + 4 <= n; k0 += 4) step(k0, false);
  if (k0 < n) step(k0, true);

#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
      if (DIAG && ti > tj) continue;
      const bool dtile = DIAG && ti == tj;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = bi * kMomBlock + 16 * ti + g + 4 * r, j = bj * kMomBlock + 16 * tj + c;
        if (i >= C || j >= C || (dtile && i > j)) continue;
        const double v = acc[ti][tj][r];
        outer[(long)i * C + j] = v;
        if (i != j) outer[(long)j * C + i] = v;
      }
    }

  if (DIAG) {
    // the four row groups g of a column, added in the fixed order ((g0 + g1) + g2) + g3, then onto the value in memory
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      double s = __shfl(colsum[t], c, 64);
#pragma unroll
      for (int q = 1; q < 4; ++q) s += __shfl(colsum[t], c + 16 * q, 64);
      if (g == 0 && oki[t]) sum[ci[t]] += s;
    }
  }
}

// grid (nb, nb), nb = ceil(C / 32); one wave per workgroup; blockIdx.y = block row bi, blockIdx.x = block column bj >= bi
__global__ __launch_bounds__(64) void moments_update_kernel(int n, int C, long ldx, const float* __restrict__ x,
                                                            double* __restrict__ sum, double* __restrict__ outer) {
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  if (bi == bj) moments_block<true>(n, C, ldx, x, sum, outer, bi, bj);
  else moments_block<false>(n, C, ldx, x, sum, outer, bi, bj);
}

}  // namespace

extern "C" {

int otgan_moments_update_f64(int n, int C, int ldx, const float* x, double* sum, double* outer, void* stream) {
  OTGAN_CHECK_ARG(n >= 0 && C > 0 && C % 4 == 0 && ldx >= C,
                  "otgan_moments_update_f64: n %d >= 0, C %d a positive multiple of 4, ldx %d >= C", n, C, ldx);
  OTGAN_CHECK_ARG(sum && outer && (x || n == 0), "otgan_moments_update_f64: null argument");
  OTGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(sum) & 7) == 0 && (reinterpret_cast<uintptr_t>(outer) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(x) & 3) == 0,
                  "otgan_moments_update_f64: misaligned pointer");
  if (n == 0) return OTGAN_OK;
  const int nb = ceil_div(C, kMomBlock);
  OTGAN_CHECK_ARG(nb <= 65535, "otgan_moments_update_f64: C %d too large", C);
  hipLaunchKernelGGL(moments_update_kernel, dim3(nb, nb), dim3(64), 0, (hipStream_t)stream, n, C, (long)ldx, x, sum, outer);
  OTGAN_CHECK_LAUNCH("otgan_moments_update_f64");
  return OTGAN_OK;
}

}  // extern "C"
