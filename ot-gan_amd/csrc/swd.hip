// swd.hip -- the sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018, "Progressive Growing of GANs",
// section 5; utils/swd.py): the pyramid of a uint8 image, the per-channel statistics of the 7 x 7 x 3 patch descriptors and
// their projections on given directions (otgan_swd_pyramid_u8 / otgan_swd_channel_stats_u8 / otgan_swd_project_u8; the
// formulas are stated in include/otgan_layers.h), and the L1 distance of two sorted rows (otgan_swd_row_l1_f64).
//
// One workgroup of 256 threads per image in every image kernel.  The image is read from global memory ONCE, as 4-byte words,
// and its whole pyramid is built in LDS by one device function, build_pyramid -- as fp32 for the pyramid and the projection
// entries, whose levels therefore have the same bits, and as fp64 for the statistics (below).  At S = 64 the fp32 pyramid is
// 48 + 12 + 3 KiB; `pyr[i - 1] -= up(pyr[i])` runs in place (up reads pyr[i] only), so there is no temporary.  Patches are
// gathered from LDS and the descriptor matrix -- 1.2 GB per level and set at the paper's sizes -- never exists: a lane holds the
// 147 normalised values of ONE patch in registers.
//
// Arithmetic of the pyramid.  The taps are dyadic, so a 5 x 5 sum is accumulated with the INTEGER weights g[dy] g[dx]
// (1 4 6 4 1) in the fixed order dy outer, dx inner and scaled once, by 1/256 (down) or 4/256 (up).  With uint8 inputs every
// stage is exact in fp32 except up() of the 16 x 16 level at S = 64, whose numerators need 30 bits (measured against fp64:
// 2.1e-5 at |v| <= 255); every value of every level is a multiple of 2^-22 below 256, so the same code in fp64 is exact throughout.
//
// Projections: lanes run along the patches p of the image, a wave takes four directions j at a time (four independent
// accumulators), and each sum runs e = 0 ... 146 in order with one fma per element: the bits of proj[j][i P + p] depend on the
// image, its positions, mean / inv_std and dirs[j] alone -- not on n, nd, the wave that computed it or what shared the launch.
// dirs[j][e] is wave-uniform and travels in scalar registers; a direction's P outputs of an image leave as one contiguous row
// segment, 256 B per wave store.
//
// Statistics: the mean of a Laplacian level is a small difference of large sums, and the 2e-5 of the fp32 pyramid showed in it
// at 3.7e-5 relative.  The statistics kernel therefore builds its pyramid in fp64 (126 KiB of LDS at S = 64, one workgroup
// per CU -- it runs once per set and evaluation), where every level is exact.  Per image, fp64 sums of x and x^2 over the patch
// elements in a fixed order (a fixed sequence per thread, the wave butterfly, (w0 + w1) + (w2 + w3)) go to the workspace.  The
// finishing launch adds the images' sums EXACTLY, as integers: a sum of x is a multiple of 2^-22 and a sum of x^2 a multiple of
// 2^-44 (rounding in fp64 only coarsens), so both are scaled to integers -- the latter split into a high part and a low 32-bit
// part -- and added in int64.  Integer addition is associative: the result does not depend on the order of the images, let
// alone on how they are spread over threads.  No atomics.
#include "common.h"
#include "../../include/otgan.h"
#include "../../include/otgan_layers.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPatch = 7;
constexpr int kDesc = 3 * kPatch * kPatch;   // 147
constexpr int kDirsPerPass = 4;              // directions a wave carries through one pass over a patch's 147 values
constexpr long kMaxPatchesTotal = 1L << 27;  // n * P: keeps the integer sums of the finishing launch inside int64

__host__ __device__ inline int swd_levels(int S) { return S == 16 ? 1 : (S == 32 ? 2 : (S == 64 ? 3 : 0)); }
__host__ __device__ inline int level_offset(int S, int l) {     // floats in front of level l
  int off = 0;
  for (int i = 0; i < l; ++i) off += 3 * (S >> i) * (S >> i);
  return off;
}

// mirror without repeating the edge pixel: -1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3 (|overhang| <= 2 < n)
__device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

__device__ __forceinline__ float tap(int k) { return k == 2 ? 6.0f : ((k == 1 || k == 3) ? 4.0f : 1.0f); }
__device__ __forceinline__ float mad(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double mad(double a, double b, double c) { return fma(a, b, c); }

// dst [s/2][s/2][3] = (g * src)[::2, ::2], src [s][s][3]
template <typename T>
__device__ void pyr_down(const T* src, int s, T* dst) {
  const int h = s >> 1;
  for (int o = threadIdx.x; o < 3 * h * h; o += kThreads) {
    const int c = o % 3, x = (o / 3) % h, y = o / (3 * h);
    T acc = (T)0;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
      const T* row = src + mirror(2 * y + dy - 2, s) * 3 * s + c;
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) acc = mad((T)(tap(dy) * tap(dx)), row[3 * mirror(2 * x + dx - 2, s)], acc);
    }
    dst[o] = acc * (T)(1.0f / 256.0f);
  }
}

// dst [s][s][3] -= (4 g) * z, z = src [s/2][s/2][3] on the even pixels of a zero s x s image.  The mirror keeps parity, so the
// taps that meet a non-zero of z are those with y + dy and x + dx even.
template <typename T>
__device__ void pyr_sub_up(const T* src, int s, T* dst) {
  const int h = s >> 1;
  for (int o = threadIdx.x; o < 3 * s * s; o += kThreads) {
    const int c = o % 3, x = (o / 3) % s, y = o / (3 * s);
    T acc = (T)0;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
      const int yy = y + dy - 2;
      if (yy & 1) continue;
      const T* row = src + (mirror(yy, s) >> 1) * 3 * h + c;
#pragma unroll
      for (int dx = 0; dx < 5; ++dx) {
        const int xx = x + dx - 2;
        if (xx & 1) continue;
        acc = mad((T)(tap(dy) * tap(dx)), row[3 * (mirror(xx, s) >> 1)], acc);
      }
    }
    dst[o] -= acc * (T)(4.0f / 256.0f);
  }
}

// the whole pyramid of one uint8 image [S][S][3] in s_pyr (level l at level_offset(S, l)); every thread of the workgroup calls it
template <typename T>
__device__ void build_pyramid(const uint8_t* __restrict__ img, int S, T* s_pyr) {
  const int words = 3 * S * S / 4;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(img);
  for (int q = threadIdx.x; q < words; q += kThreads) {
    const uint32_t v = w[q];
    s_pyr[4 * q] = (T)(v & 0xffu);
    s_pyr[4 * q + 1] = (T)((v >> 8) & 0xffu);
    s_pyr[4 * q + 2] = (T)((v >> 16) & 0xffu);
    s_pyr[4 * q + 3] = (T)(v >> 24);
  }
  __syncthreads();
  const int L = swd_levels(S);
  for (int i = 1; i < L; ++i) {
    T* fine = s_pyr + level_offset(S, i - 1);
    T* coarse = s_pyr + level_offset(S, i);
    pyr_down(fine, S >> (i - 1), coarse);
    __syncthreads();
    pyr_sub_up(coarse, S >> (i - 1), fine);
    __syncthreads();
  }
}

__global__ __launch_bounds__(kThreads) void swd_pyramid_kernel(const uint8_t* __restrict__ img, int S, int level,
                                                              float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const long i = blockIdx.x;
  build_pyramid(img + i * 3 * S * S, S, s_mem);
  const int sl = S >> level, quads = 3 * sl * sl / 4;
  const float* src = s_mem + level_offset(S, level);
  float* dst = out + i * 3 * sl * sl;
  for (int q = threadIdx.x; q < quads; q += kThreads)
    *reinterpret_cast<f32x4*>(dst + 4 * q) = *reinterpret_cast<const f32x4*>(src + 4 * q);
}

// top-left corner of patch p of image i at level l, kept inside the level whatever the caller passed
__device__ __forceinline__ void patch_corner(const int32_t* __restrict__ pos, long n, int P, int l, long i, int p, int sl,
                                             int* y, int* x) {
  const int32_t* q = pos + (((long)l * n + i) * P + p) * 2;
  *y = min(max(q[0], 0), sl - kPatch);
  *x = min(max(q[1], 0), sl - kPatch);
}

// partial: double [n][L][6] = per channel (sum x, sum x^2) over the image's P patches of level l
__global__ __launch_bounds__(kThreads) void swd_stats_partial_kernel(const uint8_t* __restrict__ img, long n, int S,
                                                                    const int32_t* __restrict__ pos, int P,
                                                                    double* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) double s_pyr64[];
  __shared__ double s_red[4][6];
  const long i = blockIdx.x;
  build_pyramid(img + i * 3 * S * S, S, s_pyr64);
  const int L = swd_levels(S);
  for (int l = 0; l < L; ++l) {
    const int sl = S >> l;
    const double* lev = s_pyr64 + level_offset(S, l);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < P; p += kThreads) {
      int y0, x0;
      patch_corner(pos, n, P, l, i, p, sl, &y0, &x0);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double sx = 0.0, sxx = 0.0;
        for (int dy = 0; dy < kPatch; ++dy) {
          const double* row = lev + ((y0 + dy) * sl + x0) * 3 + c;
#pragma unroll
          for (int dx = 0; dx < kPatch; ++dx) {
            const double v = row[3 * dx];
            sx += v;
            sxx += v * v;
          }
        }
        acc[2 * c] += sx;
        acc[2 * c + 1] += sxx;
      }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double v = wave_sum_d(acc[k]);
      if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 6)
      partial[(i * L + l) * 6 + threadIdx.x] =
          (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
    __syncthreads();
  }
}

// one workgroup per (level, channel): the exact integer sum of the images' partial sums, then mean and 1 / std in fp64
__global__ __launch_bounds__(kThreads) void swd_stats_finish_kernel(const double* __restrict__ partial, long n, int L, int P,
                                                                   float* __restrict__ mean, float* __restrict__ inv_std) {
  __shared__ long long s_acc[kThreads][3];
  const int l = blockIdx.x / 3, c = blockIdx.x % 3;
  long long ax = 0, ahi = 0, alo = 0;
  for (long i = threadIdx.x; i < n; i += kThreads) {
    const double* q = partial + (i * L + l) * 6 + 2 * c;
    ax += __double2ll_rn(q[0] * 4194304.0);                    // 2^22
    const double v = q[1] * 17592186044416.0;                  // 2^44: an integer below 2^73
    const double hi = floor(v * (1.0 / 4294967296.0));
    ahi += (long long)hi;
    alo += (long long)(v - hi * 4294967296.0);
  }
  s_acc[threadIdx.x][0] = ax; s_acc[threadIdx.x][1] = ahi; s_acc[threadIdx.x][2] = alo;
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s_acc[threadIdx.x][k] += s_acc[threadIdx.x + h][k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double N = (double)n * (double)P * (double)(kPatch * kPatch);
    const double sx = (double)s_acc[0][0] * (1.0 / 4194304.0);
    const double sxx = ((double)s_acc[0][1] * 4294967296.0 + (double)s_acc[0][2]) * (1.0 / 17592186044416.0);
    const double m = sx / N;
    const double var = sxx / N - m * m;
    mean[l * 3 + c] = (float)m;
    inv_std[l * 3 + c] = (float)(1.0 / sqrt(var));             // var == 0: +inf, and every projection NaN (0 * inf) -- loud
  }
}

__global__ __launch_bounds__(kThreads) void swd_project_kernel(const uint8_t* __restrict__ img, long n, int S,
                                                              const int32_t* __restrict__ pos, int P, int level,
                                                              const float* __restrict__ mean, const float* __restrict__ inv_std,
                                                              const float* __restrict__ dirs, int nd, float* __restrict__ proj,
                                                              long ldp) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const long i = blockIdx.x;
  build_pyramid(img + i * 3 * S * S, S, s_mem);
  const int sl = S >> level;
  const float* lev = s_mem + level_offset(S, level);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63;
  float mu[3], is[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { mu[c] = mean[level * 3 + c]; is[c] = inv_std[level * 3 + c]; }
  const int ngroups = (nd + kDirsPerPass - 1) / kDirsPerPass;
  for (int p0 = 0; p0 < P; p0 += 64) {
    const int p = p0 + lane;
    const bool live = p < P;
    int y0, x0;
    patch_corner(pos, n, P, level, i, live ? p : P - 1, sl, &y0, &x0);
    float x[kDesc];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int dy = 0; dy < kPatch; ++dy)
#pragma unroll
        for (int dx = 0; dx < kPatch; ++dx)
          x[(c * kPatch + dy) * kPatch + dx] = (lev[((y0 + dy) * sl + x0 + dx) * 3 + c] - mu[c]) * is[c];
    for (int q = wave; q < ngroups; q += kThreads / 64) {
      const int j0 = kDirsPerPass * q;
      // a row past the last direction is computed from the last one and not stored
      const float* d[kDirsPerPass];
      float acc[kDirsPerPass];
#pragma unroll
      for (int k = 0; k < kDirsPerPass; ++k) {
        d[k] = dirs + (long)min(j0 + k, nd - 1) * kDesc;
        acc[k] = 0.0f;
      }
#pragma unroll
      for (int e = 0; e < kDesc; ++e)
#pragma unroll
        for (int k = 0; k < kDirsPerPass; ++k) acc[k] = fmaf(x[e], d[k][e], acc[k]);
      if (live) {
        float* o = proj + (long)j0 * ldp + i * P + p;
#pragma unroll
        for (int k = 0; k < kDirsPerPass; ++k)
          if (j0 + k < nd) o[k * ldp] = acc[k];
      }
    }
  }
}

// out[r] = (sum over k < m of |a[r][k] - b[r][k]|) / m in fp64: one workgroup of 1024 threads per row.  The order depends on m
// only: thread t adds the quads q = t, t + 1024, ... of four consecutive elements in that order, element by element; the thread
// that the quad after the last whole one would fall to adds the m % 4 elements left; then the wave butterfly and the 16 wave sums
// in index order.  Rows that are 16-byte aligned are read in 16-byte loads, any other row word by word -- the same order.
constexpr int kL1Threads = 1024;

__global__ __launch_bounds__(kL1Threads) void swd_row_l1_kernel(const float* __restrict__ a, long lda, const float* __restrict__ b,
                                                               long ldb, long m, double* __restrict__ out) {
  __shared__ double s_red[kL1Threads / 64];
  const long r = blockIdx.x;
  const float* pa = a + r * lda;
  const float* pb = b + r * ldb;
  const long quads = m / 4;
  const bool wide = (((uintptr_t)pa | (uintptr_t)pb) & 15) == 0;
  double acc = 0.0;
  if (wide) {
    for (long q = threadIdx.x; q < quads; q += kL1Threads) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(pa + 4 * q);
      const f32x4 vb = *reinterpret_cast<const f32x4*>(pb + 4 * q);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += fabs((double)va[k] - (double)vb[k]);
    }
  } else {
    for (long q = threadIdx.x; q < quads; q += kL1Threads) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += fabs((double)pa[4 * q + k] - (double)pb[4 * q + k]);
    }
  }
  if ((long)threadIdx.x == quads % kL1Threads)
    for (long k = 4 * quads; k < m; ++k) acc += fabs((double)pa[k] - (double)pb[k]);
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < kL1Threads / 64; ++w) t += s_red[w];
    out[r] = t / (double)m;
  }
}

size_t lds_bytes(int S) { return (size_t)level_offset(S, swd_levels(S)) * sizeof(float); }
size_t lds_bytes_f64(int S) { return (size_t)level_offset(S, swd_levels(S)) * sizeof(double); }   // 126 KiB at S = 64

int check_images(const char* what, const void* img, long n, int S) {
  if (swd_levels(S) == 0) {
    otgan_set_error("%s: S = %d (the pyramid is defined for 16, 32 and 64: coarsest level 16 x 16)", what, S);
    return OTGAN_ERR_UNSUPPORTED;
  }
  OTGAN_CHECK_ARG(img, "%s: null images", what);
  OTGAN_CHECK_ARG(n >= 0 && n <= 0x7fffffffL, "%s: n = %ld (0 ... 2^31 - 1)", what, n);
  OTGAN_CHECK_ARG(((uintptr_t)img & 3) == 0, "%s: the images must be 4-byte aligned", what);
  return OTGAN_OK;
}

int check_patches(const char* what, long n, int P, const void* pos) {
  OTGAN_CHECK_ARG(pos, "%s: null positions", what);
  OTGAN_CHECK_ARG(P >= 1 && (long)P <= kMaxPatchesTotal, "%s: P = %d (at least 1)", what, P);
  OTGAN_CHECK_ARG(n * (long)P <= kMaxPatchesTotal, "%s: n P = %ld patches per level (at most 2^27)", what, n * (long)P);
  OTGAN_CHECK_ARG(((uintptr_t)pos & 3) == 0, "%s: the positions must be 4-byte aligned", what);
  return OTGAN_OK;
}

}  // namespace

extern "C" int otgan_swd_levels(int S) { return swd_levels(S); }

extern "C" int otgan_swd_pyramid_u8(const uint8_t* img, long n, int S, int level, float* out, void* stream) {
  const int rc = check_images("swd_pyramid", img, n, S);
  if (rc != OTGAN_OK) return rc;
  OTGAN_CHECK_ARG(level >= 0 && level < swd_levels(S), "swd_pyramid: level = %d of %d", level, swd_levels(S));
  OTGAN_CHECK_ARG(out && ((uintptr_t)out & 15) == 0, "swd_pyramid: the output must be non-null and 16-byte aligned");
  if (n == 0) return OTGAN_OK;
  hipLaunchKernelGGL(swd_pyramid_kernel, dim3((unsigned)n), dim3(kThreads), lds_bytes(S), (hipStream_t)stream, img, S, level, out);
  OTGAN_CHECK_LAUNCH("swd_pyramid");
  return OTGAN_OK;
}

extern "C" size_t otgan_swd_workspace_bytes(long n, int S, int P) {
  (void)P;
  return n > 0 ? (size_t)n * swd_levels(S) * 6 * sizeof(double) : 0;
}

extern "C" int otgan_swd_channel_stats_u8(const uint8_t* img, long n, int S, const int32_t* pos, int P, float* mean,
                                          float* inv_std, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_images("swd_channel_stats", img, n, S);
  if (rc != OTGAN_OK) return rc;
  rc = check_patches("swd_channel_stats", n, P, pos);
  if (rc != OTGAN_OK) return rc;
  OTGAN_CHECK_ARG(n >= 1, "swd_channel_stats: n = %ld (statistics of no image)", n);
  OTGAN_CHECK_ARG(mean && inv_std, "swd_channel_stats: null mean or inv_std");
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < otgan_swd_workspace_bytes(n, S, P)) {
    otgan_set_error("swd_channel_stats: the workspace needs %zu bytes, 8-byte aligned (given %zu)",
                    otgan_swd_workspace_bytes(n, S, P), workspace_bytes);
    return OTGAN_ERR_WORKSPACE;
  }
  const int L = swd_levels(S);
  double* partial = reinterpret_cast<double*>(workspace);
  static bool once = (hipFuncSetAttribute(reinterpret_cast<const void*>(swd_stats_partial_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes_f64(64)), true);
  (void)once;
  hipLaunchKernelGGL(swd_stats_partial_kernel, dim3((unsigned)n), dim3(kThreads), lds_bytes_f64(S), (hipStream_t)stream, img, n, S,
                     pos, P, partial);
  OTGAN_CHECK_LAUNCH("swd_channel_stats");
  hipLaunchKernelGGL(swd_stats_finish_kernel, dim3(3 * L), dim3(kThreads), 0, (hipStream_t)stream, partial, n, L, P, mean, inv_std);
  OTGAN_CHECK_LAUNCH("swd_channel_stats (finish)");
  return OTGAN_OK;
}

extern "C" int otgan_swd_project_u8(const uint8_t* img, long n, int S, const int32_t* pos, int P, int level, const float* mean,
                                    const float* inv_std, const float* dirs, int nd, float* proj, long ldp, void* stream) {
  int rc = check_images("swd_project", img, n, S);
  if (rc != OTGAN_OK) return rc;
  rc = check_patches("swd_project", n, P, pos);
  if (rc != OTGAN_OK) return rc;
  OTGAN_CHECK_ARG(level >= 0 && level < swd_levels(S), "swd_project: level = %d of %d", level, swd_levels(S));
  OTGAN_CHECK_ARG(mean && inv_std && dirs && proj, "swd_project: null mean, inv_std, dirs or proj");
  OTGAN_CHECK_ARG(nd >= 0, "swd_project: nd = %d", nd);
  OTGAN_CHECK_ARG(ldp >= n * (long)P, "swd_project: ldp = %ld is below n P = %ld", ldp, n * (long)P);
  OTGAN_CHECK_ARG(((uintptr_t)dirs & 3) == 0 && ((uintptr_t)proj & 3) == 0, "swd_project: dirs and proj must be 4-byte aligned");
  if (n == 0 || nd == 0) return OTGAN_OK;
  hipLaunchKernelGGL(swd_project_kernel, dim3((unsigned)n), dim3(kThreads), lds_bytes(S), (hipStream_t)stream, img, n, S, pos, P,
                     level, mean, inv_std, dirs, nd, proj, ldp);
  OTGAN_CHECK_LAUNCH("swd_project");
  return OTGAN_OK;
}

extern "C" int otgan_swd_row_l1_f64(const float* a, long lda, const float* b, long ldb, int rows, long m, double* out,
                                    void* stream) {
  OTGAN_CHECK_ARG(a && b && out, "swd_row_l1: null a, b or out");
  OTGAN_CHECK_ARG(rows >= 0 && m >= 1, "swd_row_l1: rows = %d, m = %ld", rows, m);
  OTGAN_CHECK_ARG(lda >= m && ldb >= m, "swd_row_l1: lda = %ld, ldb = %ld below m = %ld", lda, ldb, m);
  OTGAN_CHECK_ARG(((uintptr_t)out & 7) == 0, "swd_row_l1: out must be 8-byte aligned");
  if (rows == 0) return OTGAN_OK;
  hipLaunchKernelGGL(swd_row_l1_kernel, dim3((unsigned)rows), dim3(kL1Threads), 0, (hipStream_t)stream, a, lda, b, ldb, m, out);
  OTGAN_CHECK_LAUNCH("swd_row_l1");
  return OTGAN_OK;
}
