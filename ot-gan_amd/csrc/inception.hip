// inception.hip -- inference kernels of the 2015 Inception graph (the evaluation network of the reference's
// utils/inception.py), lowered by utils/inception_net.py:
//   * otgan_incep_conv2d_f32: implicit-GEMM convolution on the gemm_tile.h engine (fp32 MFMA, exact fp32 products)
//     for arbitrary H, W, KH x KW taps, strides and TF SAME / VALID padding; folded batch-norm bias and ReLU in the
//     epilogue; output at a channel offset of a wider buffer (the concats of the graph are never materialised).
//     A = the [N*OH*OW, KH*KW*C] patch matrix gathered on the fly, B = the HWIO weights as [KH*KW*C, Cout].
//   * otgan_incep_pool_f32: 2-D max / average pooling with TF padding (SAME average: in-bounds taps only).
//   * otgan_incep_resize_f32: legacy bilinear resize (src = dst * in / out, upper neighbour clamped) and a scalar
//     affine -- the graph's Sub / Mul pair, or 127.5 (x + 1) of generator output folded in front of it.
//   * otgan_incep_head_f32: global average pool -> pool_3, logits = pool_3 . W (no bias: the reference's
//     utils/inception.py:91-93), row softmax.
#include <type_traits>

#include "common.h"
#include "gemm_tile.h"
#include "../../include/otgan.h"

namespace {

using IncCfg128 = GemmCfg<2, 2, 2, 2, 32>;   // 128 x 128 x 32, four waves of 64 x 64
using IncCfg64 = GemmCfg<4, 1, 1, 2, 32>;    // 128 x 64 x 32 (Cout % 128 in 1..64: 192, 320, 448, 32, 64 ...)

template <auto Kern>
inline void inc_ensure_lds(size_t bytes) {
  static const bool done = [bytes] {
    hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return true;
  }();
  (void)done;
}

struct IncConvArgs {
  const float* x;
  const float* w;      // [K][Cout]
  const float* bias;   // [Cout] or null
  float* y;
  int H, W, C, ldx;
  int KW, sh, sw, pt, pl;
  int OH, OW;
  int M, K, Cout, ldy, y_coff, relu;
};

// TF output size and leading pad of one spatial dimension
inline void tf_pad(int in, int k, int s, int same, int* out, int* before) {
  if (same) {
    *out = (in + s - 1) / s;
    int total = (*out - 1) * s + k - in;
    if (total < 0) total = 0;
    *before = total / 2;
  } else {
    *out = in >= k ? (in - k) / s + 1 : 0;
    *before = 0;
  }
}

// A operand of the implicit GEMM: element (r, k) = x[n, oh*sh - pt + kh, ow*sw - pl + kw, ci] (zero outside the
// image), k = (kh * KW + kw) * C + ci.  k-contiguous staging as MatLoaderK: each thread fetches 4 consecutive k of
// PASSES rows.  VEC (C % 4 == 0, ldx % 4 == 0): the 4 k are 4 channels of one tap -> one 16-byte load; else scalar.
template <class Cfg, int BR, bool VEC>
struct IncGatherA {
  static constexpr int BK = Cfg::BK;
  static constexpr int LD = BR + KPad<BK>::value;
  static constexpr int FLOATS = BK * LD;
  static constexpr int CPR = BK / 4;
  static constexpr int RPP = Cfg::THREADS / CPR;
  static constexpr int PASSES = (BR + RPP - 1) / RPP;
  IncConvArgs a;
  long pix[PASSES];   // pixel index of (n, 0, 0), or -1 for rows past M
  int ih0[PASSES], iw0[PASSES];
  float4 reg[PASSES];

  __device__ __forceinline__ void init(const IncConvArgs& args, int m0) {
    a = args;
    const int r0 = threadIdx.x / CPR;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int r = r0 + p * RPP, m = m0 + r;
      pix[p] = -1;
      ih0[p] = iw0[p] = 0;
      if (r < BR && m < args.M) {
        const int ow = m % args.OW, t = m / args.OW;
        const int oh = t % args.OH, n = t / args.OH;
        pix[p] = (long)n * args.H * args.W;
        ih0[p] = oh * args.sh - args.pt;
        iw0[p] = ow * args.sw - args.pl;
      }
    }
  }
  __device__ __forceinline__ float fetch(int p, int k) const {
    if (k >= a.K || pix[p] < 0) return 0.f;
    const int ci = k % a.C, t = k / a.C;
    const int ih = ih0[p] + t / a.KW, iw = iw0[p] + t % a.KW;
    if ((unsigned)ih >= (unsigned)a.H || (unsigned)iw >= (unsigned)a.W) return 0.f;
    return a.x[(pix[p] + (long)ih * a.W + iw) * a.ldx + ci];
  }
  __device__ __forceinline__ void load(int kt) {
    const int c = threadIdx.x % CPR;
    const int k = kt * BK + 4 * c;
    if (VEC) {
      const bool kin = k < a.K;
      const int ci = kin ? k % a.C : 0, t = kin ? k / a.C : 0;
      const int kh = t / a.KW, kw = t % a.KW;
#pragma unroll
      for (int p = 0; p < PASSES; ++p) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const int ih = ih0[p] + kh, iw = iw0[p] + kw;
        if (kin && pix[p] >= 0 && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
          v = *reinterpret_cast<const float4*>(a.x + (pix[p] + (long)ih * a.W + iw) * a.ldx + ci);
        reg[p] = v;
      }
    } else {
#pragma unroll
      for (int p = 0; p < PASSES; ++p)
        reg[p] = make_float4(fetch(p, k), fetch(p, k + 1), fetch(p, k + 2), fetch(p, k + 3));
    }
  }
  __device__ __forceinline__ void store(float* t) const {
    const int c = threadIdx.x % CPR, r0 = threadIdx.x / CPR;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int r = r0 + p * RPP;
      if (r < BR) {
        float* d = t + (4 * c) * LD + r;
        d[0] = reg[p].x;
        d[LD] = reg[p].y;
        d[2 * LD] = reg[p].z;
        d[3 * LD] = reg[p].w;
      }
    }
  }
};

// AMODE 0: 1x1 / stride 1 / no pad -- A is x itself ([M][C], row stride ldx; 16-byte loads);
//       1: gather, 16-byte loads (C % 4 == 0);  2: gather, scalar loads (the 3-channel first layer)
template <class Cfg, int AMODE>
__global__ __launch_bounds__(Cfg::THREADS) void incep_conv_kernel(IncConvArgs a) {
  using LA = typename std::conditional<AMODE == 0, MatLoaderK<Cfg, Cfg::BM, true>,
                                       IncGatherA<Cfg, Cfg::BM, AMODE == 1>>::type;
  using LB = MatLoaderR<Cfg, Cfg::BN, true>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int m0 = blockIdx.x * Cfg::BM, n0 = blockIdx.y * Cfg::BN;
  LA la;
  if constexpr (AMODE == 0) la.init(a.x + (long)m0 * a.ldx, a.ldx, a.M - m0, a.K);
  else la.init(a, m0);
  LB lb;
  lb.init(a.w + n0, a.Cout, a.Cout - n0, a.K);
  typename Cfg::acc_t acc[Cfg::MT][Cfg::NT];
  zero_acc<Cfg>(acc);
  gemm_mainloop<Cfg>(la, lb, (a.K + Cfg::BK - 1) / Cfg::BK, smem, acc);
  foreach_acc<Cfg>(acc, [&](int row, int col, int, int, int, float v) {
    const int m = m0 + row, n = n0 + col;
    if (m < a.M && n < a.Cout) {
      if (a.bias) v += a.bias[n];
      if (a.relu) v = fmaxf(v, 0.f);
      a.y[(long)m * a.ldy + a.y_coff + n] = v;
    }
  });
}

template <class Cfg, int AMODE>
void launch_conv(const IncConvArgs& a, hipStream_t s) {
  constexpr size_t lds = 2 * sizeof(float) *
      ((AMODE == 0 ? MatLoaderK<Cfg, Cfg::BM, true>::FLOATS : IncGatherA<Cfg, Cfg::BM, true>::FLOATS) +
       MatLoaderR<Cfg, Cfg::BN, true>::FLOATS);
  inc_ensure_lds<incep_conv_kernel<Cfg, AMODE>>(lds);
  dim3 grid((a.M + Cfg::BM - 1) / Cfg::BM, (a.Cout + Cfg::BN - 1) / Cfg::BN);
  hipLaunchKernelGGL((incep_conv_kernel<Cfg, AMODE>), grid, dim3(Cfg::THREADS), lds, s, a);
}

template <class Cfg>
void launch_conv_mode(const IncConvArgs& a, int mode, hipStream_t s) {
  if (mode == 0) launch_conv<Cfg, 0>(a, s);
  else if (mode == 1) launch_conv<Cfg, 1>(a, s);
  else launch_conv<Cfg, 2>(a, s);
}

// one thread per output element (pixel, channel): channels fastest, coalesced
__global__ __launch_bounds__(256) void incep_pool_kernel(const float* __restrict__ x, float* __restrict__ y, long total,
                                                         int H, int W, int C, int ldx, int OH, int OW, int KH, int KW,
                                                         int sh, int sw, int pt, int pl, int is_max, int ldy, int y_coff) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const long opix = i / C;
  const int ow = (int)(opix % OW);
  const long t = opix / OW;
  const int oh = (int)(t % OH);
  const long n = t / OH;
  const int h0 = oh * sh - pt, w0 = ow * sw - pl;
  float acc = is_max ? -INFINITY : 0.f;
  int cnt = 0;
  for (int kh = 0; kh < KH; ++kh) {
    const int ih = h0 + kh;
    if ((unsigned)ih >= (unsigned)H) continue;
    for (int kw = 0; kw < KW; ++kw) {
      const int iw = w0 + kw;
      if ((unsigned)iw >= (unsigned)W) continue;
      const float v = x[((n * H + ih) * W + iw) * ldx + c];
      acc = is_max ? fmaxf(acc, v) : acc + v;
      ++cnt;
    }
  }
  if (!is_max) acc = cnt ? acc / (float)cnt : 0.f;
  y[opix * ldy + y_coff + c] = acc;
}

// legacy bilinear: in = dst * scale, lo = floor(in), hi = min(lo + 1, size - 1); y = a * bilinear(x) + b
__global__ __launch_bounds__(256) void incep_resize_kernel(const float* __restrict__ x, float* __restrict__ y, long total,
                                                           int H, int W, int C, int OH, int OW, float sy, float sx,
                                                           float a, float b) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const long opix = i / C;
  const int ox = (int)(opix % OW);
  const long t = opix / OW;
  const int oy = (int)(t % OH);
  const long n = t / OH;
  const float fy = oy * sy, fx = ox * sx;
  const int y0 = min((int)floorf(fy), H - 1), x0 = min((int)floorf(fx), W - 1);
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  const float ly = fy - y0, lx = fx - x0;
  const float* p = x + n * H * W * C + c;
  const float tl = p[((long)y0 * W + x0) * C], tr = p[((long)y0 * W + x1) * C];
  const float bl = p[((long)y1 * W + x0) * C], br = p[((long)y1 * W + x1) * C];
  const float top = tl + (tr - tl) * lx, bot = bl + (br - bl) * lx;
  y[i] = a * (top + (bot - top) * ly) + b;
}

// pool3[n][c] = mean over the HW pixels of image n
__global__ __launch_bounds__(256) void incep_gap_kernel(const float* __restrict__ x, float* __restrict__ pool3, int N, int HW,
                                                        int C, int ldx) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)N * C) return;
  const int c = (int)(i % C);
  const long n = i / C;
  const float* p = x + n * HW * ldx + c;
  float s = 0.f;
  for (int k = 0; k < HW; ++k) s += p[(long)k * ldx];
  pool3[i] = s / (float)HW;
}

// one workgroup per row: probs = softmax(logits)
__global__ __launch_bounds__(256) void incep_softmax_kernel(const float* __restrict__ logits, float* __restrict__ probs,
                                                            int classes) {
  __shared__ float s_red[4];
  const float* l = logits + (long)blockIdx.x * classes;
  float* p = probs + (long)blockIdx.x * classes;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < classes; j += 256) m = fmaxf(m, l[j]);
  m = wave_max(m);
  if (lane == 0) s_red[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  __syncthreads();
  float s = 0.f;
  for (int j = threadIdx.x; j < classes; j += 256) s += expf(l[j] - m);
  s = wave_sum(s);
  if (lane == 0) s_red[wave] = s;
  __syncthreads();
  const float inv = 1.f / (s_red[0] + s_red[1] + s_red[2] + s_red[3]);
  for (int j = threadIdx.x; j < classes; j += 256) p[j] = expf(l[j] - m) * inv;
}

inline unsigned grid1(long total) { return (unsigned)((total + 255) / 256); }

int conv_launch(const IncConvArgs& a, hipStream_t s) {
  const bool direct = a.K == a.C && a.OH == a.H && a.OW == a.W && a.pt == 0 && a.pl == 0 && a.sh == 1 && a.sw == 1;
  const bool vec = a.C % 4 == 0 && a.ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0;
  const int mode = direct && a.ldx % 4 == 0 && (reinterpret_cast<uintptr_t>(a.x) & 15) == 0 ? 0 : (vec ? 1 : 2);
  OTGAN_CHECK_ARG(a.Cout % 4 == 0 && (reinterpret_cast<uintptr_t>(a.w) & 15) == 0,
                  "incep conv: Cout %d must be a multiple of 4 and w 16-byte aligned", a.Cout);
  if (a.M == 0) return OTGAN_OK;
  const int r = a.Cout % 128;
  if (r > 0 && r <= 64) launch_conv_mode<IncCfg64>(a, mode, s);
  else launch_conv_mode<IncCfg128>(a, mode, s);
  OTGAN_CHECK_LAUNCH("otgan_incep_conv2d_f32");
  return OTGAN_OK;
}

}  // namespace

extern "C" {

int otgan_incep_out_size(int in, int k, int stride, int same) {
  if (in <= 0 || k <= 0 || stride <= 0) return -1;
  int out, before;
  tf_pad(in, k, stride, same, &out, &before);
  return out;
}

int otgan_incep_conv2d_f32(const otgan_incep_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                           void* stream) {
  OTGAN_CHECK_ARG(d && x && w && y, "otgan_incep_conv2d_f32: null argument");
  OTGAN_CHECK_ARG(d->N >= 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->ldx >= d->C && d->KH > 0 && d->KW > 0 &&
                      d->stride_h > 0 && d->stride_w > 0 && d->Cout > 0 && d->y_coff >= 0 && d->ldy >= d->y_coff + d->Cout,
                  "otgan_incep_conv2d_f32: bad geometry");
  IncConvArgs a;
  a.x = x; a.w = w; a.bias = bias; a.y = y;
  a.H = d->H; a.W = d->W; a.C = d->C; a.ldx = d->ldx;
  a.KW = d->KW; a.sh = d->stride_h; a.sw = d->stride_w;
  tf_pad(d->H, d->KH, d->stride_h, d->same, &a.OH, &a.pt);
  tf_pad(d->W, d->KW, d->stride_w, d->same, &a.OW, &a.pl);
  OTGAN_CHECK_ARG(a.OH > 0 && a.OW > 0, "otgan_incep_conv2d_f32: %dx%d input smaller than the %dx%d VALID window",
                  d->H, d->W, d->KH, d->KW);
  const long M = (long)d->N * a.OH * a.OW, K = (long)d->KH * d->KW * d->C;
  OTGAN_CHECK_ARG(M < (1L << 31) && K < (1L << 30), "otgan_incep_conv2d_f32: batch too large for one call");
  a.M = (int)M; a.K = (int)K;
  a.Cout = d->Cout; a.ldy = d->ldy; a.y_coff = d->y_coff; a.relu = d->relu;
  return conv_launch(a, (hipStream_t)stream);
}

int otgan_incep_pool_f32(const otgan_incep_pool_desc* d, const float* x, float* y, void* stream) {
  OTGAN_CHECK_ARG(d && x && y, "otgan_incep_pool_f32: null argument");
  OTGAN_CHECK_ARG(d->N >= 0 && d->H > 0 && d->W > 0 && d->C > 0 && d->ldx >= d->C && d->KH > 0 && d->KW > 0 &&
                      d->stride_h > 0 && d->stride_w > 0 && d->y_coff >= 0 && d->ldy >= d->y_coff + d->C &&
                      (d->op == OTGAN_INCEP_POOL_MAX || d->op == OTGAN_INCEP_POOL_AVG),
                  "otgan_incep_pool_f32: bad geometry");
  int OH, OW, pt, pl;
  tf_pad(d->H, d->KH, d->stride_h, d->same, &OH, &pt);
  tf_pad(d->W, d->KW, d->stride_w, d->same, &OW, &pl);
  OTGAN_CHECK_ARG(OH > 0 && OW > 0, "otgan_incep_pool_f32: input smaller than the VALID window");
  const long total = (long)d->N * OH * OW * d->C;
  if (total == 0) return OTGAN_OK;
  hipLaunchKernelGGL(incep_pool_kernel, dim3(grid1(total)), dim3(256), 0, (hipStream_t)stream, x, y, total, d->H, d->W,
                     d->C, d->ldx, OH, OW, d->KH, d->KW, d->stride_h, d->stride_w, pt, pl,
                     d->op == OTGAN_INCEP_POOL_MAX ? 1 : 0, d->ldy, d->y_coff);
  OTGAN_CHECK_LAUNCH("otgan_incep_pool_f32");
  return OTGAN_OK;
}

int otgan_incep_resize_f32(int N, int H, int W, int C, int OH, int OW, int align_corners, float scale, float shift,
                           const float* x, float* y, void* stream) {
  OTGAN_CHECK_ARG(x && y && N >= 0 && H > 0 && W > 0 && C > 0 && OH > 0 && OW > 0, "otgan_incep_resize_f32: bad geometry");
  const float sy = (align_corners && OH > 1) ? (float)(H - 1) / (float)(OH - 1) : (float)H / (float)OH;
  const float sx = (align_corners && OW > 1) ? (float)(W - 1) / (float)(OW - 1) : (float)W / (float)OW;
  const long total = (long)N * OH * OW * C;
  if (total == 0) return OTGAN_OK;
  hipLaunchKernelGGL(incep_resize_kernel, dim3(grid1(total)), dim3(256), 0, (hipStream_t)stream, x, y, total, H, W, C, OH,
                     OW, sy, sx, scale, shift);
  OTGAN_CHECK_LAUNCH("otgan_incep_resize_f32");
  return OTGAN_OK;
}

int otgan_incep_head_f32(int N, int HW, int C, int ldx, int classes, const float* x, const float* w, float* pool3,
                         float* logits, float* probs, void* stream) {
  OTGAN_CHECK_ARG(x && w && pool3 && logits && probs && N >= 0 && HW > 0 && C > 0 && ldx >= C && classes > 0,
                  "otgan_incep_head_f32: bad arguments");
  OTGAN_CHECK_ARG(C % 4 == 0 && classes % 4 == 0 && (reinterpret_cast<uintptr_t>(pool3) & 15) == 0,
                  "otgan_incep_head_f32: C %d and classes %d must be multiples of 4, pool3 16-byte aligned", C, classes);
  if (N == 0) return OTGAN_OK;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(incep_gap_kernel, dim3(grid1((long)N * C)), dim3(256), 0, s, x, pool3, N, HW, C, ldx);
  OTGAN_CHECK_LAUNCH("otgan_incep_head_f32 (pool)");
  IncConvArgs a;
  a.x = pool3; a.w = w; a.bias = nullptr; a.y = logits;
  a.H = a.W = 1; a.C = C; a.ldx = C;
  a.KW = 1; a.sh = a.sw = 1; a.pt = a.pl = 0; a.OH = a.OW = 1;
  a.M = N; a.K = C; a.Cout = classes; a.ldy = classes; a.y_coff = 0; a.relu = 0;
  const int rc = conv_launch(a, s);
  if (rc != OTGAN_OK) return rc;
  hipLaunchKernelGGL(incep_softmax_kernel, dim3(N), dim3(256), 0, s, logits, probs, classes);
  OTGAN_CHECK_LAUNCH("otgan_incep_head_f32 (softmax)");
  return OTGAN_OK;
}

}  // extern "C"
