// augment.hip -- differentiable augmentation of the critic's inputs (Zhao et al. 2020, "DiffAugment"): colour, translation and
// cutout of one image by parameters derived on the device from its row of uniforms, and the exact transpose
// (otgan_augment_fwd_f32 / otgan_augment_bwd_f32; the formulas are stated in include/otgan_layers.h).
//
// One workgroup of 256 threads per image, one launch per direction.  The image (the upstream gradient in the backward pass) is
// read from global memory ONCE, with aligned 16-byte loads, into LDS -- 12 KiB at 32 x 32, 48 KiB at 64 x 64 -- and everything
// after that reads LDS: the per-image sum, and the transform, whose source is shifted by 3 tx floats against the 16-byte grid of
// the output and is therefore read word by word, which LDS does at no cost in transactions.  (The alternative, a second read of
// the shifted source through L2, makes every wave's load straddle cache lines and reads HBM-resident batches twice when the
// launch does not fit L2.)  The output leaves in aligned 16-byte stores.
//
// Order of the per-image sum, the same for every image of a given S: thread t adds the quads t, t + 256, ... in that order
// (inside a quad: ((e0 + e1) + e2) + e3), a wave adds its 64 lanes by the xor butterfly of wave_sum, and every thread adds the
// four wave sums as (w0 + w1) + (w2 + w3).  No atomics and nothing crosses a workgroup: an image's output bits depend on its
// pixels, its row of u, S and policy alone.
#include "common.h"
#include "../../include/otgan.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxS = 64;

struct AugParams {
  float b, ks, kc;          // colour
  int tx, ty;               // translation: out(yy, xx) = colour(in(yy - ty, xx - tx))
  int wx0, wx1, wy0, wy1;   // cutout window [wx0, wx1) x [wy0, wy1) in output coordinates (empty when the bit is off)
};

__device__ __forceinline__ AugParams aug_params(const float* __restrict__ u, int S, int policy) {
  AugParams p;
  p.b = 0.0f; p.ks = 1.0f; p.kc = 1.0f;
  p.tx = p.ty = 0;
  p.wx0 = p.wx1 = p.wy0 = p.wy1 = 0;
  if (policy & OTGAN_AUG_COLOR) {
    p.b = u[0] - 0.5f;
    p.ks = 2.0f * u[1];
    p.kc = u[2] + 0.5f;
  }
  if (policy & OTGAN_AUG_TRANSLATION) {
    const int R = (S + 4) / 8;
    const float n = (float)(2 * R + 1);
    p.tx = min((int)(u[3] * n), 2 * R) - R;
    p.ty = min((int)(u[4] * n), 2 * R) - R;
  }
  if (policy & OTGAN_AUG_CUTOUT) {
    const int h = (S / 2) / 2;
    const float n = (float)(S + 1);
    const int ox = min((int)(u[5] * n), S), oy = min((int)(u[6] * n), S);
    p.wx0 = max(ox - h, 0); p.wx1 = min(ox + h, S);
    p.wy0 = max(oy - h, 0); p.wy1 = min(oy + h, S);
  }
  return p;
}

// the sum of one value per thread over the workgroup, in every thread; s_w: 4 floats of LDS, free again on return
__device__ __forceinline__ float block_sum(float v, float* s_w) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  const float t = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
  __syncthreads();
  return t;
}

// global -> LDS, aligned 16-byte accesses on both sides
__device__ __forceinline__ void stage_image(const float* __restrict__ src, float* s_img, int quads) {
  for (int q = threadIdx.x; q < quads; q += kThreads)
    *reinterpret_cast<f32x4*>(s_img + 4 * q) = *reinterpret_cast<const f32x4*>(src + 4 * q);
  __syncthreads();
}

// A quad of a line -- elements p ... p + 3 of its 3 S -- touches exactly the two pixels x0 = p / 3 and x0 + 1 (p + 3 <= 3 S - 1).
// Element j of the quad is channel (p + j) % 3 of pixel x0 + (p + j) / 3 - x0: slot k = p + j - 3 x0 of the six loaded values.

__global__ __launch_bounds__(kThreads) void augment_fwd_kernel(const float* __restrict__ x, int S, const float* __restrict__ u,
                                                               int policy, float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const long r = blockIdx.x;
  const int line = 3 * S, n = line * S, quads = n / 4;
  float* s_img = s_mem;
  float* s_w = s_mem + n;
  const AugParams a = aug_params(u + 8 * r, S, policy);
  const bool colour = (policy & OTGAN_AUG_COLOR) != 0;
  stage_image(x + r * n, s_img, quads);
  float mu = 0.0f;
  if (colour) {
    float acc = 0.0f;
    for (int q = threadIdx.x; q < quads; q += kThreads) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(s_img + 4 * q);
      acc += ((v[0] + v[1]) + v[2]) + v[3];
    }
    mu = block_sum(acc, s_w) / (float)n + a.b;
  }
  float* out = y + r * n;
  for (int q = threadIdx.x; q < quads; q += kThreads) {
    const int e = 4 * q;
    const int yy = e / line, p = e - yy * line;
    const int x0 = p / 3, k0 = p - 3 * x0;
    const int ys = yy - a.ty;
    const bool row_ok = ys >= 0 && ys < S, row_cut = yy >= a.wy0 && yy < a.wy1;
    float c[6];
#pragma unroll
    for (int px = 0; px < 2; ++px) {
      const int xx = x0 + px, xs = xx - a.tx;
      const bool cut = row_cut && xx >= a.wx0 && xx < a.wx1;
      float v0 = 0.0f, v1 = 0.0f, v2 = 0.0f;
      if (row_ok && !cut && xs >= 0 && xs < S) {
        const float* s = s_img + ys * line + 3 * xs;
        v0 = s[0]; v1 = s[1]; v2 = s[2];
        if (colour) {
          v0 += a.b; v1 += a.b; v2 += a.b;
          const float m = (v0 + v1 + v2) / 3.0f;
          v0 = (v0 - m) * a.ks + m; v1 = (v1 - m) * a.ks + m; v2 = (v2 - m) * a.ks + m;
          v0 = (v0 - mu) * a.kc + mu; v1 = (v1 - mu) * a.kc + mu; v2 = (v2 - mu) * a.kc + mu;
        }
      }
      c[3 * px] = v0; c[3 * px + 1] = v1; c[3 * px + 2] = v2;
    }
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = k0 == 0 ? c[j] : (k0 == 1 ? c[j + 1] : c[j + 2]);
    *reinterpret_cast<f32x4*>(out + e) = o;
  }
}

// e[q] of the header: the upstream gradient that reaches input position (yi, xi), channels 0 .. 2, from the staged dy
__device__ __forceinline__ void bwd_gather(const float* s_dy, const AugParams& a, int S, int yi, int xi, float* e3) {
  const int yo = yi + a.ty, xo = xi + a.tx;
  const bool in = yo >= 0 && yo < S && xo >= 0 && xo < S;
  const bool cut = yo >= a.wy0 && yo < a.wy1 && xo >= a.wx0 && xo < a.wx1;
  e3[0] = e3[1] = e3[2] = 0.0f;
  if (in && !cut) {
    const float* s = s_dy + (yo * S + xo) * 3;
    e3[0] = s[0]; e3[1] = s[1]; e3[2] = s[2];
  }
}

__global__ __launch_bounds__(kThreads) void augment_bwd_kernel(const float* __restrict__ dy, int S, const float* __restrict__ u,
                                                               int policy, float* __restrict__ dx) {
  extern __shared__ __attribute__((aligned(16))) float s_mem[];
  const long r = blockIdx.x;
  const int line = 3 * S, n = line * S, quads = n / 4;
  float* s_dy = s_mem;
  float* s_w = s_mem + n;
  const AugParams a = aug_params(u + 8 * r, S, policy);
  const bool colour = (policy & OTGAN_AUG_COLOR) != 0;
  stage_image(dy + r * n, s_dy, quads);
  float mean = 0.0f;
  if (colour) {
    // the sum of e over the image: every input element once, in the order stated at the top of the file
    float acc = 0.0f;
    for (int q = threadIdx.x; q < quads; q += kThreads) {
      const int e = 4 * q;
      const int yi = e / line, p = e - yi * line;
      const int x0 = p / 3, k0 = p - 3 * x0;
      float c[6];
      bwd_gather(s_dy, a, S, yi, x0, c);
      bwd_gather(s_dy, a, S, yi, x0 + 1, c + 3);
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = k0 == 0 ? c[j] : (k0 == 1 ? c[j + 1] : c[j + 2]);
      acc += ((v[0] + v[1]) + v[2]) + v[3];
    }
    mean = block_sum(acc, s_w) / (float)n;
  }
  float* out = dx + r * n;
  for (int q = threadIdx.x; q < quads; q += kThreads) {
    const int e = 4 * q;
    const int yi = e / line, p = e - yi * line;
    const int x0 = p / 3, k0 = p - 3 * x0;
    float c[6];
    bwd_gather(s_dy, a, S, yi, x0, c);
    bwd_gather(s_dy, a, S, yi, x0 + 1, c + 3);
    if (colour) {
#pragma unroll
      for (int px = 0; px < 2; ++px) {
        float* e3 = c + 3 * px;
        const float f0 = a.kc * e3[0] + (1.0f - a.kc) * mean;       // e2 = kc e + (1 - kc) mean_image(e)
        const float f1 = a.kc * e3[1] + (1.0f - a.kc) * mean;
        const float f2 = a.kc * e3[2] + (1.0f - a.kc) * mean;
        const float m = (f0 + f1 + f2) / 3.0f;                      // dx = ks e2 + (1 - ks) mean_channels(e2)
        e3[0] = a.ks * f0 + (1.0f - a.ks) * m;
        e3[1] = a.ks * f1 + (1.0f - a.ks) * m;
        e3[2] = a.ks * f2 + (1.0f - a.ks) * m;
      }
    }
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = k0 == 0 ? c[j] : (k0 == 1 ? c[j + 1] : c[j + 2]);
    *reinterpret_cast<f32x4*>(out + e) = o;
  }
}

int check_args(const char* what, const void* in, long rows, int S, const float* u, int policy, const void* out) {
  OTGAN_CHECK_ARG(in && u && out, "%s: null input, u or output", what);
  OTGAN_CHECK_ARG(rows >= 0 && rows <= 0x7fffffffL, "%s: rows = %ld (0 ... 2^31 - 1)", what, rows);
  OTGAN_CHECK_ARG(S >= 4 && S <= kMaxS && S % 4 == 0, "%s: S = %d must be a multiple of 4 in 4 ... %d", what, S, kMaxS);
  OTGAN_CHECK_ARG(policy >= 0 && policy <= (OTGAN_AUG_COLOR | OTGAN_AUG_TRANSLATION | OTGAN_AUG_CUTOUT),
                  "%s: policy = %d is no mask of OTGAN_AUG_COLOR | OTGAN_AUG_TRANSLATION | OTGAN_AUG_CUTOUT", what, policy);
  OTGAN_CHECK_ARG(((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)u & 3) == 0,
                  "%s: input and output must be 16-byte aligned, u 4-byte aligned", what);
  OTGAN_CHECK_ARG(in != out, "%s: the output must not be the input", what);
  return OTGAN_OK;
}

size_t lds_bytes(int S) { return (size_t)(3 * S * S + 4) * sizeof(float); }

}  // namespace

extern "C" int otgan_augment_fwd_f32(const float* x, long rows, int S, const float* u, int policy, float* y, void* stream) {
  const int rc = check_args("augment_fwd", x, rows, S, u, policy, y);
  if (rc != OTGAN_OK || rows == 0) return rc;
  hipLaunchKernelGGL(augment_fwd_kernel, dim3((unsigned)rows), dim3(kThreads), lds_bytes(S), (hipStream_t)stream, x, S, u, policy, y);
  OTGAN_CHECK_LAUNCH("augment_fwd");
  return OTGAN_OK;
}

extern "C" int otgan_augment_bwd_f32(const float* dy, long rows, int S, const float* u, int policy, float* dx, void* stream) {
  const int rc = check_args("augment_bwd", dy, rows, S, u, policy, dx);
  if (rc != OTGAN_OK || rows == 0) return rc;
  hipLaunchKernelGGL(augment_bwd_kernel, dim3((unsigned)rows), dim3(kThreads), lds_bytes(S), (hipStream_t)stream, dy, S, u, policy, dx);
  OTGAN_CHECK_LAUNCH("augment_bwd");
  return OTGAN_OK;
}
