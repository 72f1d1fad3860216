// data.hip -- the training batch straight from a device-resident uint8 dataset (otgan_batch_from_u8_f32).
// One launch gathers the step's images by the epoch's permutation, flips them horizontally per image, converts
// uint8 -> [-1, 1] and (optionally) box-downsamples by 2 or 4 (reference train.py:158,163-170,209-211).
#include "common.h"
#include "../../include/otgan.h"

struct BatchU8Args {
  const uint8_t* store;
  const int32_t* perm;
  const uint8_t* flip;
  const float* lut;
  float* out;
  long ldo;
  long off[OTGAN_BATCH_U8_MAX_SHARDS];
  int B, S, SW;
  long image_bytes;        // SH * SW * 3
};

// Thread = one float4 of one output image.  A line of the output is 3 S floats, a multiple of 4 (S % 4 == 0): a float4 never
// crosses a line, and image rows are written contiguously.  grid.x = output row, grid.y = workgroups per image.
//   F = 1: out = lut[byte] (the host's own table: bit-identical to `x / 127.5 - 1.` of load_cifar by construction); without a
//          flip the four source bytes are the four bytes at the same offset of the source image (one aligned 32-bit load),
//          with a flip the PIXEL order reverses inside the line and the channel order stays: byte by byte.
//   F = 2, 4: the exact integer sum of the F x F box, then (float)sum / (127.5 F^2) - 1 (correctly rounded division: the
//          library is built without fast-math; a quotient and a subtraction do not contract).
template <int F>
__global__ __launch_bounds__(256) void batch_from_u8_kernel(BatchU8Args a) {
  __shared__ float s_lut[256];
  if (F == 1) {
    s_lut[threadIdx.x] = a.lut[threadIdx.x];
    __syncthreads();
  }
  const int S = a.S;
  const int quads = 3 * S * S / 4;
  const int q = blockIdx.y * 256 + threadIdx.x;
  if (q >= quads) return;
  const long r = blockIdx.x;
  const int s = (int)(r / a.B), k = (int)(r % a.B);
  const long at = a.off[s] + k;
  const long idx = a.perm ? (long)a.perm[at] : at;
  const uint8_t* __restrict__ img = a.store + idx * a.image_bytes;          // 64-bit: idx * 12288 passes 2^32 at image 349 526
  const bool flip = a.flip && a.flip[r];
  const int e = 4 * q;                   // first element of the quad inside the image
  const int y = e / (3 * S);
  const int p = e - y * 3 * S;           // element inside the line: pixel p / 3, channel p % 3
  f32x4 v;
  if (F == 1) {
    if (!flip) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(img + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = s_lut[(w >> (8 * j)) & 0xffu];
    } else {
      const uint8_t* line = img + (long)y * 3 * S;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int x = (p + j) / 3, c = (p + j) - 3 * x;
        v[j] = s_lut[line[3 * (S - 1 - x) + c]];
      }
    }
  } else {
    const int lds = 3 * a.SW;            // bytes per source line
    const float den = 127.5f * F * F;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = (p + j) / 3, c = (p + j) - 3 * x;
      const int xs = flip ? S - 1 - x : x;
      const uint8_t* box = img + (long)(F * y) * lds + 3 * (F * xs) + c;
      unsigned sum = 0;
#pragma unroll
      for (int dy = 0; dy < F; ++dy)
#pragma unroll
        for (int dx = 0; dx < F; ++dx) sum += box[dy * lds + 3 * dx];
      v[j] = (float)sum / den - 1.0f;
    }
  }
  *reinterpret_cast<f32x4*>(a.out + r * a.ldo + e) = v;
}

extern "C" int otgan_batch_from_u8_f32(const uint8_t* store, long n_images, int SH, int SW, const int32_t* perm, long perm_len,
                                       const long* shard_offsets, int n_shards, int B, const uint8_t* flip, const float* lut,
                                       int S, float* out, long ldo, void* stream) {
  OTGAN_CHECK_ARG(store && lut && out && shard_offsets, "batch_from_u8: null store, lut, out or shard_offsets");
  OTGAN_CHECK_ARG(n_images > 0 && SH > 0 && SW > 0 && B > 0, "batch_from_u8: n_images %ld, SH %d, SW %d, B %d must be positive",
                  n_images, SH, SW, B);
  OTGAN_CHECK_ARG(SH <= 4096 && SW <= 4096, "batch_from_u8: images of %d x %d (at most 4096 x 4096)", SH, SW);
  OTGAN_CHECK_ARG(n_shards >= 1 && n_shards <= OTGAN_BATCH_U8_MAX_SHARDS, "batch_from_u8: %d shards (1 ... %d)", n_shards,
                  OTGAN_BATCH_U8_MAX_SHARDS);
  OTGAN_CHECK_ARG(S > 0 && S % 4 == 0, "batch_from_u8: S = %d must be a positive multiple of 4", S);
  const int f = SH / S;
  OTGAN_CHECK_ARG(SH == f * S && SW == f * S && (f == 1 || f == 2 || f == 4),
                  "batch_from_u8: %d x %d images feed S = %d only by an integer factor 1, 2 or 4 in both directions", SH, SW, S);
  OTGAN_CHECK_ARG(perm == nullptr || perm_len > 0, "batch_from_u8: permutation of %ld entries", perm_len);
  const long limit = perm ? perm_len : n_images;
  for (int s = 0; s < n_shards; ++s)
    OTGAN_CHECK_ARG(shard_offsets[s] >= 0 && shard_offsets[s] <= limit - B,
                    "batch_from_u8: shard %d reads rows %ld ... %ld of %ld (%s)", s, shard_offsets[s], shard_offsets[s] + B, limit,
                    perm ? "the permutation" : "the store");
  const long row = 3L * S * S;
  OTGAN_CHECK_ARG(ldo >= row && ldo % 4 == 0, "batch_from_u8: ldo = %ld (needs >= %ld and a multiple of 4)", ldo, row);
  OTGAN_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)store & 3) == 0,
                  "batch_from_u8: out must be 16-byte aligned and store 4-byte aligned");
  const long rows = (long)n_shards * B;
  OTGAN_CHECK_ARG(rows <= 0x7fffffffL, "batch_from_u8: %ld rows in one launch", rows);
  BatchU8Args a;
  a.store = store; a.perm = perm; a.flip = flip; a.lut = lut; a.out = out; a.ldo = ldo;
  for (int s = 0; s < OTGAN_BATCH_U8_MAX_SHARDS; ++s) a.off[s] = s < n_shards ? shard_offsets[s] : 0;
  a.B = B; a.S = S; a.SW = SW; a.image_bytes = 3L * SH * SW;
  const dim3 grid((unsigned)rows, (unsigned)ceil_div_l(row / 4, 256)), block(256);   // (y <= 49152 at 4096 x 4096)
  if (f == 1) hipLaunchKernelGGL(batch_from_u8_kernel<1>, grid, block, 0, (hipStream_t)stream, a);
  else if (f == 2) hipLaunchKernelGGL(batch_from_u8_kernel<2>, grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(batch_from_u8_kernel<4>, grid, block, 0, (hipStream_t)stream, a);
  OTGAN_CHECK_LAUNCH("batch_from_u8");
  return OTGAN_OK;
}
