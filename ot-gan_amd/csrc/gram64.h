// gram64.h -- the fp64 Gram-block stage of kid.hip and knn.hip: a workgroup of four waves forms the 64 x 64 block
// A B^T of two sets of 64 fp32 rows (each wave 32 x 32 as 2 x 2 tiles of v_mfma_f64_16x16x4_f64), the channels in slabs
// of 32.  The fp32 inputs are converted to fp64 BEFORE the multiply, so every product is exact.
// Operand layout of the f64 MFMA (also what moments.hip builds on): lane l holds A[m = l & 15][k = l >> 4] and
// B[k = l >> 4][n = l & 15]; result register r of lane l is D[m = (l >> 4) + 4 r][n = l & 15] -- NOT the row map of
// the f32 forms.
// Operands: unlike moments.hip (lanes of a tile = adjacent columns of x, coalesced) the lanes of a tile are different ROWS
// here and K runs along the contiguous axis, so the rows go through LDS: each thread fetches two 16-byte pieces of the
// A rows and two of the B rows per slab (8 threads = the 128 contiguous bytes of one row), one slab ahead in registers,
// into one of two LDS buffers (one barrier per slab).  A dot product may visit k in any order as long as A and B agree,
// so the lane of k-group g = lane >> 4 takes the 8 CONSECUTIVE floats 8 g .. 8 g + 7 of its row of the slab (two
// ds_read_b128) and step u of the slab multiplies k = 8 g + u: no scalar LDS reads.  Rows are 36 floats apart in LDS
// (144 bytes): the 16 rows of a tile start in 16 different 16-byte slots of the 256-byte bank row; a ds_read_b128 lane
// group mixes two k-groups, which leaves at most a 2-way conflict on a pair of its lanes -- 8 reads against 32 MFMAs of
// 16 passes each per slab and wave, the reads do not show.
// Ragged edges: rows past the end read the last row (gram64_fetch_row: a valid address) and are masked by the caller
// where it uses the block; channels past C read channel 0 and are zeroed on the way into LDS.
// One bit pattern per pair: every element of every block, whichever kernel, tile, lane or operand side it is in, adds
// the products of its pair in the order of the ONE loop below -- slab by slab, step u = 0 .. 7 of a slab adds channels
// u, 8 + u, 16 + u, 24 + u in one MFMA, channels past C as zeros -- so a.b depends on (a, b, C) only and a.b == b.a.
#pragma once
#include "common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kGramBlock = 64;    // rows and columns of a Gram block per workgroup
constexpr int kGramSlab = 32;     // channels per K slab
constexpr int kGramLdsRow = 36;   // floats between rows of a slab in LDS

typedef float Gram64Lds[2][2][kGramBlock * kGramLdsRow];   // [buffer][A | B][row][k]

// the row of n that piece u = 0, 1 of this thread comes from in block b: rows tid >> 3 and 32 + (tid >> 3) of the block,
// clamped to the last row
__device__ __forceinline__ int gram64_fetch_row(int b, int u, int n) {
  return min(b * kGramBlock + (int)(threadIdx.x >> 3) + 32 * u, n - 1);
}

// acc = A B^T of the 64 rows at pa (this thread's two 16-byte pieces: the rows of gram64_fetch_row, floats
// 4 (tid & 7) ...) and the 64 rows at pb, all C channels (C % 4 == 0).  Wave (wi, wj) = (wave >> 1, wave & 1) owns rows
// 32 wi .. and columns 32 wj .. of the block; tile (ti, tj) register r of a lane (g = lane >> 4, c = lane & 15) is the
// element (32 wi + 16 ti + g + 4 r, 32 wj + 16 tj + c).  256 threads, all of them; ends after a barrier: LDS is free again.
__device__ __forceinline__ void gram64_block_product(int C, const float* const (&pa)[2], const float* const (&pb)[2],
                                                     Gram64Lds& lds, f64x4 (&acc)[2][2]) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int q = tid & 7, lrow = tid >> 3, wi = wave >> 1, wj = wave & 1;
  f32x4 ra[2], rb[2];
  auto fetch = [&](int k0) {
    const int k = k0 + 4 * q;
    const bool ok = k < C;          // C % 4 == 0: a piece is inside or outside as a whole
    const int kc = ok ? k : 0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const f32x4 va = *reinterpret_cast<const f32x4*>(pa[u] + kc), vb = *reinterpret_cast<const f32x4*>(pb[u] + kc);
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
      ra[u] = ok ? va : zero;
      rb[u] = ok ? vb : zero;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      *reinterpret_cast<f32x4*>(&lds[buf][0][(lrow + 32 * u) * kGramLdsRow + 4 * q]) = ra[u];
      *reinterpret_cast<f32x4*>(&lds[buf][1][(lrow + 32 * u) * kGramLdsRow + 4 * q]) = rb[u];
    }
  };
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[ti][tj][r] = 0.0;

  const int slabs = (C + kGramSlab - 1) / kGramSlab;
  fetch(0);
  stage(0);
  __syncthreads();
  for (int sl = 0; sl < slabs; ++sl) {
    const int buf = sl & 1;
    if (sl + 1 < slabs) fetch((sl + 1) * kGramSlab);
    f32x4 fa[2][2], fb[2][2];      // [tile][half]: floats 8 g + 4 half .. of row 16 tile + c
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        fa[tt][h] = *reinterpret_cast<const f32x4*>(&lds[buf][0][(32 * wi + 16 * tt + c) * kGramLdsRow + 8 * g + 4 * h]);
        fb[tt][h] = *reinterpret_cast<const f32x4*>(&lds[buf][1][(32 * wj + 16 * tt + c) * kGramLdsRow + 8 * g + 4 * h]);
      }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double a0 = (double)fa[0][h][e], a1 = (double)fa[1][h][e];
        const double b0 = (double)fb[0][h][e], b1 = (double)fb[1][h][e];
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
      }
    if (sl + 1 < slabs) stage(buf ^ 1);      // (the buffer the slab before this one was read from: every wave is past it)
    __syncthreads();
  }
}
