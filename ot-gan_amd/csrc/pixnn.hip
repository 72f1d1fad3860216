// pixnn.hip -- exact nearest neighbours of uint8 images in pixel space (utils/authenticity.py), on the int8 matrix pipe:
//   * otgan_nn_u8: for every query row q_i and the columns y_j with j != self0 + i,
//       index[i][0 .. k) = the columns of the k smallest d(q_i, y_j) = sum_d (q_id - y_jd)^2 over the raw uint8 values,
//       dist[i][0 .. k)  = those values,
//     sorted by distance ascending, equal distances by the smaller column first ((-1, -1) where fewer were counted).
// The selection -- lists, merges, column split, second launch -- is selectk.h's; the product, the score and the order are
// this file's.  Operands: a byte x becomes the int8 x - 128 while it is staged (x ^ 0x80), which changes no difference;
// with a = q - 128, b = y - 128
//       d = |a|^2 + |b|^2 - 2 a.b,
// a.b from v_mfma_i32_16x16x64_i8 (int32 accumulators), the norms from a pre-pass into the workspace.  Bounds, D <= 49152:
//   |a.b| and the norms <= D 2^14 <= 805 306 368 < 2^31 -- int32 holds every partial sum, products and sums are EXACT;
//   d <= D 255^2 <= 3 196 108 800: past int32, inside uint32.  The epilogue adds the three terms in unsigned 32 bits (the true
//   value is in range, so the wrapped sum is it) and packs (d << 32) | j into one 64-bit key: plain unsigned order on the
//   key is the pair order above -- total, since a column occurs once per row -- and an exchange is one 64-bit min and max.
//   Integers throughout: the outputs are exact, with no tolerance anywhere.
// A masked element (ragged row, ragged column, the excluded column) is the key ~0: above every real key (d < 2^32 - 1).
// Tile: a workgroup of four waves (2 x 2) takes 128 queries x 128 columns per block step, K in chunks of 128 bytes through
// LDS (rows of 144 bytes: the 16 rows a fragment load touches fall on 16 different bank quads), the next chunk in flight in
// registers while this one multiplies; two workgroups per CU (at most 256 registers, 52 KB of LDS each) cover each other's
// barriers and load latency.  The product is computed TRANSPOSED, C = Y Q^T: the C/D map of the 16 x 16 forms has
// the column on the lane (lane & 15) and the rows in the 4 registers, so a lane then owns 4 queries (one per 16-wide query
// tile of its wave) and sees 16 columns of each per block step -- 4 sorted lists per lane, 2 KL registers each, instead of
// 16.  A value enters its list only when it is below the list's last key: after the first blocks almost none does, and the
// epilogue is a compare per value.  The A/B lane map (which k a lane's 16 bytes are) does not matter as long as both
// operands are fetched alike: a dot product is a sum over k in any order, and integer sums are exact.
// K tail: 16-byte units at or past D are staged as int8 zeros in both operands (D % 16 == 0).
// The holders of a query are 8: 4 lane groups x the 2 waves of a query half.
// Workspace: [splits][nq][k] uint64 keys, then nq + ny int32 norms (queries first).
#include "common.h"
#include "selectk.h"
#include "../../include/otgan.h"
#include "../../include/otgan_layers.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int kNnTile = 128;        // queries and columns of a block step
constexpr int kNnChunk = 128;       // bytes of K per staged chunk
constexpr int kNnPitch = 144;       // LDS row pitch in bytes
constexpr int kNnMaxD = 49152;

// packed (distance << 32) | column keys ascending
struct NnOrder {
  typedef u64 Entry;
  static __device__ __forceinline__ u64 none() { return ~0ull; }
  static __device__ __forceinline__ void exchange(u64& slot, u64& v) {
    const u64 a = slot;
    slot = a < v ? a : v;
    v = a < v ? v : a;
  }
  static __device__ __forceinline__ u64 shfl_xor(u64 e, int o) { return __shfl_xor(e, o, 64); }
};

inline size_t nn_key_slots(const SelPlan& p, int nq, int k) { return (size_t)p.splits * (size_t)nq * (size_t)k; }

// norm[r] = sum_d (x_rd - 128)^2, one wave per row and trip of the grid, 16 bytes per lane and trip of the row
__global__ __launch_bounds__(256) void nn_norm_kernel(long rows, int D, const uint8_t* __restrict__ x, long ld, int* __restrict__ norm) {
  const int lane = threadIdx.x & 63;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * 4) {
  const uint4* p = reinterpret_cast<const uint4*>(x + r * ld);
  int s = 0;
  for (int u = lane; u < D / 16; u += 64) {
    const uint4 v = p[u];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int t = (int)((w[e] >> (8 * b)) & 255u) - 128;
        s += t * t;
      }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) norm[r] = s;
  }
}

inline unsigned nn_norm_grid(long rows) { return (unsigned)min((rows + 3) / 4, 1l << 20); }

// grid (query blocks, splits), 256 threads.  part: [splits][nq][k] keys.  KL >= k: the length of the lists
template <int KL>
__global__ __launch_bounds__(256, 2) void nn_block_kernel(int nq, int ny, int D, const uint8_t* __restrict__ q, long ldq,
                                                       const uint8_t* __restrict__ y, long ldy, int k, int self0, int per,
                                                       const int* __restrict__ qnorm, const int* __restrict__ ynorm,
                                                       u64* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) unsigned char sq[kNnTile * kNnPitch];
  __shared__ __attribute__((aligned(16))) unsigned char sy[kNnTile * kNnPitch];
  __shared__ u64 wave_keys[2][kNnTile][KL];        // [wy][query of the block][entry]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, c = lane & 15;
  const int wy = wave >> 1, wq = wave & 1;
  const int bi = blockIdx.x, nbc = (ny + kNnTile - 1) / kNnTile;
  const int jb0 = blockIdx.y * per, jb1 = min(jb0 + per, nbc);
  const int nchunks = (D + kNnChunk - 1) / kNnChunk;

  // staging: unit u = tid + 256 e of a tile is 16 bytes, row u >> 3, byte offset 16 (u & 7) of the chunk
  const uint8_t* pq[4];
  int lds_at[4];
  const int ku = 16 * (tid & 7);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int row = (tid + 256 * e) >> 3;
    pq[e] = q + (long)min((unsigned)bi * kNnTile + row, (unsigned)nq - 1u) * ldq + ku;
    lds_at[e] = row * kNnPitch + ku;
  }

  // slot b of this lane is query 64 wq + 16 b + c of the block; the guards as two ints per query: its columns end at jend
  // (0 past nq: none is counted), selfj is the excluded one (~0: none).  Row and column numbers are unsigned here:
  // the last block of ny = 2^31 - 2 columns runs past 2^31
  u64 lst[4][KL];
  unsigned selfj[4], jend[4], qn[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const unsigned i = (unsigned)bi * kNnTile + 64 * wq + 16 * b + c;
    jend[b] = i < (unsigned)nq ? (unsigned)ny : 0u;
    qn[b] = i < (unsigned)nq ? (unsigned)qnorm[i] : 0u;
    selfj[b] = (self0 >= 0 && (long)self0 + (long)i < ny) ? (unsigned)self0 + i : ~0u;
    sel_fill<NnOrder>(lst[b]);
  }

  for (int jb = jb0; jb < jb1; ++jb) {
    const uint8_t* py[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) py[e] = y + (long)min((unsigned)jb * kNnTile + ((tid + 256 * e) >> 3), (unsigned)ny - 1u) * ldy + ku;

    i32x4 acc[4][4];                     // [column tile a][query tile b]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = i32x4{0, 0, 0, 0};

    uint4 rq[4], ry[4];
    // a unit at or past D reads its row's first unit instead (a valid address) and becomes int8 zeros after the ^ 0x80
#define NN_FETCH(ch)                                                                        \
  {                                                                                         \
    const bool in = (ch) * kNnChunk + ku < D;                                               \
    const long off = in ? (long)(ch) * kNnChunk : -(long)ku;                                \
    const unsigned fill = in ? 0u : 0xffffffffu, pad = in ? 0u : 0x80808080u;               \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                         \
      const uint4 vq = *reinterpret_cast<const uint4*>(pq[e] + off);                        \
      const uint4 vy = *reinterpret_cast<const uint4*>(py[e] + off);                        \
      rq[e] = make_uint4((vq.x & ~fill) | pad, (vq.y & ~fill) | pad, (vq.z & ~fill) | pad, (vq.w & ~fill) | pad); \
      ry[e] = make_uint4((vy.x & ~fill) | pad, (vy.y & ~fill) | pad, (vy.z & ~fill) | pad, (vy.w & ~fill) | pad); \
    }                                                                                       \
  }
    NN_FETCH(0)
    for (int ch = 0; ch < nchunks; ++ch) {
      __syncthreads();                   // the last chunk (and the last block's) has been read
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned m = 0x80808080u;
        *reinterpret_cast<uint4*>(sq + lds_at[e]) = make_uint4(rq[e].x ^ m, rq[e].y ^ m, rq[e].z ^ m, rq[e].w ^ m);
        *reinterpret_cast<uint4*>(sy + lds_at[e]) = make_uint4(ry[e].x ^ m, ry[e].y ^ m, ry[e].z ^ m, ry[e].w ^ m);
      }
      __syncthreads();
      if (ch + 1 < nchunks) NN_FETCH(ch + 1)
#pragma unroll
      for (int kk = 0; kk < kNnChunk / 64; ++kk) {
        if (ch * kNnChunk + kk * 64 >= D) break;           // a half past D holds zeros only
        i32x4 fy[4], fq[4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
          fy[a] = *reinterpret_cast<const i32x4*>(sy + (64 * wy + 16 * a + c) * kNnPitch + 64 * kk + 16 * g);
#pragma unroll
        for (int b = 0; b < 4; ++b)
          fq[b] = *reinterpret_cast<const i32x4*>(sq + (64 * wq + 16 * b + c) * kNnPitch + 64 * kk + 16 * g);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fy[a], fq[b], acc[a][b], 0, 0, 0);
      }
    }

#undef NN_FETCH
    // register r of acc[a][b] is column jb 128 + 64 wy + 16 a + 4 g + r against query slot b
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned j = (unsigned)jb * kNnTile + 64 * wy + 16 * a + 4 * g + r;
        const unsigned yn = (unsigned)ynorm[min(j, (unsigned)ny - 1u)];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const unsigned d = qn[b] + yn - 2u * (unsigned)acc[a][b][r];
          const bool counted = j < jend[b] && j != selfj[b];
          const u64 key = counted ? (((u64)d << 32) | j) : NnOrder::none();
          if (key < lst[b][KL - 1]) sel_insert<NnOrder>(lst[b], key);
        }
      }
  }

  // the 4 lane groups of a wave hold different columns of the same queries
#pragma unroll
  for (int b = 0; b < 4; ++b) sel_merge_lanes<NnOrder>(lst[b], 16, 64);
  if (g == 0) {
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int t = 0; t < KL; ++t) wave_keys[wy][64 * wq + 16 * b + c][t] = lst[b][t];
  }
  __syncthreads();
  // the two waves of a query half, one thread per query
  const unsigned i = (unsigned)bi * kNnTile + tid;
  if (tid < kNnTile && i < (unsigned)nq)
    sel_merge_waves<NnOrder>(wave_keys[0][tid], wave_keys[1][tid], k, part + ((long)blockIdx.y * nq + i) * k);
}

// one thread per query row: the first k keys of its splits' lists (splits == 0: every slot empty); an empty slot leaves
// as (-1, -1)
__global__ __launch_bounds__(256) void nn_merge_kernel(int nq, int k, int splits, const u64* __restrict__ part,
                                                       int* __restrict__ index, long long* __restrict__ dist) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  u64 m[kSelMaxK];
  sel_merge_splits<NnOrder>(m, part, i, nq, k, splits);
#pragma unroll
  for (int t = 0; t < kSelMaxK; ++t)
    if (t < k) {
      const bool none = m[t] == NnOrder::none();
      index[i * k + t] = none ? -1 : (int)(unsigned)(m[t] & 0xffffffffull);
      dist[i * k + t] = none ? -1ll : (long long)(m[t] >> 32);
    }
}

inline size_t nn_norm_bytes(int nq, int ny) { return ((((size_t)nq + (size_t)ny) * sizeof(int32_t)) + 7) & ~(size_t)7; }

}  // namespace

extern "C" {

size_t otgan_nn_u8_workspace_bytes(int nq, int ny, int k) {
  if (nq <= 0 || ny <= 0 || k < 1 || k > kSelMaxK) return 0;
  return nn_key_slots(sel_plan(nq, ny, kNnTile), nq, k) * sizeof(u64) + nn_norm_bytes(nq, ny);
}

int otgan_nn_u8(int nq, int ny, int D, const uint8_t* q, long ldq, const uint8_t* y, long ldy, int k, int self0,
                int32_t* index, int64_t* dist, void* workspace, size_t workspace_bytes, void* stream) {
  OTGAN_CHECK_ARG(nq >= 0 && ny >= 0 && ny <= 0x7ffffffe, "otgan_nn_u8: nq %d >= 0, ny %d in 0 ... 2^31 - 2", nq, ny);
  OTGAN_CHECK_ARG(D >= 16 && D <= kNnMaxD && D % 16 == 0, "otgan_nn_u8: D %d a multiple of 16 in 16 ... %d", D, kNnMaxD);
  OTGAN_CHECK_ARG(ldq >= D && ldy >= D && ldq % 16 == 0 && ldy % 16 == 0,
                  "otgan_nn_u8: ldq %ld and ldy %ld >= D %d and multiples of 16", ldq, ldy, D);
  OTGAN_CHECK_ARG(k >= 1 && k <= kSelMaxK && self0 >= -1, "otgan_nn_u8: k %d in 1 ... %d, self0 %d >= -1", k, kSelMaxK, self0);
  OTGAN_CHECK_ARG(((index && dist) || nq == 0) && (q || nq == 0) && (y || ny == 0), "otgan_nn_u8: null argument");
  OTGAN_CHECK_ARG((reinterpret_cast<uintptr_t>(q) & 15) == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(index) & 3) == 0 && (reinterpret_cast<uintptr_t>(dist) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                  "otgan_nn_u8: misaligned pointer (rows 16 bytes, dist and workspace 8, index 4)");
  if (nq == 0) return OTGAN_OK;
  const SelPlan p = sel_plan(nq, ny, kNnTile);
  if (ny > 0 && (!workspace || workspace_bytes < otgan_nn_u8_workspace_bytes(nq, ny, k))) {
    otgan_set_error("otgan_nn_u8: workspace of %zu bytes, otgan_nn_u8_workspace_bytes(%d, %d, %d) = %zu", workspace_bytes, nq,
                    ny, k, otgan_nn_u8_workspace_bytes(nq, ny, k));
    return OTGAN_ERR_WORKSPACE;
  }
  hipStream_t st = (hipStream_t)stream;
  u64* part = nullptr;
  if (ny > 0) {
    part = static_cast<u64*>(workspace);
    int* qnorm = reinterpret_cast<int*>(part + nn_key_slots(p, nq, k));
    int* ynorm = qnorm + nq;
    hipLaunchKernelGGL(nn_norm_kernel, dim3(nn_norm_grid(nq)), dim3(256), 0, st, (long)nq, D, q, ldq, qnorm);
    OTGAN_CHECK_LAUNCH("otgan_nn_u8 (query norms)");
    hipLaunchKernelGGL(nn_norm_kernel, dim3(nn_norm_grid(ny)), dim3(256), 0, st, (long)ny, D, y, ldy, ynorm);
    OTGAN_CHECK_LAUNCH("otgan_nn_u8 (column norms)");
    auto kernel = k <= 4 ? nn_block_kernel<4> : nn_block_kernel<kSelMaxK>;
    hipLaunchKernelGGL(kernel, dim3(p.nbq, p.splits), dim3(256), 0, st, nq, ny, D, q, ldq, y, ldy, k, self0, p.per,
                       (const int*)qnorm, (const int*)ynorm, part);
    OTGAN_CHECK_LAUNCH("otgan_nn_u8");
  }
  hipLaunchKernelGGL(nn_merge_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, nq, k, p.splits, (const u64*)part,
                     (int*)index, (long long*)dist);
  OTGAN_CHECK_LAUNCH("otgan_nn_u8 (merge)");
  return OTGAN_OK;
}

}  // extern "C"
