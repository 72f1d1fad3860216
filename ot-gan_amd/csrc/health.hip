// health.hip -- the reductions behind --health_every (utils/health.py): otgan_tensor_health_f32, the norms, maxima, zero and
// non-finite counts and the exponent histogram of a list of fp32 tensors (and of their differences to reference tensors) in one
// pass, and otgan_plan_marginals_f32, how far the row and column sums of Sinkhorn plans are from their targets.  The contracts
// are stated in include/otgan_layers.h.
//
// tensor_health.  A segment (one tensor) is cut into chunks of OTGAN_HEALTH_CHUNK elements counted from ITS OWN first element;
// one workgroup of 256 threads takes one chunk.  The chunk is staged in LDS -- scalar loads up to the first 16-byte boundary,
// 16-byte loads on the aligned body, scalar loads on the tail, x and ref each by its own alignment -- and is then read back by
// chunk-relative index: thread t adds the elements t, t + 256, ... in that order, the wave butterfly and the four wave sums in
// index order follow.  So the order of every fp64 sum is a function of the element's index in its segment alone: not of the
// pointer's alignment, not of the segments that share the launch.  The chunk's six numbers go to the workspace; the finishing
// launch (one workgroup per segment) adds a segment's chunks as thread t = chunks t, t + 256, ... and the same two tree steps.
// The histogram counts are integers: eight LDS copies per workgroup (lane & 7 picks the copy, so that a tensor whose elements
// share one exponent does not serialise a whole wave on one LDS word), summed and added to the output with integer atomics,
// whose result does not depend on arrival order.  No float atomics anywhere.
//
// x^2 is exact in fp64 (24-bit significands).  d = (double)x - (double)ref and d * d are single IEEE operations (no
// contraction into the sum), so the terms are the terms a numpy fp64 restatement forms and only the order of the sum differs.
//
// plan_marginals.  One workgroup per (problem, block of 64 rows): column sums of the block with lanes along the columns and the
// rows in order, then the block's row sums, one wave per row with lanes along the columns (the block's second read comes from
// cache).  The finishing launch adds the blocks' column partials in block order and takes the maxima and means.
#include "common.h"
#include "../../include/otgan.h"
#include "../../include/otgan_layers.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = OTGAN_HEALTH_CHUNK;
constexpr int kMaxSeg = OTGAN_HEALTH_MAX_SEGMENTS;
constexpr int kHistCopies = 8;
constexpr int kRowBlock = 64;

static_assert(kChunk % (4 * kThreads) == 0, "a chunk is whole rounds of 16-byte loads");

struct HealthSegs {
  const float* x[kMaxSeg];
  const float* ref[kMaxSeg];
  long n[kMaxSeg];
  int first[kMaxSeg + 1];      // chunks of this launch in front of segment s
};

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// slots 0, 2, 4, 5 are sums, 1 and 3 maxima of non-negative numbers
__device__ __forceinline__ double combine(int k, double a, double b) { return (k == 1 || k == 3) ? fmax(a, b) : a + b; }

// every thread of the workgroup calls this; thread 0 returns with the workgroup's six numbers in v
__device__ __forceinline__ void block_reduce6(double v[6], double (*s_red)[6]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    const double w = (k == 1 || k == 3) ? wave_max_d(v[k]) : wave_sum_d(v[k]);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][k] = w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = combine(k, combine(k, s_red[0][k], s_red[1][k]), combine(k, s_red[2][k], s_red[3][k]));
  }
}

// p[0, len) -> s[0, len), len <= kChunk, p 4-byte aligned
__device__ __forceinline__ void stage_chunk(const float* __restrict__ p, int len, float* s) {
  const int t = threadIdx.x;
  int head = (int)((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2;
  head = head < len ? head : len;
  if (t < head) s[t] = p[t];
  const int quads = (len - head) >> 2;
  const f32x4* pv = reinterpret_cast<const f32x4*>(p + head);
  if (head == 0) {
    for (int q = t; q < quads; q += kThreads) *reinterpret_cast<f32x4*>(s + 4 * q) = pv[q];
  } else {
    for (int q = t; q < quads; q += kThreads) {
      const f32x4 v = pv[q];
#pragma unroll
      for (int k = 0; k < 4; ++k) s[head + 4 * q + k] = v[k];
    }
  }
  const int done = head + 4 * quads;
  if (t < len - done) s[done + t] = p[done + t];
}

__global__ __launch_bounds__(kThreads) void health_chunk_kernel(HealthSegs segs, int nseg, double* __restrict__ partial,
                                                               unsigned long long* __restrict__ hist) {
  __shared__ __attribute__((aligned(16))) float s_x[kChunk];
  __shared__ __attribute__((aligned(16))) float s_r[kChunk];
  __shared__ unsigned s_hist[256 * kHistCopies];
  __shared__ double s_red[kThreads / 64][6];
  const int t = threadIdx.x;
  // the segment of this chunk: the last s with first[s] <= blockIdx.x (wave-uniform)
  int lo = 0, hi = nseg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (segs.first[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int seg = lo;
  const long c = (long)blockIdx.x - segs.first[seg];
  const long n = segs.n[seg];
  const long left = n - c * kChunk;
  const int len = left < kChunk ? (int)left : kChunk;
  const float* x = segs.x[seg] + c * kChunk;
  const float* ref = segs.ref[seg];
  for (int i = t; i < 256 * kHistCopies; i += kThreads) s_hist[i] = 0u;
  stage_chunk(x, len, s_x);
  if (ref) stage_chunk(ref + c * kChunk, len, s_r);
  __syncthreads();
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned mb = 0u;
  const int copy = t & (kHistCopies - 1);
  for (int e = t; e < len; e += kThreads) {
    const float xf = s_x[e];
    const unsigned b = __float_as_uint(xf) & 0x7fffffffu;
    if (b >= 0x7f800000u) {
      v[5] += 1.0;
      continue;
    }
    if (b == 0u) v[4] += 1.0;
    else atomicAdd(&s_hist[(b >> 23) * kHistCopies + copy], 1u);
    mb = b > mb ? b : mb;
    const double xd = (double)xf;
    v[0] = __dadd_rn(v[0], __dmul_rn(xd, xd));
    if (ref) {
      const float rf = s_r[e];
      if ((__float_as_uint(rf) & 0x7fffffffu) < 0x7f800000u) {
        const double d = __dsub_rn(xd, (double)rf);
        v[2] = __dadd_rn(v[2], __dmul_rn(d, d));
        v[3] = fmax(v[3], fabs(d));
      }
    }
  }
  v[1] = (double)__uint_as_float(mb);
  block_reduce6(v, s_red);        // (its barrier also orders the LDS histogram adds before the reads below)
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) partial[(long)blockIdx.x * 6 + k] = v[k];
  }
  unsigned cnt = 0u;
#pragma unroll
  for (int k = 0; k < kHistCopies; ++k) cnt += s_hist[t * kHistCopies + k];
  if (cnt) atomicAdd(&hist[(long)seg * 256 + t], (unsigned long long)cnt);
}

__global__ __launch_bounds__(kThreads) void health_finish_kernel(HealthSegs segs, const double* __restrict__ partial,
                                                                double* __restrict__ out) {
  __shared__ double s_red[kThreads / 64][6];
  const int seg = blockIdx.x;
  const long c0 = segs.first[seg], nch = segs.first[seg + 1] - c0;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long c = threadIdx.x; c < nch; c += kThreads) {
    const double* q = partial + (c0 + c) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = combine(k, v[k], q[k]);
  }
  block_reduce6(v, s_red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) out[(long)seg * 6 + k] = v[k];
  }
}

// part: double [P][RB][m + 2]: the block's column sums, then max and sum over its rows of |r_i - 1|
__global__ __launch_bounds__(kThreads) void marginals_block_kernel(const float* __restrict__ plan, int n, int m, long ldp,
                                                                  double* __restrict__ part) {
  __shared__ double s_row[kThreads / 64][2];
  const int p = blockIdx.y, rb = blockIdx.x, RB = gridDim.x;
  const int i0 = rb * kRowBlock, rows = min(kRowBlock, n - i0);
  const float* a = plan + ((long)p * n + i0) * ldp;
  double* out = part + ((long)p * RB + rb) * (m + 2);
  for (int j = threadIdx.x; j < m; j += kThreads) {
    double acc = 0.0;
    for (int i = 0; i < rows; ++i) acc += (double)a[i * ldp + j];
    out[j] = acc;
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double emax = 0.0, esum = 0.0;
  for (int i = wave; i < rows; i += kThreads / 64) {
    double acc = 0.0;
    for (int j = lane; j < m; j += 64) acc += (double)a[i * ldp + j];
    const double e = fabs(wave_sum_d(acc) - 1.0);
    emax = fmax(emax, e);
    esum += e;
  }
  if (lane == 0) { s_row[wave][0] = emax; s_row[wave][1] = esum; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[m] = fmax(fmax(s_row[0][0], s_row[1][0]), fmax(s_row[2][0], s_row[3][0]));
    out[m + 1] = (s_row[0][1] + s_row[1][1]) + (s_row[2][1] + s_row[3][1]);
  }
}

__global__ __launch_bounds__(kThreads) void marginals_finish_kernel(const double* __restrict__ part, int n, int m, int RB,
                                                                   double* __restrict__ out) {
  __shared__ double s_red[kThreads / 64][4];
  const int p = blockIdx.x;
  const double* q = part + (long)p * RB * (m + 2);
  const double target = (double)n / (double)m;
  double v[4] = {0.0, 0.0, 0.0, 0.0};      // row max, row sum, column max, column sum
  for (int rb = threadIdx.x; rb < RB; rb += kThreads) {
    v[0] = fmax(v[0], q[(long)rb * (m + 2) + m]);
    v[1] += q[(long)rb * (m + 2) + m + 1];
  }
  for (int j = threadIdx.x; j < m; j += kThreads) {
    double c = 0.0;
    for (int rb = 0; rb < RB; ++rb) c += q[(long)rb * (m + 2) + j];
    const double e = fabs(c - target);
    v[2] = fmax(v[2], e);
    v[3] += e;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double w = (k & 1) ? wave_sum_d(v[k]) : wave_max_d(v[k]);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][k] = w;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[p * 4 + 0] = fmax(fmax(s_red[0][0], s_red[1][0]), fmax(s_red[2][0], s_red[3][0]));
    out[p * 4 + 1] = ((s_red[0][1] + s_red[1][1]) + (s_red[2][1] + s_red[3][1])) / (double)n;
    out[p * 4 + 2] = fmax(fmax(s_red[0][2], s_red[1][2]), fmax(s_red[2][2], s_red[3][2]));
    out[p * 4 + 3] = ((s_red[0][3] + s_red[1][3]) + (s_red[2][3] + s_red[3][3])) / (double)m;
  }
}

long chunks_of(long n) { return (n + kChunk - 1) / kChunk; }

}  // namespace

extern "C" size_t otgan_tensor_health_workspace_bytes(const long* n, int nseg) {
  if (!n || nseg <= 0) return 0;
  long total = 0;
  for (int i = 0; i < nseg; ++i) {
    if (n[i] < 0) return 0;
    total += chunks_of(n[i]);
  }
  return (size_t)(total > 0 ? total : 1) * 6 * sizeof(double);
}

extern "C" int otgan_tensor_health_f32(const float* const* x, const float* const* ref, const long* n, int nseg, double* out,
                                       unsigned long long* hist, void* workspace, size_t workspace_bytes, void* stream) {
  OTGAN_CHECK_ARG(nseg >= 0, "tensor_health: nseg = %d", nseg);
  if (nseg == 0) return OTGAN_OK;
  OTGAN_CHECK_ARG(x && n && out && hist, "tensor_health: null x, n, out or hist");
  OTGAN_CHECK_ARG(((uintptr_t)out & 7) == 0 && ((uintptr_t)hist & 7) == 0, "tensor_health: out and hist must be 8-byte aligned");
  for (int i = 0; i < nseg; ++i) {
    OTGAN_CHECK_ARG(n[i] >= 0, "tensor_health: segment %d has n = %ld", i, n[i]);
    OTGAN_CHECK_ARG(n[i] == 0 || (x[i] && ((uintptr_t)x[i] & 3) == 0), "tensor_health: segment %d: x is null or not 4-byte aligned", i);
    OTGAN_CHECK_ARG(!ref || ((uintptr_t)ref[i] & 3) == 0, "tensor_health: segment %d: ref is not 4-byte aligned", i);
  }
  const size_t need = otgan_tensor_health_workspace_bytes(n, nseg);
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need) {
    otgan_set_error("tensor_health: the workspace needs %zu bytes, 8-byte aligned (given %zu)", need, workspace_bytes);
    return OTGAN_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(hist, 0, (size_t)nseg * 256 * sizeof(unsigned long long), s) != hipSuccess) {
    otgan_set_error("tensor_health: clearing the histogram failed");
    return OTGAN_ERR_LAUNCH;
  }
  double* partial = reinterpret_cast<double*>(workspace);
  // a launch takes as many segments as its argument struct holds and as many chunks as a grid: batches of both
  int s0 = 0;
  while (s0 < nseg) {
    HealthSegs segs;
    memset(&segs, 0, sizeof(segs));
    int k = 0;
    long chunks = 0;
    while (s0 + k < nseg && k < kMaxSeg) {
      const long c = chunks_of(n[s0 + k]);
      OTGAN_CHECK_ARG(c <= 0x7fffffffL, "tensor_health: segment %d has n = %ld (at most 2^31 - 1 chunks)", s0 + k, n[s0 + k]);
      if (k > 0 && chunks + c > 0x7fffffffL) break;
      segs.x[k] = x[s0 + k];
      segs.ref[k] = ref ? ref[s0 + k] : nullptr;
      segs.n[k] = n[s0 + k];
      segs.first[k] = (int)chunks;
      chunks += c;
      ++k;
    }
    for (int j = k; j <= kMaxSeg; ++j) segs.first[j] = (int)chunks;
    if (chunks > 0) {
      hipLaunchKernelGGL(health_chunk_kernel, dim3((unsigned)chunks), dim3(kThreads), 0, s, segs, k, partial, hist + (long)s0 * 256);
      OTGAN_CHECK_LAUNCH("tensor_health");
    }
    hipLaunchKernelGGL(health_finish_kernel, dim3((unsigned)k), dim3(kThreads), 0, s, segs, partial, out + (long)s0 * 6);
    OTGAN_CHECK_LAUNCH("tensor_health (finish)");
    partial += chunks * 6;
    s0 += k;
  }
  return OTGAN_OK;
}

extern "C" size_t otgan_plan_marginals_workspace_bytes(int P, int n, int m) {
  if (P <= 0 || n <= 0 || m <= 0) return 0;
  return (size_t)P * ceil_div(n, kRowBlock) * ((size_t)m + 2) * sizeof(double);
}

extern "C" int otgan_plan_marginals_f32(const float* plan, int P, int n, int m, long ldp, double* out, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  OTGAN_CHECK_ARG(P >= 0 && P <= 65535, "plan_marginals: P = %d (0 ... 65535)", P);
  if (P == 0) return OTGAN_OK;
  OTGAN_CHECK_ARG(plan && out, "plan_marginals: null plan or out");
  OTGAN_CHECK_ARG(n >= 1 && m >= 1 && ldp >= m, "plan_marginals: n = %d, m = %d, ldp = %ld", n, m, ldp);
  OTGAN_CHECK_ARG((long)kRowBlock * ldp <= 0x7fffffffL, "plan_marginals: ldp = %ld (at most 2^25)", ldp);
  OTGAN_CHECK_ARG(((uintptr_t)plan & 3) == 0 && ((uintptr_t)out & 7) == 0, "plan_marginals: plan or out misaligned");
  const size_t need = otgan_plan_marginals_workspace_bytes(P, n, m);
  if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < need) {
    otgan_set_error("plan_marginals: the workspace needs %zu bytes, 8-byte aligned (given %zu)", need, workspace_bytes);
    return OTGAN_ERR_WORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const int RB = ceil_div(n, kRowBlock);
  double* part = reinterpret_cast<double*>(workspace);
  hipLaunchKernelGGL(marginals_block_kernel, dim3((unsigned)RB, (unsigned)P), dim3(kThreads), 0, s, plan, n, m, ldp, part);
  OTGAN_CHECK_LAUNCH("plan_marginals");
  hipLaunchKernelGGL(marginals_finish_kernel, dim3((unsigned)P), dim3(kThreads), 0, s, part, n, m, RB, out);
  OTGAN_CHECK_LAUNCH("plan_marginals (finish)");
  return OTGAN_OK;
}
