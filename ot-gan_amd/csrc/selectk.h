// selectk.h -- the k-best selection stage of the fused neighbour searches: knn.hip (the k smallest squared distances),
// topk.hip (the k largest dot products with their columns) and pixnn.hip (the k smallest integer distances with their
// columns).  Each of them forms a block of a product matrix per step and never writes it; what a file keeps to itself is
// the product, the score it forms from it, the ORDER it ranks by and its masks.  Everything after that is here, once.
//
// The order.  A kernel names a policy P with
//     P::Entry                  what a list holds (a value, a (score, column) pair, a packed key),
//     P::none()                 the entry of an empty slot and of a masked element: after every real entry,
//     P::exchange(slot, v)      leaves the earlier of the two in slot and the later in v (the compare-exchange primitive,
//                               not a predicate: each order keeps its own instructions -- a min and a max, or selects),
//     P::shfl_xor(e, offset)    the entry of the lane `offset` away.
// The order must be TOTAL on the entries a row can meet: values alone (equal values are interchangeable), or pairs in which
// a column occurs once per row.  Then the first KL of a set of entries are one definite list, so
//     a list is a function of the SET of entries it was offered,
// and so is every merge of lists: the outputs depend neither on the order in which the columns are visited nor on how they
// are split over lanes, waves and workgroups -- bit for bit, which the tests assert by permuting columns and moving splits.
//
// The lists.  A lane keeps one sorted list of KL entries per row it owns, in registers with static indices; sel_insert is
// a chain of KL exchanges in which the last of the KL + 1 falls out.  KL = 4 serves k <= 4 and KL = kSelMaxK = 8 the
// rest: the short lists are what lets two workgroups share a CU at the usual k = 3.  Masked elements (ragged rows, ragged
// columns, the excluded column) are offered as none() and never displace a real entry.
//
// The merges.  The holders of a row -- the lanes of a wave that saw different columns of it, times the two waves of the
// workgroup that did -- are merged ONCE, after the last column block: sel_merge_lanes is an xor tree over the lanes,
// after which each holds the merged list; one lane per row and wave writes it to LDS [2][rows][KL], and after the barrier
// sel_merge_waves, one thread per row, merges the two and stores the first k to the workspace, [split][row][k].
// (The steps of the tree stay a loop: it runs once per workgroup, and fully unrolled -- rows x steps x KL x KL exchanges
// on top of the block loop's -- the compiler did not finish topk.hip in 40 minutes; as a loop it takes seconds.)
//
// The column split.  With few query blocks the column blocks are split over blockIdx.y (sel_plan: about kSelGroups
// workgroups, at least kSelMinPer column blocks each).  A second launch, one thread per row, merges the splits of the row
// with sel_merge_splits and formats the outputs -- always, also for one split: two launches whatever the shape, one code
// path, and NO atomics anywhere.  With no split at all (no columns) the merged list is all none().
// (sel_merge_waves and sel_merge_splits read and write whole entries; topk.hip, which keeps the two halves of its pairs in
// two arrays, spells the same two merges out on sel_insert: the reason is in its header.)
#pragma once
#include <hip/hip_runtime.h>

constexpr int kSelMaxK = 8;       // length of the long register lists: the largest k
constexpr int kSelMinPer = 4;     // fewest column blocks a split is worth
constexpr int kSelGroups = 1024;  // workgroups the column split aims at

struct SelPlan {
  int nbq, nbc, per, splits;      // query blocks, column blocks, column blocks per split, splits
};

// tile: the queries and the columns of a block step (long: ny + tile may pass 2^31)
inline SelPlan sel_plan(int nq, int ny, int tile) {
  SelPlan p;
  p.nbq = (int)(((long)nq + tile - 1) / tile);
  p.nbc = (int)(((long)ny + tile - 1) / tile);
  p.per = p.splits = 0;
  if (p.nbq == 0 || p.nbc == 0) return p;
  const int want = (kSelGroups + p.nbq - 1) / p.nbq;
  p.per = (p.nbc + want - 1) / want;
  if (p.per < kSelMinPer) p.per = kSelMinPer;
  p.splits = (p.nbc + p.per - 1) / p.per;
  return p;
}

template <class P, int KL>
__device__ __forceinline__ void sel_fill(typename P::Entry (&list)[KL]) {
#pragma unroll
  for (int t = 0; t < KL; ++t) list[t] = P::none();
}

// v into the sorted list, the last of the KL + 1 falls out
template <class P, int KL>
__device__ __forceinline__ void sel_insert(typename P::Entry (&list)[KL], typename P::Entry v) {
#pragma unroll
  for (int t = 0; t < KL; ++t) P::exchange(list[t], v);
}

// xor tree over the lanes first_offset, 2 first_offset, ... < end_offset apart, which hold lists of the same row
template <class P, int KL>
__device__ __forceinline__ void sel_merge_lanes(typename P::Entry (&list)[KL], int first_offset, int end_offset) {
#pragma unroll 1
  for (int o = first_offset; o < end_offset; o <<= 1) {
    typename P::Entry other[KL];
#pragma unroll
    for (int t = 0; t < KL; ++t) other[t] = P::shfl_xor(list[t], o);
#pragma unroll
    for (int t = 0; t < KL; ++t) sel_insert<P>(list, other[t]);
  }
}

// a, b: the lists the two waves of a row left in LDS; the first k of their merge go to part
template <class P, int KL>
__device__ __forceinline__ void sel_merge_waves(const typename P::Entry (&a)[KL], const typename P::Entry (&b)[KL], int k,
                                                typename P::Entry* __restrict__ part) {
  typename P::Entry m[KL];
#pragma unroll
  for (int t = 0; t < KL; ++t) m[t] = a[t];
#pragma unroll
  for (int t = 0; t < KL; ++t) sel_insert<P>(m, b[t]);
#pragma unroll
  for (int t = 0; t < KL; ++t)
    if (t < k) part[t] = m[t];
}

// m = the merge of row i's lists of k entries in part, [splits][nq][k]; entries of m from k on are none()
template <class P>
__device__ __forceinline__ void sel_merge_splits(typename P::Entry (&m)[kSelMaxK], const typename P::Entry* __restrict__ part,
                                                 long i, int nq, int k, int splits) {
  sel_fill<P>(m);
  for (int s = 0; s < splits; ++s) {
    const long at = ((long)s * nq + i) * k;
#pragma unroll
    for (int t = 0; t < kSelMaxK; ++t)
      if (t < k) sel_insert<P>(m, part[at + t]);
  }
}
