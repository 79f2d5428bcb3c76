// sift_match_common.h -- what the two brute-force matchers (sift_match.hip: fp32 MFMA, sift_match8.hip: int8 MFMA) share
// on the device: the write-out of a (best, second, index) triple, the frame of a pair-list workgroup, the fold of the
// partial results and the "partial or final" sink of a main kernel.  Device code only.
#pragma once

#include "sift_device.h"

namespace cusift {

// ---- write-out ---------------------------------------------------------------------------------------------------------
// the 1e-6 is a double constant in the reference (extras/matching.cu:143,222): evaluate in double, store float
__device__ __forceinline__ float match_ambiguity(float best, float second, bool l2) {
  return l2 ? (float)(best / (second + 1e-6)) : (float)((1 - best) / (1 - second + 1e-6));
}

// the tail of FindMinCorr/FindMaxCorr (extras/matching.cu:140-150,220-229): the five fields MatchSiftData fills
__device__ __forceinline__ void write_match(cusift_point *pt, const cusift_point *__restrict__ sift2, int n2,
                                            float best, float second, int idx, bool l2) {
  pt->score = best;
  pt->ambiguity = match_ambiguity(best, second, l2);
  pt->match = idx;
  const int m = (idx >= 0 && idx < n2) ? idx : 0;  // the reference reads sift2[-1] here
  pt->match_xpos = sift2[m].coords2D[0];
  pt->match_ypos = sift2[m].coords2D[1];
}

// the pair-list calls' form of it: rows[pair][max_pts] (score, ambiguity, match: write_match's arithmetic), never the
// records, so that a frame can be the first member of any number of pairs
__device__ __forceinline__ void write_match_row(cusift_match_row *__restrict__ row, float best, float second, int idx,
                                                bool l2) {
  f4 v;
  v[0] = best;
  v[1] = match_ambiguity(best, second, l2);
  v[2] = __int_as_float(idx);
  v[3] = 0.0f;  // reserved
  *reinterpret_cast<f4 *>(row) = v;
}

// ---- the pair-list frame -----------------------------------------------------------------------------------------------
// points[n_images][max_pts] + counters[n_images] as cusift_extract_batch leaves them; pairs[p] = (frame 1, frame 2).  The
// two record counts come from device memory (clamped to max_pts like rgbd_lift_kernel's); the grids are sized from
// max_pts because the host does not know them.  PairCounts is what a batch merge kernel needs of its pair.
struct PairCounts {
  int pair, f1, f2, n1, n2;
  __device__ __forceinline__ PairCounts(int pair_, const unsigned int *__restrict__ counters,
                                        const int *__restrict__ pairs, int max_pts)
      : pair(pair_),
        f1(pairs[2 * pair_]),
        f2(pairs[2 * pair_ + 1]),
        n1(frame_count(counters, f1, max_pts)),
        n2(frame_count(counters, f2, max_pts)) {}
};

// A main kernel's workgroup (row block blockIdx.x, column split blockIdx.y, pair blockIdx.z): its columns
// [col_begin, col_end) and `empty`, the workgroup-uniform "no rows or no columns".  An empty workgroup returns before it
// loads a record, initialises anything or reaches a barrier.
struct PairFrame : PairCounts {
  int col_begin, col_end;
  bool empty;
  __device__ __forceinline__ PairFrame(const unsigned int *__restrict__ counters, const int *__restrict__ pairs,
                                       int max_pts, int cols_per_split, int rows_per_block)
      : PairCounts(blockIdx.z, counters, pairs, max_pts),
        col_begin(blockIdx.y * cols_per_split),
        col_end(min(col_begin + cols_per_split, n2)),
        empty((int)blockIdx.x * rows_per_block >= n1 || col_begin >= n2) {}
};

// ---- the fold of a merge kernel ----------------------------------------------------------------------------------------
// first[0], then first[stride], ... first[(count - 1) stride] merged into it in that order: the column splits of a row in
// column order, or the row blocks of a column in ascending row order.  merge(m, o): o's columns (rows) lie above m's.
template <class Partial, class Merge>
__device__ __forceinline__ Partial fold_partials(const Partial *__restrict__ first, size_t stride, int count,
                                                 const Merge &merge) {
  Partial m = first[0];
  for (int s = 1; s < count; ++s) {
    const Partial o = first[(size_t)s * stride];  // one load of the whole partial, not one per field where it is used
    merge(m, o);
  }
  return m;
}

// ---- the sink of a main kernel -----------------------------------------------------------------------------------------
// What a main kernel does with the triple of row (or column) i: with partials -- several column splits, or several row
// blocks on the column side -- it goes to partials[slab + i] for the merge kernel, otherwise it is final.  The two
// addressing forms, a record set and a row array, differ in `final(i, best, second, idx)` alone.
template <class Partial, class Final>
__device__ __forceinline__ auto partial_or(Partial *partials, size_t slab, Final final) {
  return [=](int i, auto best, auto second, int idx) {
    if (partials)
      partials[slab + i] = Partial{best, second, idx};
    else
      final(i, best, second, idx);
  };
}

}  // namespace cusift
