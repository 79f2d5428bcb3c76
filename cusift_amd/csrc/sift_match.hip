// sift_match.hip -- brute-force descriptor matcher (the first consumer of SiftData).
// Reference: MatchSiftData, extras/matching.cu:232-362 = ComputeDistance (:12-58) + ComputeL2Distance (:63-74) +
// FindMaxCorr (:76-152) / FindMinCorr (:154-230).
//
// The reference materialises the numPts1 x numPts2 score matrix in memory and scans it a second time.  Here one
// kernel does both: a wave owns 16 descriptors of image 1 (their 128 floats stay in registers as MFMA A fragments),
// the workgroup streams image 2 through LDS in tiles of 32 descriptors, the 16x16 dot products come from
// v_mfma_f32_16x16x4_f32 (exact fp32: a k-ordered fmaf chain, no reduced-precision path), and every lane keeps the
// running (best, second, index) of its rows for the columns it sees -- exactly what reference thread `tx` sees
// (columns tx, tx+16, ...), followed by the reference's tree over tx.  N1*N2*4 bytes of HBM traffic never exist.
// The next tile's global loads are in flight while the current one is multiplied (register staging), and image 2's
// columns are split over blockIdx.y so that a few thousand keypoints still fill the chip; per-split results are
// folded in column order by match_merge_kernel (equal to the single scan except for exact score ties between
// columns of different splits).
//
// Numerics: the reference sums pt1[k]*pt2[k] starting at k = (p2 mod 16) and wrapping; the MFMA chain visits k in
// the order 16u+j, 16u+4+j, 16u+8+j, 16u+12+j (u = 0..7, j = 0..3).  Scores agree to ~1e-7; indices agree except
// for exact-score near-ties (tests bound both).
#include "sift_device.h"


namespace cusift {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMatchRowsPerBlock = 64;  // 4 waves x 16 descriptors of image 1
constexpr int kMatchTileCols = 32;      // descriptors of image 2 per LDS tile
constexpr int kBStride = 132;           // floats per LDS row: 16-byte aligned and conflict-free for ds_read_b128
constexpr float kMatchFltMax = 999.0f;  // extras/matching.cu:3

// (val, idx) beats (best) under the reference's strict comparison; L2 looks for minima, dot product for maxima
__device__ __forceinline__ bool beats(float val, float cur, bool l2) { return l2 ? (val < cur) : (val > cur); }

// FindMinCorr/FindMaxCorr inner update (extras/matching.cu:104-113,182-191)
__device__ __forceinline__ void top2_scan(float &best, float &second, int &idx, float val, int i, bool l2) {
  if (beats(val, best, l2)) {
    second = best;
    best = val;
    idx = i;
  } else if (beats(val, second, l2)) {
    second = val;
  }
}

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

// 16-byte loads from the 588-byte records: descriptors are only 4-byte aligned
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));

// The same update without branches: two compares and four selects per score (a NaN score changes nothing, as in the
// reference: both comparisons are false).
template <bool kL2>
__device__ __forceinline__ void top2_update(float &best, float &second, int &idx, float val, int i) {
  const bool win = kL2 ? (val < best) : (val > best);
  const bool place = kL2 ? (val < second) : (val > second);
  second = win ? best : (place ? val : second);
  idx = win ? i : idx;
  best = win ? val : best;
}

// One workgroup = 64 descriptors of image 1 (16 per wave) x one contiguous range of image 2's columns
// (blockIdx.y = column split; the host picks the number of splits so that the grid fills 256 CUs even for a few
// thousand keypoints).  With one split the kernel writes the final fields; otherwise the (best, second, index)
// partial of every row goes to `partials[split][row]` and match_merge_kernel folds the splits in column order.
template <bool kL2>
__global__ void __launch_bounds__(256) match_kernel(cusift_point *__restrict__ sift1, int n1,
                                                   const cusift_point *__restrict__ sift2, int n2,
                                                   int cols_per_split, MatchPartial *__restrict__ partials,
                                                   int n1_pad) {
  __shared__ float sB[kMatchTileCols * kBStride];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int p1_base = blockIdx.x * kMatchRowsPerBlock + wv * 16;
  const int col_begin = blockIdx.y * cols_per_split;
  const int col_end = min(col_begin + cols_per_split, n2);  // padded columns (:57) can never win: skip them
  constexpr float kInit = kL2 ? kMatchFltMax : -1.0f;       // also what a masked column scores: it changes nothing

#include "match_tile.inc"
  if (r == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p1 = p1_base + 4 * g + q;
      if (p1 >= n1) continue;
      if (partials) {
        MatchPartial mp;
        mp.best = best[q];
        mp.second = second[q];
        mp.idx = bidx[q];
        partials[(size_t)blockIdx.y * n1_pad + p1] = mp;
      } else {
        write_match(sift1 + p1, sift2, n2, best[q], second[q], bidx[q], kL2);
      }
    }
  }
}

template __global__ void match_kernel<false>(cusift_point *, int, const cusift_point *, int, int, MatchPartial *, int);
template __global__ void match_kernel<true>(cusift_point *, int, const cusift_point *, int, int, MatchPartial *, int);

// Folds the column splits of one row in column order: the same update the tree applies between lanes.
__global__ void __launch_bounds__(256) match_merge_kernel(cusift_point *__restrict__ sift1, int n1,
                                                         const cusift_point *__restrict__ sift2, int n2, int l2_mode,
                                                         const MatchPartial *__restrict__ partials, int n1_pad,
                                                         int n_splits) {
  const bool l2 = l2_mode != 0;
  const int p1 = blockIdx.x * 256 + threadIdx.x;
  if (p1 >= n1) return;
  MatchPartial m = partials[p1];
  for (int s = 1; s < n_splits; ++s) {
    const MatchPartial o = partials[(size_t)s * n1_pad + p1];
    top2_scan(m.best, m.second, m.idx, o.best, o.idx, l2);
    if (beats(o.second, m.second, l2)) m.second = o.second;
  }
  write_match(sift1 + p1, sift2, n2, m.best, m.second, m.idx, l2);
}

// ---- the same matcher over a pair list (cusift_match_batch) -----------------------------------------------------------
// points[n_images][max_pts] + counters[n_images] as cusift_extract_batch leaves them; pairs[p] = (frame 1, frame 2).
// A workgroup is (row block, column split, pair): blockIdx.z picks the pair, the two record counts come from device
// memory (clamped to max_pts like rgbd_lift_kernel's), and a workgroup without rows or without columns returns before
// it loads a record.  The grid is sized from max_pts because the host does not know the counts.  Results go to
// rows[pair][max_pts] (score, ambiguity, match: write_match's arithmetic), never into the records, so that a frame can
// be the first member of any number of pairs.  Rows past frame 1's count are not written; a pair whose frame 2 is empty
// writes no row at all.
__device__ __forceinline__ void write_match_row(cusift_match_row *__restrict__ row, float best, float second, int idx,
                                                bool l2) {
  f4 v;
  v[0] = best;
  v[1] = match_ambiguity(best, second, l2);
  v[2] = __int_as_float(idx);
  v[3] = 0.0f;  // reserved
  *reinterpret_cast<f4 *>(row) = v;
}

// partials[pair][split][n1_pad]; NULL with one split: the rows are final
template <bool kL2>
__global__ void __launch_bounds__(256) match_batch_kernel(const cusift_point *__restrict__ points,
                                                         const unsigned int *__restrict__ counters, int max_pts,
                                                         const int *__restrict__ pairs, int cols_per_split,
                                                         MatchPartial *__restrict__ partials, int n1_pad,
                                                         cusift_match_row *__restrict__ rows) {
  __shared__ float sB[kMatchTileCols * kBStride];
  const int pair = blockIdx.z;
  const int f1 = pairs[2 * pair], f2 = pairs[2 * pair + 1];
  const int n1 = frame_count(counters, f1, max_pts), n2 = frame_count(counters, f2, max_pts);
  const int col_begin = blockIdx.y * cols_per_split;
  if ((int)blockIdx.x * kMatchRowsPerBlock >= n1 || col_begin >= n2) return;  // uniform: no rows or no columns
  const cusift_point *__restrict__ sift1 = points + (size_t)f1 * max_pts;
  const cusift_point *__restrict__ sift2 = points + (size_t)f2 * max_pts;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int p1_base = blockIdx.x * kMatchRowsPerBlock + wv * 16;
  const int col_end = min(col_begin + cols_per_split, n2);
  constexpr float kInit = kL2 ? kMatchFltMax : -1.0f;

#include "match_tile.inc"
  if (r == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p1 = p1_base + 4 * g + q;
      if (p1 >= n1) continue;
      if (partials) {
        MatchPartial mp;
        mp.best = best[q];
        mp.second = second[q];
        mp.idx = bidx[q];
        partials[((size_t)pair * gridDim.y + blockIdx.y) * n1_pad + p1] = mp;
      } else {
        write_match_row(rows + (size_t)pair * max_pts + p1, best[q], second[q], bidx[q], kL2);
      }
    }
  }
}

template __global__ void match_batch_kernel<false>(const cusift_point *, const unsigned int *, int, const int *, int,
                                                   MatchPartial *, int, cusift_match_row *);
template __global__ void match_batch_kernel<true>(const cusift_point *, const unsigned int *, int, const int *, int,
                                                  MatchPartial *, int, cusift_match_row *);

// match_merge_kernel per pair (blockIdx.y): folds the splits that had columns, in column order.
__global__ void __launch_bounds__(256) match_batch_merge_kernel(const unsigned int *__restrict__ counters, int max_pts,
                                                               const int *__restrict__ pairs, int l2_mode,
                                                               int cols_per_split,
                                                               const MatchPartial *__restrict__ partials, int n1_pad,
                                                               int n_splits, cusift_match_row *__restrict__ rows) {
  const bool l2 = l2_mode != 0;
  const int pair = blockIdx.y;
  const int n1 = frame_count(counters, pairs[2 * pair], max_pts), n2 = frame_count(counters, pairs[2 * pair + 1], max_pts);
  const int p1 = blockIdx.x * 256 + threadIdx.x;
  if (p1 >= n1 || n2 <= 0) return;
  const int live = min(n_splits, (n2 + cols_per_split - 1) / cols_per_split);  // the others wrote nothing
  const MatchPartial *__restrict__ mine = partials + (size_t)pair * n_splits * n1_pad + p1;
  MatchPartial m = mine[0];
  for (int s = 1; s < live; ++s) {
    const MatchPartial o = mine[(size_t)s * n1_pad];
    top2_scan(m.best, m.second, m.idx, o.best, o.idx, l2);
    if (beats(o.second, m.second, l2)) m.second = o.second;
  }
  write_match_row(rows + (size_t)pair * max_pts + p1, m.best, m.second, m.idx, l2);
}

}  // namespace cusift
