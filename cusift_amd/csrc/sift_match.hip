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

// The column side of a tile as match_tile.inc sees it: tile() once a tile's scores are in the accumulators, drain() for
// the previous tile behind the next tile's barriers, finish() behind the loop.  NoColumnSide is the one-directional
// kernels': every call is an empty inline function.  ColumnSide (cusift_match_mutual) is defined with its kernels below.
struct NoColumnSide {
  template <class... A>
  __device__ __forceinline__ void tile(A...) const {}
  template <class... A>
  __device__ __forceinline__ void drain(A...) const {}
  template <class... A>
  __device__ __forceinline__ void finish(A...) const {}
};

// The geometric predicate of a tile as match_tile.inc sees it: rows() before the column loop, fetch() / store() beside
// the descriptors' staging, column() and pass() in the update.  NoGuide is every unguided kernel's: empty inline
// functions and a test that is always true.  GuideH / GuideF (cusift_match_guided) are defined with their kernels below.
struct NoGuide {
  struct Column {};
  template <class... A>
  __device__ __forceinline__ void rows(A...) const {}
  template <class... A>
  __device__ __forceinline__ void fetch(A...) const {}
  template <class... A>
  __device__ __forceinline__ void store(A...) const {}
  template <class... A>
  __device__ __forceinline__ Column column(A...) const {
    return Column{};
  }
  __device__ __forceinline__ bool pass(int, Column) const { return true; }
};

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
  const NoColumnSide cols;
  const NoGuide guide;

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
  const NoColumnSide cols;
  const NoGuide guide;

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

// ---- both directions from one pass (cusift_match_mutual, cusift_match_batch_mutual) -----------------------------------
// The row side is match_kernel's, from the same text.  The column side -- for every descriptor of image 2 the best and
// second best of image 1 -- is reduced from the same accumulators (match_tile.inc's `cols`) and is defined by
// a plain model: top2_scan over the rows 0 .. n1 - 1 in ascending order from (kInit, kInit, -1).  Best and second of that
// scan do not depend on the order in which partial scans are merged, the index does: every merge takes the lower rows
// first and compares strictly, so an exactly tied best keeps the LOWEST row, whatever the grid.  Column splits
// (blockIdx.y) partition the columns; row blocks (blockIdx.x) each see every column of their split, so with more than
// one row block a column's triple goes to col_partials[row block][column] and match_mutual_merge_kernel folds the row
// blocks in ascending order.  No atomics: the same input gives the same bytes on every run.
//
// Per tile a wave folds its 16 rows of every column -- in the lane over q, then the 16-lane groups g + 1 and g + 2 into g
// -- and leaves 32 triples in LDS (two buffers, by tile parity); behind the next tile's barriers eight lanes of every
// wave fold the four waves of a column and hand it to `out`.  A buffer is written again two tiles later, behind a
// barrier that every wave reaches only after its drain.
typedef float ColFloats[4][kMatchTileCols];  // [wave][column of the tile]
typedef int ColInts[4][kMatchTileCols];

template <bool kL2, class Out>
struct ColumnSide {
  ColFloats *best, *second;  // [2]: tile parity
  ColInts *idx;
  int n1;
  Out out;  // out(column, best, second, idx): the column's result over this workgroup's 64 rows
  static constexpr float kInit = kL2 ? kMatchFltMax : -1.0f;

  __device__ __forceinline__ void tile(int c0, int col_begin, const f32x4 &acc0, const f32x4 &acc1, int p1_base, int lane,
                                       int wv) const {
    const int r = lane & 15, g = lane >> 4;
    const int par = ((c0 - col_begin) / kMatchTileCols) & 1;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float cb = kInit, cs = kInit;
      int ci = -1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {  // rows 4g .. 4g + 3 in ascending order: the model's scan
        const int p1 = p1_base + 4 * g + q;
        const float dot = t ? acc1[q] : acc0[q];
        float val = kL2 ? (dot > -1.0f ? __builtin_fmaf(-2.0f, dot, 2.0f) : kMatchFltMax) : dot;
        val = p1 < n1 ? val : kInit;  // a padding row is a copy of the last descriptor: it changes nothing
        top2_update<kL2>(cb, cs, ci, val, p1);
      }
      // group g takes g + 1, then g + 2 (their rows lie above): lanes 0..15 end with the wave's 16 rows
#pragma unroll
      for (int d = 16; d <= 32; d <<= 1) {
        const float ob = __shfl_down(cb, d);
        const float os = __shfl_down(cs, d);
        const int oi = __shfl_down(ci, d);
        top2_scan(cb, cs, ci, ob, oi, kL2);
        if (beats(os, cs, kL2)) cs = os;
      }
      if (g == 0) {
        best[par][wv][16 * t + r] = cb;
        second[par][wv][16 * t + r] = cs;
        idx[par][wv][16 * t + r] = ci;
      }
    }
  }

  // the columns of the tile at c_prev: lane j < 8 of wave wv folds the four waves of column 8 wv + j, lower rows first
  __device__ __forceinline__ void drain(int c_prev, int col_begin, int col_end, int lane, int wv) const {
    const int j = 8 * wv + lane, col = c_prev + j;
    if (lane < 8 && col < col_end) {
      const int par = ((c_prev - col_begin) / kMatchTileCols) & 1;
      float cb = best[par][0][j], cs = second[par][0][j];
      int ci = idx[par][0][j];
#pragma unroll
      for (int w = 1; w < 4; ++w) {
        top2_scan(cb, cs, ci, best[par][w][j], idx[par][w][j], kL2);
        const float os = second[par][w][j];
        if (beats(os, cs, kL2)) cs = os;
      }
      out(col, cb, cs, ci);
    }
  }

  // the last tile's columns (a split always has columns where this is reached with col_begin < col_end)
  __device__ __forceinline__ void finish(int col_begin, int col_end, int lane, int wv) const {
    if (col_begin >= col_end) return;
    __syncthreads();
    drain(col_begin + (col_end - col_begin - 1) / kMatchTileCols * kMatchTileCols, col_begin, col_end, lane, wv);
  }
};

template <bool kL2>
__global__ void __launch_bounds__(256) match_mutual_kernel(cusift_point *sift1, int n1, cusift_point *sift2, int n2,
                                                          int cols_per_split, MatchPartial *__restrict__ partials,
                                                          int n1_pad, MatchPartial *__restrict__ col_partials) {
  __shared__ float sB[kMatchTileCols * kBStride];
  __shared__ ColFloats sColBest[2], sColSecond[2];
  __shared__ ColInts sColIdx[2];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int p1_base = blockIdx.x * kMatchRowsPerBlock + wv * 16;
  const int col_begin = blockIdx.y * cols_per_split;
  const int col_end = min(col_begin + cols_per_split, n2);
  constexpr float kInit = kL2 ? kMatchFltMax : -1.0f;
  auto col_out = [&](int col, float cb, float cs, int ci) {
    if (col_partials) {
      MatchPartial mp;
      mp.best = cb;
      mp.second = cs;
      mp.idx = ci;
      col_partials[(size_t)blockIdx.x * n2 + col] = mp;
    } else {
      write_match(sift2 + col, sift1, n1, cb, cs, ci, kL2);
    }
  };
  const ColumnSide<kL2, decltype(col_out)> cols{sColBest, sColSecond, sColIdx, n1, col_out};
  const NoGuide guide;

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

template __global__ void match_mutual_kernel<false>(cusift_point *, int, cusift_point *, int, int, MatchPartial *, int,
                                                    MatchPartial *);
template __global__ void match_mutual_kernel<true>(cusift_point *, int, cusift_point *, int, int, MatchPartial *, int,
                                                   MatchPartial *);

// The twin of match_merge_kernel for the column side: folds the row blocks of one column in ascending row order.
__global__ void __launch_bounds__(256) match_mutual_merge_kernel(cusift_point *sift2, int n2, const cusift_point *sift1,
                                                                int n1, int l2_mode,
                                                                const MatchPartial *__restrict__ col_partials,
                                                                int row_blocks) {
  const bool l2 = l2_mode != 0;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n2) return;
  MatchPartial m = col_partials[j];
  for (int b = 1; b < row_blocks; ++b) {
    const MatchPartial o = col_partials[(size_t)b * n2 + j];
    top2_scan(m.best, m.second, m.idx, o.best, o.idx, l2);
    if (beats(o.second, m.second, l2)) m.second = o.second;
  }
  write_match(sift2 + j, sift1, n1, m.best, m.second, m.idx, l2);
}

// match_batch_kernel with the column side: rows_back[pair][max_pts] receives, for record j of frame 2, what the model
// above gives over the records of frame 1.  col_partials[pair][row block][max_pts]; NULL when max_pts fits one row block.
template <bool kL2>
__global__ void __launch_bounds__(256) match_batch_mutual_kernel(const cusift_point *__restrict__ points,
                                                                const unsigned int *__restrict__ counters,
                                                                int max_pts, const int *__restrict__ pairs,
                                                                int cols_per_split, MatchPartial *__restrict__ partials,
                                                                int n1_pad, cusift_match_row *__restrict__ rows,
                                                                MatchPartial *__restrict__ col_partials,
                                                                cusift_match_row *__restrict__ rows_back) {
  __shared__ float sB[kMatchTileCols * kBStride];
  __shared__ ColFloats sColBest[2], sColSecond[2];
  __shared__ ColInts sColIdx[2];
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
  auto col_out = [&](int col, float cb, float cs, int ci) {
    if (col_partials) {
      MatchPartial mp;
      mp.best = cb;
      mp.second = cs;
      mp.idx = ci;
      col_partials[((size_t)pair * gridDim.x + blockIdx.x) * max_pts + col] = mp;
    } else {
      write_match_row(rows_back + (size_t)pair * max_pts + col, cb, cs, ci, kL2);
    }
  };
  const ColumnSide<kL2, decltype(col_out)> cols{sColBest, sColSecond, sColIdx, n1, col_out};
  const NoGuide guide;

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

template __global__ void match_batch_mutual_kernel<false>(const cusift_point *, const unsigned int *, int, const int *,
                                                          int, MatchPartial *, int, cusift_match_row *, MatchPartial *,
                                                          cusift_match_row *);
template __global__ void match_batch_mutual_kernel<true>(const cusift_point *, const unsigned int *, int, const int *,
                                                         int, MatchPartial *, int, cusift_match_row *, MatchPartial *,
                                                         cusift_match_row *);

// match_mutual_merge_kernel per pair (blockIdx.y): folds the row blocks that had rows, in ascending order.
__global__ void __launch_bounds__(256) match_batch_mutual_merge_kernel(const unsigned int *__restrict__ counters,
                                                                      int max_pts, const int *__restrict__ pairs,
                                                                      int l2_mode,
                                                                      const MatchPartial *__restrict__ col_partials,
                                                                      int row_blocks,
                                                                      cusift_match_row *__restrict__ rows_back) {
  const bool l2 = l2_mode != 0;
  const int pair = blockIdx.y;
  const int n1 = frame_count(counters, pairs[2 * pair], max_pts), n2 = frame_count(counters, pairs[2 * pair + 1], max_pts);
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n2 || n1 <= 0) return;
  const int live = min(row_blocks, (n1 + kMatchRowsPerBlock - 1) / kMatchRowsPerBlock);  // the others wrote nothing
  const MatchPartial *__restrict__ mine = col_partials + (size_t)pair * row_blocks * max_pts + j;
  MatchPartial m = mine[0];
  for (int b = 1; b < live; ++b) {
    const MatchPartial o = mine[(size_t)b * max_pts];
    top2_scan(m.best, m.second, m.idx, o.best, o.idx, l2);
    if (beats(o.second, m.second, l2)) m.second = o.second;
  }
  write_match_row(rows_back + (size_t)pair * max_pts + j, m.best, m.second, m.idx, l2);
}

// ---- nearest neighbours under a known H or F (cusift_match_guided, cusift_match_batch_guided) ------------------------
// match_kernel with one more rule: a column whose coords2D fail the geometric test against the row's coords2D scores
// kInit for that row, which changes nothing in the scan.  The definition, expression by expression, is in
// include/cusift_amd_extras.h; per row it is fp64 and evaluated once, before the column loop -- lane (r, g) computes row
// 4g + (r & 3) of its wave and the four lanes of a quad exchange, so every lane ends with the terms of its rows 4g + q in
// registers -- and per (row, column) it is a handful of fp32 operations in the update, beside the MFMAs of the other
// waves.  The columns' coordinates ride in the four spare floats of the LDS rows (kBStride 132, 128 used): the first 32
// threads load them through the descriptors' buffer resource, so a column past col_end reads (0, 0) -- and is still
// masked by `live`, because (0, 0) can pass.
struct GuideColumns {
  struct Column {
    float x, y;
  };
  const double *m;  // the model, row-major
  float r2;         // radius * radius
  u2 staged;        // threads 0..31: coords2D of column c0 + threadIdx.x of the tile in flight

  __device__ __forceinline__ void fetch(__amdgpu_buffer_rsrc_t rsrc2, int soff) {
    if (threadIdx.x < kMatchTileCols)
      staged = __builtin_amdgcn_raw_buffer_load_b64(
          rsrc2, (int)threadIdx.x * (int)sizeof(cusift_point) + (int)offsetof(cusift_point, coords2D), soff, 0);
  }
  __device__ __forceinline__ void store(float *sB) const {
    if (threadIdx.x < kMatchTileCols) *reinterpret_cast<u2 *>(sB + threadIdx.x * kBStride + 128) = staged;
  }
  __device__ __forceinline__ Column column(const float *sB, int j) const {
    const f2 v = *reinterpret_cast<const f2 *>(sB + j * kBStride + 128);
    return Column{v[0], v[1]};
  }
  // coords2D of the row this lane evaluates, and what the quad's lane q evaluated
  __device__ __forceinline__ const float *row_xy(const cusift_point *__restrict__ sift1, int n1, int p1_base,
                                                 int lane) const {
    return sift1[min(p1_base + 4 * (lane >> 4) + (lane & 3), n1 - 1)].coords2D;
  }
  static __device__ __forceinline__ float from_quad(float v, int lane, int q) { return __shfl(v, (lane & ~3) | q); }
};

// x2 ~ H x1: the row's image (px, py), then |x2 - p|^2 < r2.  W == 0 gives an infinity or a NaN: no pass.
struct GuideH : GuideColumns {
  float px[4], py[4];
  __device__ __forceinline__ void rows(const cusift_point *__restrict__ sift1, int n1, int p1_base, int lane) {
    const float *xy = row_xy(sift1, n1, p1_base, lane);
    const double x1 = xy[0], y1 = xy[1];
    const double X = (m[0] * x1 + m[1] * y1) + m[2];
    const double Y = (m[3] * x1 + m[4] * y1) + m[5];
    const double W = (m[6] * x1 + m[7] * y1) + m[8];
    const float x = (float)(X / W), y = (float)(Y / W);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      px[q] = from_quad(x, lane, q);
      py[q] = from_quad(y, lane, q);
    }
  }
  __device__ __forceinline__ bool pass(int q, Column c) const {
    const float dx = c.x - px[q], dy = c.y - py[q];
    return dx * dx + dy * dy < r2;
  }
};

// x2^T F x1 = 0: the row's epipolar line scaled to a unit normal (a, b, c), then (a x2 + b y2 + c)^2 < r2.  A line whose
// normal has length 0 or that is not finite is three NaNs: no pass for the whole row.
struct GuideF : GuideColumns {
  float a[4], b[4], c[4];
  __device__ __forceinline__ void rows(const cusift_point *__restrict__ sift1, int n1, int p1_base, int lane) {
    const float *xy = row_xy(sift1, n1, p1_base, lane);
    const double x1 = xy[0], y1 = xy[1];
    const double l0 = (m[0] * x1 + m[1] * y1) + m[2];
    const double l1 = (m[3] * x1 + m[4] * y1) + m[5];
    const double l2 = (m[6] * x1 + m[7] * y1) + m[8];
    const double n = sqrt(l0 * l0 + l1 * l1);
    const double kInf = __builtin_huge_val();
    const bool line = n > 0.0 && n < kInf && fabs(l2) < kInf;
    const float kNaN = __builtin_nanf("");
    const float la = line ? (float)(l0 / n) : kNaN, lb = line ? (float)(l1 / n) : kNaN, lc = line ? (float)(l2 / n) : kNaN;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      a[q] = from_quad(la, lane, q);
      b[q] = from_quad(lb, lane, q);
      c[q] = from_quad(lc, lane, q);
    }
  }
  __device__ __forceinline__ bool pass(int q, Column p) const {
    const float d = (a[q] * p.x + b[q] * p.y) + c[q];
    return d * d < r2;
  }
};

template <bool kL2, class Guide>
__global__ void __launch_bounds__(256) match_guided_kernel(cusift_point *__restrict__ sift1, int n1,
                                                          const cusift_point *__restrict__ sift2, int n2,
                                                          int cols_per_split, MatchPartial *__restrict__ partials,
                                                          int n1_pad, GuideModel model, float r2) {
  __shared__ float sB[kMatchTileCols * kBStride];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int p1_base = blockIdx.x * kMatchRowsPerBlock + wv * 16;
  const int col_begin = blockIdx.y * cols_per_split;
  const int col_end = min(col_begin + cols_per_split, n2);
  constexpr float kInit = kL2 ? kMatchFltMax : -1.0f;
  const NoColumnSide cols;
  Guide guide;
  guide.m = model.m;
  guide.r2 = r2;

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

// match_batch_kernel with pair blockIdx.z's model from models[pair] (a device copy of the caller's array)
template <bool kL2, class Guide>
__global__ void __launch_bounds__(256) match_batch_guided_kernel(const cusift_point *__restrict__ points,
                                                                const unsigned int *__restrict__ counters,
                                                                int max_pts, const int *__restrict__ pairs,
                                                                int cols_per_split, MatchPartial *__restrict__ partials,
                                                                int n1_pad, cusift_match_row *__restrict__ rows,
                                                                const GuideModel *__restrict__ models, float r2) {
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
  const NoColumnSide cols;
  Guide guide;
  guide.m = models[pair].m;
  guide.r2 = r2;

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

#define CUSIFT_GUIDED_KERNELS(kL2, Guide)                                                                               \
  template __global__ void match_guided_kernel<kL2, Guide>(cusift_point *, int, const cusift_point *, int, int,          \
                                                           MatchPartial *, int, GuideModel, float);                      \
  template __global__ void match_batch_guided_kernel<kL2, Guide>(const cusift_point *, const unsigned int *, int,        \
                                                                 const int *, int, MatchPartial *, int,                  \
                                                                 cusift_match_row *, const GuideModel *, float);
CUSIFT_GUIDED_KERNELS(false, GuideH)
CUSIFT_GUIDED_KERNELS(true, GuideH)
CUSIFT_GUIDED_KERNELS(false, GuideF)
CUSIFT_GUIDED_KERNELS(true, GuideF)
#undef CUSIFT_GUIDED_KERNELS

}  // namespace cusift
