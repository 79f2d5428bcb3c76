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
//
// Every main kernel is match_block (sift_match_block.h, shared with sift_match_project.hip) between its frame and its
// sinks: one text, so that a (row, column) dot product is the same chain whichever kernel computes it.  The write-out, the
// pair-list frame, the fold of the merge kernels and the "partial or final" sink are sift_match_common.h's, shared with
// the 8-bit matcher.
#include "sift_match_block.h"

namespace cusift {

struct Top2Merge {  // as fold_partials' merge step
  bool l2;
  __device__ __forceinline__ void operator()(MatchPartial &m, const MatchPartial &o) const {
    top2_merge(m.best, m.second, m.idx, o.best, o.second, o.idx, l2);
  }
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
  const int col_begin = blockIdx.y * cols_per_split;
  match_block<kL2>(sift1, n1, sift2, col_begin, min(col_begin + cols_per_split, n2), sB, NoColumnSide{}, NoGuide{},
                   point_sink<kL2>(partials, (size_t)blockIdx.y * n1_pad, sift1, sift2, n2));
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
  const MatchPartial m = fold_partials(partials + p1, n1_pad, n_splits, Top2Merge{l2});
  write_match(sift1 + p1, sift2, n2, m.best, m.second, m.idx, l2);
}

// ---- the same matcher over a pair list (cusift_match_batch) -----------------------------------------------------------
// A workgroup is (row block, column split, pair) of PairFrame (sift_match_common.h); one without rows or without columns
// returns before it loads a record.  Results go to rows[pair][max_pts], never into the records.  Rows past frame 1's
// count are not written; a pair whose frame 2 is empty writes no row at all.
// partials[pair][split][n1_pad]; NULL with one split: the rows are final
template <bool kL2>
__global__ void __launch_bounds__(256) match_batch_kernel(const cusift_point *__restrict__ points,
                                                         const unsigned int *__restrict__ counters, int max_pts,
                                                         const int *__restrict__ pairs, int cols_per_split,
                                                         MatchPartial *__restrict__ partials, int n1_pad,
                                                         cusift_match_row *__restrict__ rows) {
  __shared__ float sB[kMatchTileCols * kBStride];
  const PairFrame fr(counters, pairs, max_pts, cols_per_split, kMatchRowsPerBlock);
  if (fr.empty) return;
  match_block<kL2>(points + (size_t)fr.f1 * max_pts, fr.n1, points + (size_t)fr.f2 * max_pts, fr.col_begin, fr.col_end,
                   sB, NoColumnSide{}, NoGuide{},
                   row_sink<kL2>(partials, ((size_t)fr.pair * gridDim.y + blockIdx.y) * n1_pad,
                                 rows + (size_t)fr.pair * max_pts));
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
  const PairCounts pc(blockIdx.y, counters, pairs, max_pts);
  const int p1 = blockIdx.x * 256 + threadIdx.x;
  if (p1 >= pc.n1 || pc.n2 <= 0) return;
  const int live = min(n_splits, (pc.n2 + cols_per_split - 1) / cols_per_split);  // the others wrote nothing
  const MatchPartial m =
      fold_partials(partials + (size_t)pc.pair * n_splits * n1_pad + p1, n1_pad, live, Top2Merge{l2});
  write_match_row(rows + (size_t)pc.pair * max_pts + p1, m.best, m.second, m.idx, l2);
}

// ---- both directions from one pass (cusift_match_mutual, cusift_match_batch_mutual) -----------------------------------
// The row side is match_kernel's, from the same text.  The column side -- for every descriptor of image 2 the best and
// second best of image 1 -- is reduced from the same accumulators (match_block's `cols`) and is defined by
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
struct ColumnTriples {  // [tile parity][wave][column of the tile]
  float best[2][4][kMatchTileCols], second[2][4][kMatchTileCols];
  int idx[2][4][kMatchTileCols];
};

template <bool kL2, class Out>
struct ColumnSide {
  ColumnTriples *s;
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
        top2_merge(cb, cs, ci, ob, os, oi, kL2);
      }
      if (g == 0) {
        s->best[par][wv][16 * t + r] = cb;
        s->second[par][wv][16 * t + r] = cs;
        s->idx[par][wv][16 * t + r] = ci;
      }
    }
  }

  // the columns of the tile at c_prev: lane j < 8 of wave wv folds the four waves of column 8 wv + j, lower rows first
  __device__ __forceinline__ void drain(int c_prev, int col_begin, int col_end, int lane, int wv) const {
    const int j = 8 * wv + lane, col = c_prev + j;
    if (lane < 8 && col < col_end) {
      const int par = ((c_prev - col_begin) / kMatchTileCols) & 1;
      float cb = s->best[par][0][j], cs = s->second[par][0][j];
      int ci = s->idx[par][0][j];
#pragma unroll
      for (int w = 1; w < 4; ++w) top2_merge(cb, cs, ci, s->best[par][w][j], s->second[par][w][j], s->idx[par][w][j], kL2);
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
template <bool kL2, class Out>
__device__ __forceinline__ ColumnSide<kL2, Out> column_side(ColumnTriples *s, int n1, Out out) {
  return ColumnSide<kL2, Out>{s, n1, out};
}

template <bool kL2>
__global__ void __launch_bounds__(256) match_mutual_kernel(cusift_point *sift1, int n1, cusift_point *sift2, int n2,
                                                          int cols_per_split, MatchPartial *__restrict__ partials,
                                                          int n1_pad, MatchPartial *__restrict__ col_partials) {
  __shared__ float sB[kMatchTileCols * kBStride];
  __shared__ ColumnTriples sCols;
  const int col_begin = blockIdx.y * cols_per_split;
  match_block<kL2>(
      sift1, n1, sift2, col_begin, min(col_begin + cols_per_split, n2), sB,
      column_side<kL2>(&sCols, n1, point_sink<kL2>(col_partials, (size_t)blockIdx.x * n2, sift2, sift1, n1)), NoGuide{},
      point_sink<kL2>(partials, (size_t)blockIdx.y * n1_pad, sift1, sift2, n2));
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
  const MatchPartial m = fold_partials(col_partials + j, n2, row_blocks, Top2Merge{l2});
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
  __shared__ ColumnTriples sCols;
  const PairFrame fr(counters, pairs, max_pts, cols_per_split, kMatchRowsPerBlock);
  if (fr.empty) return;
  match_block<kL2>(
      points + (size_t)fr.f1 * max_pts, fr.n1, points + (size_t)fr.f2 * max_pts, fr.col_begin, fr.col_end, sB,
      column_side<kL2>(&sCols, fr.n1,
                       row_sink<kL2>(col_partials, ((size_t)fr.pair * gridDim.x + blockIdx.x) * max_pts,
                                     rows_back + (size_t)fr.pair * max_pts)),
      NoGuide{},
      row_sink<kL2>(partials, ((size_t)fr.pair * gridDim.y + blockIdx.y) * n1_pad, rows + (size_t)fr.pair * max_pts));
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
  const PairCounts pc(blockIdx.y, counters, pairs, max_pts);
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= pc.n2 || pc.n1 <= 0) return;
  const int live = min(row_blocks, (pc.n1 + kMatchRowsPerBlock - 1) / kMatchRowsPerBlock);  // the others wrote nothing
  const MatchPartial m =
      fold_partials(col_partials + (size_t)pc.pair * row_blocks * max_pts + j, max_pts, live, Top2Merge{l2});
  write_match_row(rows_back + (size_t)pc.pair * max_pts + j, m.best, m.second, m.idx, l2);
}

// ---- nearest neighbours under a known H or F (cusift_match_guided, cusift_match_batch_guided) ------------------------
// match_kernel with one more rule: a column whose coords2D fail the geometric test against the row's coords2D scores
// kInit for that row, which changes nothing in the scan.  The definition, expression by expression, is in
// include/cusift_amd_extras.h; per row it is fp64 and evaluated once, before the column loop -- lane (r, g) computes row
// 4g + (r & 3) of its wave and the four lanes of a quad exchange, so every lane ends with the terms of its rows 4g + q in
// registers -- and per (row, column) it is a handful of fp32 operations in the update, beside the MFMAs of the other
// waves.  The columns' staging is GuideColumns (sift_match_block.h).

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
  const int col_begin = blockIdx.y * cols_per_split;
  Guide guide;
  guide.m = model.m;
  guide.r2 = r2;
  match_block<kL2>(sift1, n1, sift2, col_begin, min(col_begin + cols_per_split, n2), sB, NoColumnSide{}, guide,
                   point_sink<kL2>(partials, (size_t)blockIdx.y * n1_pad, sift1, sift2, n2));
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
  const PairFrame fr(counters, pairs, max_pts, cols_per_split, kMatchRowsPerBlock);
  if (fr.empty) return;
  Guide guide;
  guide.m = models[fr.pair].m;
  guide.r2 = r2;
  match_block<kL2>(points + (size_t)fr.f1 * max_pts, fr.n1, points + (size_t)fr.f2 * max_pts, fr.col_begin, fr.col_end,
                   sB, NoColumnSide{}, guide,
                   row_sink<kL2>(partials, ((size_t)fr.pair * gridDim.y + blockIdx.y) * n1_pad,
                                 rows + (size_t)fr.pair * max_pts));
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
