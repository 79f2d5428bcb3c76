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
// Every main kernel is match_block (below) between its frame and its sinks: one text, so that a (row, column) dot
// product is the same chain whichever kernel computes it.  The write-out, the pair-list frame, the fold of the merge
// kernels and the "partial or final" sink are sift_match_common.h's, shared with the 8-bit matcher.
#include "sift_match_common.h"

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

// The triple (ob, os, oi) of the columns (or rows) that lie above this triple's, merged into it: the step of the tree
// over the lanes and of every fold over splits, waves and row blocks.  The comparisons are strict, so an exactly tied
// best keeps the lower index.
__device__ __forceinline__ void top2_merge(float &best, float &second, int &idx, float ob, float os, int oi, bool l2) {
  top2_scan(best, second, idx, ob, oi, l2);
  if (beats(os, second, l2)) second = os;
}
struct Top2Merge {  // as fold_partials' merge step
  bool l2;
  __device__ __forceinline__ void operator()(MatchPartial &m, const MatchPartial &o) const {
    top2_merge(m.best, m.second, m.idx, o.best, o.second, o.idx, l2);
  }
};

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

// The two sinks of the main kernels (partial_or, sift_match_common.h): the triple of record i of `dst` against the
// records `other`, and of row i of a pair's row array.
template <bool kL2>
__device__ __forceinline__ auto point_sink(MatchPartial *partials, size_t slab, cusift_point *dst,
                                           const cusift_point *other, int n_other) {
  return partial_or(partials, slab,
                    [=](int i, float b, float s, int idx) { write_match(dst + i, other, n_other, b, s, idx, kL2); });
}
template <bool kL2>
__device__ __forceinline__ auto row_sink(MatchPartial *partials, size_t slab, cusift_match_row *rows) {
  return partial_or(partials, slab, [=](int i, float b, float s, int idx) { write_match_row(rows + i, b, s, idx, kL2); });
}

// The column side of a tile as match_block sees it: tile() once a tile's scores are in the accumulators, drain() for
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

// The geometric predicate of a tile as match_block sees it: rows() before the column loop, fetch() / store() beside
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

// One workgroup's 64 rows [blockIdx.x * 64 ..) of (sift1, n1) -- descriptors p1_base .. p1_base + 15 in each wave --
// against the columns [col_begin, col_end) of sift2, through the LDS tile sB.  out(row, best, second, idx) receives every
// row < n1 once.
// `cols` is the column side: NoColumnSide in the one-directional kernels, whose three calls below are empty inline
// functions -- no barrier, no LDS, no register (tools/kernel_regs.py: 96 VGPRs, 16,896 B); ColumnSide in the mutual
// kernels.
// `guide` is the geometric predicate of the guided kernels: NoGuide everywhere else, again nothing but empty inline
// functions; GuideH / GuideF keep the per-row terms of this lane's rows 4g + q in registers (rows()), stage coords2D of
// a tile's 32 columns into floats 128..129 of the columns' LDS rows (fetch() / store(), the descriptors' range-checked
// buffer resource, no new LDS) and turn a (row, column) that fails the test into kInit in the update.
template <bool kL2, class Cols, class Guide, class Out>
__device__ __forceinline__ void match_block(const cusift_point *sift1, int n1, const cusift_point *sift2, int col_begin,
                                            int col_end, float *sB, const Cols cols, Guide guide, const Out out) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int p1_base = blockIdx.x * kMatchRowsPerBlock + wv * 16;
  constexpr float kInit = kL2 ? kMatchFltMax : -1.0f;  // also what a masked column scores: it changes nothing

  // A fragments: lane (r, g) holds elements 16u + 4g + j of descriptor p1_base + r (u = 0..7, j = 0..3)
  float a[8][4];
  {
    const float *d1 = sift1[min(p1_base + r, n1 - 1)].data;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const f4u v = *reinterpret_cast<const f4u *>(d1 + 16 * u + 4 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[u][j] = v[j];
    }
  }
  // running top-2 of rows 4g + q for the columns this lane sees (p2 = r mod 16): reference thread tx = r
  float best[4], second[4];
  int bidx[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    best[q] = second[q] = kInit;
    bidx[q] = -1;
  }
  guide.rows(sift1, n1, p1_base, lane);

  // staging: thread t moves four 16-byte chunks per tile; chunk c = t + 256 i -> descriptor c >> 5, floats 4 (c & 31).
  // Raw buffer loads from a descriptor based at this split's first column: the lane offset is computed once, the tile
  // and the chunk row advance in the scalar offset, and columns past col_end read as 0 (their scores are masked below;
  // padded columns, extras/matching.cu:57, can never win: they are skipped).
  const __amdgpu_buffer_rsrc_t rsrc2 = __builtin_amdgcn_make_buffer_rsrc(
      (void *)(sift2 + col_begin), 0, (int)((col_end > col_begin ? col_end - col_begin : 0) * sizeof(cusift_point)),
      kBufFlags);
  constexpr int kRec = (int)sizeof(cusift_point);
  const int voff = (int)(threadIdx.x >> 5) * kRec + (int)offsetof(cusift_point, data) + 16 * (int)(threadIdx.x & 31);
  u4 stage[4];
  auto fetch = [&](int c0) {
    const int soff = __builtin_amdgcn_readfirstlane((c0 - col_begin) * kRec);
#pragma unroll
    for (int i = 0; i < 4; ++i) stage[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc2, voff, soff + 8 * i * kRec, 0);
    guide.fetch(rsrc2, soff);
  };
  if (col_begin < col_end) fetch(col_begin);
  const float *brow = sB + r * kBStride + 4 * g;
  for (int c0 = col_begin; c0 < col_end; c0 += kMatchTileCols) {
    __syncthreads();  // the previous tile has been consumed
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = threadIdx.x + 256 * i;
      *reinterpret_cast<u4 *>(sB + (c >> 5) * kBStride + 4 * (c & 31)) = stage[i];
    }
    guide.store(sB);
    __syncthreads();
    if (c0 + kMatchTileCols < col_end) fetch(c0 + kMatchTileCols);  // in flight while this tile is multiplied
    if (c0 > col_begin) cols.drain(c0 - kMatchTileCols, col_begin, col_end, lane, wv);  // the previous tile's columns
    // this lane's two columns' coordinates, read in front of the MFMAs so that the update does not wait for LDS
    const auto xy2a = guide.column(sB, r), xy2b = guide.column(sB, 16 + r);

    // two independent 16x16 accumulators (columns c0 + r and c0 + 16 + r), each a k-ordered chain; the B fragments
    // of step u + 1 are read from LDS before the MFMAs of step u are issued
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_s_setprio(1);  // a wave with MFMAs to issue goes before its SIMD's waves that are in the update
    f4 b0 = *reinterpret_cast<const f4 *>(brow);
    f4 b1 = *reinterpret_cast<const f4 *>(brow + 16 * kBStride);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      f4 n0 = b0, n1v = b1;
      if (u < 7) {
        n0 = *reinterpret_cast<const f4 *>(brow + 16 * (u + 1));
        n1v = *reinterpret_cast<const f4 *>(brow + 16 * kBStride + 16 * (u + 1));
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][j], b0[j], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][j], b1[j], acc1, 0, 0, 0);
      }
      b0 = n0;
      b1 = n1v;
    }
    __builtin_amdgcn_s_setprio(0);
    // acc[q] = <descriptor p1_base + 4g + q, descriptor p2>.  (Deferring this update into the next tile's MFMA gaps
    // -- one score per step u -- was built and measured: no change, 110-112 TFLOP/s at 16k either way.)
    {
      const bool full = c0 + kMatchTileCols <= col_end;  // wave-uniform: only a split's last tile can be partial
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int p2 = c0 + 16 * t + r;
        const bool live = full || p2 < col_end;
        const auto xy2 = t ? xy2b : xy2a;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float dot = t ? acc1[q] : acc0[q];
          // ComputeL2Distance :71-72, 2 - 2*dot (2*dot is exact, so the fused form has the same bits)
          float val = kL2 ? (dot > -1.0f ? __builtin_fmaf(-2.0f, dot, 2.0f) : kMatchFltMax) : dot;
          // `live` stays in the condition: a column past col_end reads as zeros, and (0, 0) can pass a guide
          val = (live && guide.pass(q, xy2)) ? val : kInit;
          top2_update<kL2>(best[q], second[q], bidx[q], val, p2);
        }
      }
    }
    cols.tile(c0, col_begin, acc0, acc1, p1_base, lane, wv);
  }
  cols.finish(col_begin, col_end, lane, wv);
  // tree over tx = r (extras/matching.cu:122-138,201-218): lane r < len takes lane r + len; ties keep the lower r
#pragma unroll
  for (int len = 8; len > 0; len >>= 1) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float ob = __shfl_down(best[q], len, 16);
      const float os = __shfl_down(second[q], len, 16);
      const int oi = __shfl_down(bidx[q], len, 16);
      if (r < len) top2_merge(best[q], second[q], bidx[q], ob, os, oi, kL2);
    }
  }
  if (r == 0) {  // lane r == 0 of every 16-lane group g holds rows p1_base + 4 g + q
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int p1 = p1_base + 4 * g + q;
      if (p1 < n1) out(p1, best[q], second[q], bidx[q]);
    }
  }
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
