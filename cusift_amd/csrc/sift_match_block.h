// sift_match_block.h -- the block body of the fp32 matcher and what goes in and out of it, for the units that instantiate
// it: sift_match.hip (plain, mutual, guided by H or F) and sift_match_project.hip (guided by a pose and coords3D).  The
// tile constants, the top-2 update and merge, match_block, the two sinks, the empty column side and the empty guide, and
// the column staging every geometric guide shares (GuideColumns).  Device code only.
#pragma once

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
// kernels': every call is an empty inline function.  ColumnSide (cusift_match_mutual) is defined with its kernels in
// sift_match.hip.
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
// functions and a test that is always true.  GuideH / GuideF (cusift_match_guided) are defined with their kernels in
// sift_match.hip, GuideP (cusift_match_projected) with its kernels in sift_match_project.hip.
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

// What the geometric guides share (GuideH / GuideF in sift_match.hip, GuideP in sift_match_project.hip).  The columns'
// coordinates ride in the four spare floats of the LDS rows (kBStride 132, 128 used): the first 32 threads load them
// through the descriptors' buffer resource, so a column past col_end reads (0, 0) -- and is still masked by `live`,
// because (0, 0) can pass.
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

}  // namespace cusift
