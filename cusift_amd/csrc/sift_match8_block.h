// sift_match8_block.h -- the block body of the int8 matcher and what goes in and out of it, for the units that
// instantiate it: sift_match8.hip (plain, mutual) and sift_match8_guided.hip (guided by H, F or a pose).  The tile
// constants, the partial and its merge, the write-out and the two sinks, the column side, the empty guide and m8_block.
// How the matcher works is told at the head of sift_match8.hip.  Device code only.
#pragma once

#include "sift_match_common.h"

namespace cusift {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kM8RowsPerWave = 64;                    // four 16-row A fragments
constexpr int kM8RowsPerBlock = 4 * kM8RowsPerWave;   // 256
constexpr int kM8TileCols = 64;                       // columns per LDS tile
constexpr int kM8Stride = 144;                        // bytes per LDS column: 128 + the column's term + pad; 36 dwords,
                                                      // = 4 mod 32 like the fp32 matcher's rows: ds_read_b128 without conflicts
constexpr int kM8Masked = 1 << 30;                    // the term of a column past the split's end
constexpr int kM8None = 1 << 29;                      // a key at or above this is no column
constexpr int kM8Init = 0x7fffffff;
constexpr float kM8FltMax = 999.0f;                   // cusift_match's initial values
constexpr float kM8Scale = 1.0f / 262144.0f;          // 2^-18: (q / 512)^2

// per-(column split, row) result: final keys (D, or -S), kM8Init where there is none
struct Match8Partial {
  int best, second, idx, pad;
};

__device__ __forceinline__ int med3i(int a, int b, int c) { return max(min(a, b), min(max(a, b), c)); }

// (best, second, idx) of two disjoint column sets -> of their union: (key, column) pairs in order, second smallest key
__device__ __forceinline__ void m8_merge(int &best, int &second, int &idx, int ob, int os, int oi) {
  const bool take = ob < best || (ob == best && (unsigned)oi < (unsigned)idx);  // idx -1 (no column) loses to any column
  second = min(max(best, ob), min(second, os));
  best = min(best, ob);
  idx = take ? oi : idx;
}
struct M8Merge {  // as fold_partials' merge step
  __device__ __forceinline__ void operator()(Match8Partial &m, const Match8Partial &o) const {
    m8_merge(m.best, m.second, m.idx, o.best, o.second, o.idx);
  }
};

// what a row's term adds behind the scan
template <bool kL2>
__device__ __forceinline__ int m8_row_term(int sum, int sq) {
  return kL2 ? sq - 256 * sum + (1 << 21) : (1 << 21) - 128 * sum;
}
template <bool kL2>
__device__ __forceinline__ int m8_col_term(int sum, int sq) {
  return kL2 ? sq - 256 * sum + (1 << 21) : -128 * sum;
}

// final keys -> the three values cusift_match's tail works on.  kNone (the guided kernels): a row may have no column at
// all -- best is kM8Init -- and then scores cusift_match's initial value too.
template <bool kL2, bool kNone = false>
__device__ __forceinline__ void m8_floats(int best, int second, float &fb, float &fs) {
  fb = kL2 ? (float)best * kM8Scale : (float)(-best) * kM8Scale;
  if constexpr (kNone) fb = best >= kM8None ? (kL2 ? kM8FltMax : -1.0f) : fb;
  fs = second >= kM8None ? (kL2 ? kM8FltMax : -1.0f) : (kL2 ? (float)second * kM8Scale : (float)(-second) * kM8Scale);
}

// cusift_match's tail on them (sift_match_common.h): the five fields of a record, or a row of a pair's row array
template <bool kL2, bool kNone = false>
__device__ __forceinline__ void m8_write_point(cusift_point *pt, const cusift_point *__restrict__ sift2, int n2, int best,
                                               int second, int idx) {
  float fb, fs;
  m8_floats<kL2, kNone>(best, second, fb, fs);
  write_match(pt, sift2, n2, fb, fs, idx, kL2);
}
template <bool kL2, bool kNone = false>
__device__ __forceinline__ void m8_write_row(cusift_match_row *__restrict__ row, int best, int second, int idx) {
  float fb, fs;
  m8_floats<kL2, kNone>(best, second, fb, fs);
  write_match_row(row, fb, fs, idx, kL2);
}

// The two sinks of the main kernels (partial_or, sift_match_common.h): the keys of record i of `dst` against the records
// `other`, and of row i of a pair's row array.
template <bool kL2, bool kNone = false>
__device__ __forceinline__ auto m8_point_sink(Match8Partial *partials, size_t slab, cusift_point *dst,
                                              const cusift_point *other, int n_other) {
  return partial_or(partials, slab, [=](int i, int b, int s, int idx) {
    m8_write_point<kL2, kNone>(dst + i, other, n_other, b, s, idx);
  });
}
template <bool kL2, bool kNone = false>
__device__ __forceinline__ auto m8_row_sink(Match8Partial *partials, size_t slab, cusift_match_row *rows) {
  return partial_or(partials, slab,
                    [=](int i, int b, int s, int idx) { m8_write_row<kL2, kNone>(rows + i, b, s, idx); });
}

// ---- the column side (cusift_match8_mutual, cusift_match8_batch_mutual) -------------------------------------------------
// For every column the best and second best ROW, from the accumulators the row side already holds.  In the C/D layout lane
// (r, g) has, per B fragment, the 16 scores of one column against rows 16 i + 4 g + j of its wave.  The column's order over
// the rows does not depend on the column's own term, so the scan runs on
//     key'' = R - 2 S'   (L2)          key'' = -128 sum q1 - S'   (dot product)
// with the ROW's term (m8_col_term of the row's sums: the row is the "column" of the swapped call), and the column's term
// (m8_row_term of its sums) is added once, behind the scan: the same integers as the row side, D or -S.  A row past n1
// carries kM8ColMasked instead.  |key''| < 2^23 for a real row, so kM8ColBias - key'' lies in (2^24, 2^26) for a real row
// and below 2^24 for a padding row, and a wave sees 64 rows: (bias - key'') << 6 | (63 - local row) is one unsigned word
// whose DESCENDING order is that of (key, row) ascending.  Its maximum is the best key with the lowest row, the second
// largest word carries the second smallest key of the multiset, and 0 is "nothing yet".  The 16 row terms are kept
// negated, pre-shifted, with the row in their low bits; the accumulator enters shifted by 7 (2 S', L2) or 6, which
// leaves the low 6 bits alone.  Per score: one shift-add, one max, one med3.  Then two cross-lane
// steps fold the four g groups of a column, lanes g == 0 leave (best word, second word) in LDS -- [tile parity][wave][64]
// -- and behind the NEXT tile's barrier 16 lanes of every wave fold the four waves of a column as (key, row) pairs with the
// block's row numbers (m8_merge: the words' local rows do not order rows of different waves) and hand the final keys to
// out.  A buffer is written again two tiles later, behind a barrier that every wave reaches only after its drain.
constexpr int kM8ColBias = 1 << 25;
constexpr int kM8ColMasked = (1 << 25) - (1 << 23);  // bias - masked - 2 S' stays in [2^22, 2^24)
constexpr int kM8ColNone = 1 << 24;                  // key'' = bias - (word >> 6) above this is no row

struct M8NoCols {
  static constexpr bool kOn = false;
};
template <class ColOut>
struct M8Cols {
  static constexpr bool kOn = true;
  uint2 *buf;  // [2][4][kM8TileCols]
  ColOut out;  // out(column, best, second, row): final keys, kM8Init where there is no second
};

__device__ __forceinline__ unsigned umed3(unsigned a, unsigned b, unsigned c) { return max(min(a, b), min(max(a, b), c)); }

// the columns [c_prev, c_prev + 64) of the tile whose words lie in buffer `par`
template <bool kL2, class Cols>
__device__ __forceinline__ void m8_cols_drain(const Cols &cols, const int *__restrict__ sums2, int c_prev, int col_end,
                                              int par, int lane, int wv) {
  const int j = 16 * wv + lane, col = c_prev + j;
  if (lane < 16 && col < col_end) {
    int best = kM8Init, second = kM8Init, idx = -1;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint2 e = cols.buf[(par * 4 + w) * kM8TileCols + j];
      m8_merge(best, second, idx, kM8ColBias - (int)(e.x >> 6), kM8ColBias - (int)(e.y >> 6),
               (int)blockIdx.x * kM8RowsPerBlock + w * kM8RowsPerWave + 63 - (int)(e.x & 63u));
    }
    const int2 s = *reinterpret_cast<const int2 *>(sums2 + 2 * (size_t)col);
    const int ct = m8_row_term<kL2>(s.x, s.y);
    cols.out(col, best + ct, second > kM8ColNone ? kM8Init : second + ct, idx);
  }
}

struct M8NoGuide {
  static constexpr bool kOn = false;
  struct Column {};
};
// One workgroup's 256 rows [blockIdx.x * 256 ..) of (q1, sums1, n1) against the columns [col_begin, col_end) of
// (q2, sums2); col_begin < col_end and blockIdx.x * 256 < n1.  out(row, best, second, idx) receives every row < n1 once,
// with final keys.  Cols = M8Cols: the column side as well, over this workgroup's rows.  Guide = M8GuideH / F / P: only
// the columns that pass the guide's test against a row count for it, and a row that none passes hands out
// (kM8Init, kM8Init, -1); M8NoGuide, every other kernel's, compiles to nothing.
template <bool kL2, class Out, class Cols = M8NoCols, class Guide = M8NoGuide>
__device__ __forceinline__ void m8_block(const unsigned char *__restrict__ q1, const int *__restrict__ sums1, int n1,
                                         const unsigned char *__restrict__ q2, const int *__restrict__ sums2,
                                         int col_begin, int col_end, unsigned char *sB, Out out, Cols cols = Cols{},
                                         Guide guide = Guide{}) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int p1_base = blockIdx.x * kM8RowsPerBlock + wv * kM8RowsPerWave;

  // A fragments: lane (r, g) holds bytes 64 m + 16 g .. + 15 of row p1_base + 16 i + r (i = 0..3, m = 0..1), minus 128.
  // A row past n1 is a copy of the last one; it is never written.
  i32x4 a[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned char *row = q1 + (size_t)min(p1_base + 16 * i + r, n1 - 1) * 128 + 16 * g;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const u4 v = *reinterpret_cast<const u4 *>(row + 64 * m);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[i][m][j] = (int)(v[j] ^ 0x80808080u);
    }
  }
  // running top-2 of rows 16 i + 4 g + j over the columns this lane sees (r mod 16), on key'
  int best[4][4], second[4][4], bidx[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      best[i][j] = second[i][j] = kM8Init;
      bidx[i][j] = -1;
    }
  // column side: the terms of rows 16 i + 4 g + j, biased, shifted, the local row below them
  unsigned cterm[4][4];
  if constexpr (Cols::kOn) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int local = 16 * i + 4 * g + j;
        int term = kM8ColMasked;
        if (p1_base + local < n1) {
          const int2 s = *reinterpret_cast<const int2 *>(sums1 + 2 * (size_t)(p1_base + local));
          term = m8_col_term<kL2>(s.x, s.y);
        }
        cterm[i][j] = ((unsigned)(kM8ColBias - term) << 6) | (unsigned)(63 - local);
      }
  }
  if constexpr (Guide::kOn) guide.rows(n1, p1_base, lane);

  // staging: thread t moves two 16-byte chunks per tile; chunk c = t + 256 k -> column c >> 3, bytes 16 (c & 7).  Raw
  // buffer loads from a descriptor based at the split's first column: a column past col_end reads as 0 and is masked by
  // its term.  Threads 0..63 also fetch the sums of column c0 + t and turn them into the column's term.
  const int n_cols = col_end - col_begin;
  const __amdgpu_buffer_rsrc_t rsrc2 =
      __builtin_amdgcn_make_buffer_rsrc((void *)(q2 + (size_t)col_begin * 128), 0, n_cols * 128, kBufFlags);
  const int voff = (int)(threadIdx.x >> 3) * 128 + 16 * (int)(threadIdx.x & 7);
  u4 stage[2];
  int stage_term = kM8Masked;
  auto fetch = [&](int c0) {
    const int soff = __builtin_amdgcn_readfirstlane((c0 - col_begin) * 128);
#pragma unroll
    for (int k = 0; k < 2; ++k) stage[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc2, voff, soff + 32 * k * 128, 0);
    if (threadIdx.x < kM8TileCols) {
      const int c = c0 + (int)threadIdx.x;
      stage_term = kM8Masked;
      if (c < col_end) {
        const int2 s = *reinterpret_cast<const int2 *>(sums2 + 2 * (size_t)c);
        stage_term = m8_col_term<kL2>(s.x, s.y);
      }
    }
    if constexpr (Guide::kOn) guide.fetch(c0, col_begin, col_end);
  };
  fetch(col_begin);
  int par = 0;
  for (int c0 = col_begin; c0 < col_end; c0 += kM8TileCols, par ^= 1) {
    // buffer `par` was last read two tiles ago, in front of the previous tile's barrier
    unsigned char *buf = sB + par * (kM8TileCols * kM8Stride);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = threadIdx.x + 256 * k;
      u4 v = stage[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] ^= 0x80808080u;
      *reinterpret_cast<u4 *>(buf + (c >> 3) * kM8Stride + 16 * (c & 7)) = v;
    }
    if (threadIdx.x < kM8TileCols) *reinterpret_cast<int *>(buf + threadIdx.x * kM8Stride + 128) = stage_term;
    if constexpr (Guide::kOn) guide.store(buf);
    __syncthreads();
    if (c0 + kM8TileCols < col_end) fetch(c0 + kM8TileCols);  // in flight while this tile is multiplied
    if constexpr (Cols::kOn)
      if (c0 > col_begin) m8_cols_drain<kL2>(cols, sums2, c0 - kM8TileCols, col_end, par ^ 1, lane, wv);

    const unsigned char *bcol = buf + r * kM8Stride + 16 * g;
#pragma unroll
    for (int t = 0; t < kM8TileCols / 16; ++t) {
      const i32x4 b0 = *reinterpret_cast<const i32x4 *>(bcol + 16 * t * kM8Stride);
      const i32x4 b1 = *reinterpret_cast<const i32x4 *>(bcol + 16 * t * kM8Stride + 64);
      const int term = *reinterpret_cast<const int *>(buf + (16 * t + r) * kM8Stride + 128);
      const int p2 = c0 + 16 * t + r;
      // this column's coordinates, read in front of the MFMAs; `live` stays in the update's condition: a column past
      // col_end reads as zeros, and (0, 0) can pass a guide
      [[maybe_unused]] typename Guide::Column xy2{};
      [[maybe_unused]] const bool live = p2 < col_end;
      if constexpr (Guide::kOn) xy2 = guide.column(buf, 16 * t + r);
      i32x4 acc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        acc[i] = i32x4{0, 0, 0, 0};
        acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i][0], b0, acc[i], 0, 0, 0);
        acc[i] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i][1], b1, acc[i], 0, 0, 0);
      }
      // acc[i][j] = S' of row 16 i + 4 g + j and column p2
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          int v = kL2 ? term - 2 * acc[i][j] : term - acc[i][j];
          if constexpr (Guide::kOn) v = (live && guide.pass(i, j, xy2)) ? v : kM8Init;
          const int old = best[i][j];
          best[i][j] = min(old, v);
          second[i][j] = med3i(old, second[i][j], v);
          bidx[i][j] = v < old ? p2 : bidx[i][j];
        }
      if constexpr (Cols::kOn) {
        unsigned cb = 0u, cs = 0u;  // cs <= cb
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const unsigned w = ((unsigned)acc[i][j] << (kL2 ? 7 : 6)) + cterm[i][j];
            const unsigned old = cb;
            cb = max(old, w);
            cs = umed3(old, cs, w);  // the second largest of the three
          }
#pragma unroll
        for (int d = 16; d <= 32; d <<= 1) {  // the four g groups of column p2
          const unsigned ob = __shfl_xor(cb, d);
          const unsigned os = __shfl_xor(cs, d);
          cs = max(min(cb, ob), max(cs, os));
          cb = max(cb, ob);
        }
        if (g == 0) cols.buf[(par * 4 + wv) * kM8TileCols + 16 * t + r] = uint2{cb, cs};
      }
    }
  }
  if constexpr (Cols::kOn) {  // the last tile's columns
    __syncthreads();
    m8_cols_drain<kL2>(cols, sums2, col_begin + (col_end - col_begin - 1) / kM8TileCols * kM8TileCols, col_end, par ^ 1, lane,
                       wv);
  }
  // the tree over the 16 lanes of a row; lane r == 0 of group g ends with rows 16 i + 4 g + j
#pragma unroll
  for (int len = 8; len > 0; len >>= 1)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ob = __shfl_down(best[i][j], len, 16);
        const int os = __shfl_down(second[i][j], len, 16);
        const int oi = __shfl_down(bidx[i][j], len, 16);
        if (r < len) m8_merge(best[i][j], second[i][j], bidx[i][j], ob, os, oi);
      }
  if (r == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int p1 = p1_base + 16 * i + 4 * g + j;
        if (p1 >= n1) continue;
        const int2 s = *reinterpret_cast<const int2 *>(sums1 + 2 * (size_t)p1);
        const int rt = m8_row_term<kL2>(s.x, s.y);
        // a real column's key' is below 2^23 in magnitude; "none" stays none -- under a guide that can be the best too
        int b = best[i][j];
        if constexpr (Guide::kOn)
          b = b >= kM8None ? kM8Init : b + rt;
        else
          b += rt;
        out(p1, b, second[i][j] >= kM8None ? kM8Init : second[i][j] + rt, bidx[i][j]);
      }
  }
}

}  // namespace cusift
