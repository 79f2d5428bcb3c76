// sift_match8.hip -- 8-bit descriptors: the quantiser, the two sums of a byte descriptor, and the brute-force matcher on
// the int8 matrix pipe (v_mfma_i32_16x16x64_i8), for a pair and for a pair list.  The definitions, expression by
// expression, are in include/cusift_amd_extras.h (cusift_quantize_descriptors, cusift_desc8_sums, cusift_match8,
// cusift_match8_batch, cusift_match8_mutual, cusift_match8_batch_mutual); this text is how they are computed.  At the end:
// the registrations' matcher fronts while cusift_ctx_set_match_bits is 8.
//
// Tables: q[n][128] unsigned bytes, dense and 16-byte aligned; sums[n][2] = (sum q, sum q^2) as int.
//
// THE MATCHER.  The int8 MFMA is signed, so both operands are q - 128 (XOR 0x80 on the packed words: the rows once, into
// registers; the columns on their way into LDS).  With a = q1 - 128, b = q2 - 128 and S' = sum a b, which is what the
// accumulators hold:
//     sum a^2 = sum q1^2 - 256 sum q1 + 2^21 = R(row), sum b^2 = C(column) likewise,
//     D = sum (q1 - q2)^2 = R + C - 2 S'            (the shift cancels in the difference)
//     S = sum q1 q2       = S' + 128 (sum q1 + sum q2) - 2^21    (128 (sum a + sum b) + 128^3, all-255: 8,323,200).
// A row's order over the columns does not depend on the row's own term, so the scan of a row runs on
//     key' = C - 2 S'              (L2)        key' = -128 sum q2 - S'      (dot product: the smallest -S)
// -- one integer operation per score, the column's term read from LDS beside its bytes -- and the row's term is added once,
// behind the scan: key = key' + R, or key' - 128 sum q1 + 2^21.  |key'| < 2^23 for every real column.  A column past the
// split's end carries the term 2^30 instead: it can never be best while a real column exists (a split has one), and a
// `second` at or above 2^29 means "no second column", which the write-out turns into cusift_match's initial value.
// The update per score is min, med3, one compare and one select: best = min(best, v); second = med3(best_old, second, v)
// (best_old <= second always, so that is the second smallest of the three); idx = v < best_old ? column : idx.  A lane
// meets its columns in ascending order and compares strictly, so it keeps the lowest column of equal keys; every merge
// (the tree over the 16 lanes of a row, the fold of the column splits) orders (key, column) pairs, so the lowest column
// wins there too and `second` is the second smallest key of the multiset: the result does not depend on scan order, tile
// or split count, and there are no atomics.
//
// Shape: a workgroup is 4 waves x 64 rows (a wave keeps its 64 rows' 128 bytes as four A fragments, 32 registers) against
// one contiguous range of columns (blockIdx.y); the columns pass through LDS in tiles of 64 (two buffers, one barrier per
// tile; the next tile's global loads are in flight in registers while this one is multiplied).  Per B fragment -- 16
// columns x 128 bytes, two ds_read_b128 -- a wave issues 8 MFMAs (4 row groups x 2 k halves) and updates 16 scores per
// lane.  The k order inside a fragment is whatever 16 consecutive bytes per lane give: A and B load the same byte
// positions (bytes 64 m + 16 g .. + 15 of their row / column in lane (r, g), MFMA m), which is all a dot product needs.
// C/D: col = lane & 15, row = 4 (lane >> 4) + reg.
#include "sift_host.h"

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

// final keys -> the three values cusift_match's tail works on
template <bool kL2>
__device__ __forceinline__ void m8_floats(int best, int second, float &fb, float &fs) {
  fb = kL2 ? (float)best * kM8Scale : (float)(-best) * kM8Scale;
  fs = second >= kM8None ? (kL2 ? kM8FltMax : -1.0f) : (kL2 ? (float)second * kM8Scale : (float)(-second) * kM8Scale);
}

// cusift_match's tail on them (sift_match_common.h): the five fields of a record, or a row of a pair's row array
template <bool kL2>
__device__ __forceinline__ void m8_write_point(cusift_point *pt, const cusift_point *__restrict__ sift2, int n2, int best,
                                               int second, int idx) {
  float fb, fs;
  m8_floats<kL2>(best, second, fb, fs);
  write_match(pt, sift2, n2, fb, fs, idx, kL2);
}
template <bool kL2>
__device__ __forceinline__ void m8_write_row(cusift_match_row *__restrict__ row, int best, int second, int idx) {
  float fb, fs;
  m8_floats<kL2>(best, second, fb, fs);
  write_match_row(row, fb, fs, idx, kL2);
}

// The two sinks of the main kernels (partial_or, sift_match_common.h): the keys of record i of `dst` against the records
// `other`, and of row i of a pair's row array.
template <bool kL2>
__device__ __forceinline__ auto m8_point_sink(Match8Partial *partials, size_t slab, cusift_point *dst,
                                              const cusift_point *other, int n_other) {
  return partial_or(partials, slab,
                    [=](int i, int b, int s, int idx) { m8_write_point<kL2>(dst + i, other, n_other, b, s, idx); });
}
template <bool kL2>
__device__ __forceinline__ auto m8_row_sink(Match8Partial *partials, size_t slab, cusift_match_row *rows) {
  return partial_or(partials, slab, [=](int i, int b, int s, int idx) { m8_write_row<kL2>(rows + i, b, s, idx); });
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

// One workgroup's 256 rows [blockIdx.x * 256 ..) of (q1, sums1, n1) against the columns [col_begin, col_end) of
// (q2, sums2); col_begin < col_end and blockIdx.x * 256 < n1.  out(row, best, second, idx) receives every row < n1 once,
// with final keys.  Cols = M8Cols: the column side as well, over this workgroup's rows.
template <bool kL2, class Out, class Cols = M8NoCols>
__device__ __forceinline__ void m8_block(const unsigned char *__restrict__ q1, const int *__restrict__ sums1, int n1,
                                         const unsigned char *__restrict__ q2, const int *__restrict__ sums2,
                                         int col_begin, int col_end, unsigned char *sB, Out out, Cols cols = Cols{}) {
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
          const int v = kL2 ? term - 2 * acc[i][j] : term - acc[i][j];
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
        // a real column's key' is below 2^23 in magnitude; "none" stays none
        out(p1, best[i][j] + rt, second[i][j] >= kM8None ? kM8Init : second[i][j] + rt, bidx[i][j]);
      }
  }
}

// One pair.  grid (row blocks, column splits).  partials == NULL (one split): the five fields are final; otherwise
// partials[split][n1_pad] and match8_merge_kernel folds them.
template <bool kL2>
__global__ void __launch_bounds__(256) match8_kernel(cusift_point *__restrict__ sift1, int n1,
                                                    const unsigned char *__restrict__ q1, const int *__restrict__ sums1,
                                                    const cusift_point *__restrict__ sift2, int n2,
                                                    const unsigned char *__restrict__ q2, const int *__restrict__ sums2,
                                                    int cols_per_split, Match8Partial *__restrict__ partials, int n1_pad) {
  __shared__ __attribute__((aligned(16))) unsigned char sB[2 * kM8TileCols * kM8Stride];
  const int col_begin = blockIdx.y * cols_per_split;
  const int col_end = min(col_begin + cols_per_split, n2);
  if (col_begin >= col_end) return;  // uniform; the host sizes the splits so that this never happens
  m8_block<kL2>(q1, sums1, n1, q2, sums2, col_begin, col_end, sB,
                m8_point_sink<kL2>(partials, (size_t)blockIdx.y * n1_pad, sift1, sift2, n2));
}
template __global__ void match8_kernel<false>(cusift_point *, int, const unsigned char *, const int *, const cusift_point *,
                                              int, const unsigned char *, const int *, int, Match8Partial *, int);
template __global__ void match8_kernel<true>(cusift_point *, int, const unsigned char *, const int *, const cusift_point *,
                                             int, const unsigned char *, const int *, int, Match8Partial *, int);

template <bool kL2>
__global__ void __launch_bounds__(256) match8_merge_kernel(cusift_point *__restrict__ sift1, int n1,
                                                          const cusift_point *__restrict__ sift2, int n2,
                                                          const Match8Partial *__restrict__ partials, int n1_pad,
                                                          int n_splits) {
  const int p1 = blockIdx.x * 256 + threadIdx.x;
  if (p1 >= n1) return;
  const Match8Partial m = fold_partials(partials + p1, n1_pad, n_splits, M8Merge{});
  m8_write_point<kL2>(sift1 + p1, sift2, n2, m.best, m.second, m.idx);
}

// The pair list: a workgroup is (row block, column split, pair) of PairFrame (sift_match_common.h); one without rows or
// without columns returns before it loads a byte.
template <bool kL2>
__global__ void __launch_bounds__(256) match8_batch_kernel(const unsigned char *__restrict__ q, const int *__restrict__ sums,
                                                          const unsigned int *__restrict__ counters, int max_pts,
                                                          const int *__restrict__ pairs, int cols_per_split,
                                                          Match8Partial *__restrict__ partials, int n1_pad,
                                                          cusift_match_row *__restrict__ rows) {
  __shared__ __attribute__((aligned(16))) unsigned char sB[2 * kM8TileCols * kM8Stride];
  const PairFrame fr(counters, pairs, max_pts, cols_per_split, kM8RowsPerBlock);
  if (fr.empty) return;
  m8_block<kL2>(q + (size_t)fr.f1 * max_pts * 128, sums + (size_t)fr.f1 * max_pts * 2, fr.n1,
                q + (size_t)fr.f2 * max_pts * 128, sums + (size_t)fr.f2 * max_pts * 2, fr.col_begin, fr.col_end, sB,
                m8_row_sink<kL2>(partials, ((size_t)fr.pair * gridDim.y + blockIdx.y) * n1_pad,
                                 rows + (size_t)fr.pair * max_pts));
}
template __global__ void match8_batch_kernel<false>(const unsigned char *, const int *, const unsigned int *, int,
                                                    const int *, int, Match8Partial *, int, cusift_match_row *);
template __global__ void match8_batch_kernel<true>(const unsigned char *, const int *, const unsigned int *, int,
                                                   const int *, int, Match8Partial *, int, cusift_match_row *);

// match8_merge_kernel per pair (blockIdx.y): folds the splits that had columns
template <bool kL2>
__global__ void __launch_bounds__(256) match8_batch_merge_kernel(const unsigned int *__restrict__ counters, int max_pts,
                                                                const int *__restrict__ pairs, int cols_per_split,
                                                                const Match8Partial *__restrict__ partials, int n1_pad,
                                                                int n_splits, cusift_match_row *__restrict__ rows) {
  const PairCounts pc(blockIdx.y, counters, pairs, max_pts);
  const int p1 = blockIdx.x * 256 + threadIdx.x;
  if (p1 >= pc.n1 || pc.n2 <= 0) return;
  const int live = min(n_splits, (pc.n2 + cols_per_split - 1) / cols_per_split);  // the others wrote nothing
  const Match8Partial m = fold_partials(partials + (size_t)pc.pair * n_splits * n1_pad + p1, n1_pad, live, M8Merge{});
  m8_write_row<kL2>(rows + (size_t)pc.pair * max_pts + p1, m.best, m.second, m.idx);
}

// ---- both directions from one pass ---------------------------------------------------------------------------------------
// match8_kernel with the column side: set 2's five fields, or -- with more than one row block -- col_partials[row block][n2]
// for match8_mutual_merge_kernel.  Column splits partition the columns, so every (row block, column) is written once.
template <bool kL2>
__global__ void __launch_bounds__(256) match8_mutual_kernel(cusift_point *sift1, int n1, const unsigned char *__restrict__ q1,
                                                           const int *__restrict__ sums1, cusift_point *sift2, int n2,
                                                           const unsigned char *__restrict__ q2,
                                                           const int *__restrict__ sums2, int cols_per_split,
                                                           Match8Partial *__restrict__ partials, int n1_pad,
                                                           Match8Partial *__restrict__ col_partials) {
  __shared__ __attribute__((aligned(16))) unsigned char sB[2 * kM8TileCols * kM8Stride];
  __shared__ uint2 sCols[2 * 4 * kM8TileCols];
  const int col_begin = blockIdx.y * cols_per_split;
  const int col_end = min(col_begin + cols_per_split, n2);
  if (col_begin >= col_end) return;  // uniform; the host sizes the splits so that this never happens
  const auto col_out = m8_point_sink<kL2>(col_partials, (size_t)blockIdx.x * n2, sift2, sift1, n1);
  m8_block<kL2>(q1, sums1, n1, q2, sums2, col_begin, col_end, sB,
                m8_point_sink<kL2>(partials, (size_t)blockIdx.y * n1_pad, sift1, sift2, n2),
                M8Cols<decltype(col_out)>{sCols, col_out});
}
template __global__ void match8_mutual_kernel<false>(cusift_point *, int, const unsigned char *, const int *, cusift_point *,
                                                     int, const unsigned char *, const int *, int, Match8Partial *, int,
                                                     Match8Partial *);
template __global__ void match8_mutual_kernel<true>(cusift_point *, int, const unsigned char *, const int *, cusift_point *,
                                                    int, const unsigned char *, const int *, int, Match8Partial *, int,
                                                    Match8Partial *);

// folds the row blocks of one column
template <bool kL2>
__global__ void __launch_bounds__(256) match8_mutual_merge_kernel(cusift_point *__restrict__ sift2, int n2,
                                                                 const cusift_point *__restrict__ sift1, int n1,
                                                                 const Match8Partial *__restrict__ col_partials,
                                                                 int row_blocks) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n2) return;
  const Match8Partial m = fold_partials(col_partials + j, n2, row_blocks, M8Merge{});
  m8_write_point<kL2>(sift2 + j, sift1, n1, m.best, m.second, m.idx);
}

// match8_batch_kernel with the column side in rows_back[pair][max_pts]; col_partials[pair][row block][max_pts], NULL when
// max_pts fits one row block.
template <bool kL2>
__global__ void __launch_bounds__(256) match8_batch_mutual_kernel(const unsigned char *__restrict__ q,
                                                                 const int *__restrict__ sums,
                                                                 const unsigned int *__restrict__ counters, int max_pts,
                                                                 const int *__restrict__ pairs, int cols_per_split,
                                                                 Match8Partial *__restrict__ partials, int n1_pad,
                                                                 cusift_match_row *__restrict__ rows,
                                                                 Match8Partial *__restrict__ col_partials,
                                                                 cusift_match_row *__restrict__ rows_back) {
  __shared__ __attribute__((aligned(16))) unsigned char sB[2 * kM8TileCols * kM8Stride];
  __shared__ uint2 sCols[2 * 4 * kM8TileCols];
  const PairFrame fr(counters, pairs, max_pts, cols_per_split, kM8RowsPerBlock);
  if (fr.empty) return;
  const auto col_out = m8_row_sink<kL2>(col_partials, ((size_t)fr.pair * gridDim.x + blockIdx.x) * max_pts,
                                        rows_back + (size_t)fr.pair * max_pts);
  m8_block<kL2>(q + (size_t)fr.f1 * max_pts * 128, sums + (size_t)fr.f1 * max_pts * 2, fr.n1,
                q + (size_t)fr.f2 * max_pts * 128, sums + (size_t)fr.f2 * max_pts * 2, fr.col_begin, fr.col_end, sB,
                m8_row_sink<kL2>(partials, ((size_t)fr.pair * gridDim.y + blockIdx.y) * n1_pad,
                                 rows + (size_t)fr.pair * max_pts),
                M8Cols<decltype(col_out)>{sCols, col_out});
}
template __global__ void match8_batch_mutual_kernel<false>(const unsigned char *, const int *, const unsigned int *, int,
                                                           const int *, int, Match8Partial *, int, cusift_match_row *,
                                                           Match8Partial *, cusift_match_row *);
template __global__ void match8_batch_mutual_kernel<true>(const unsigned char *, const int *, const unsigned int *, int,
                                                          const int *, int, Match8Partial *, int, cusift_match_row *,
                                                          Match8Partial *, cusift_match_row *);

// match8_mutual_merge_kernel per pair (blockIdx.y): folds the row blocks that had rows
template <bool kL2>
__global__ void __launch_bounds__(256) match8_batch_mutual_merge_kernel(const unsigned int *__restrict__ counters,
                                                                       int max_pts, const int *__restrict__ pairs,
                                                                       const Match8Partial *__restrict__ col_partials,
                                                                       int row_blocks,
                                                                       cusift_match_row *__restrict__ rows_back) {
  const PairCounts pc(blockIdx.y, counters, pairs, max_pts);
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= pc.n2 || pc.n1 <= 0) return;
  const int live = min(row_blocks, (pc.n1 + kM8RowsPerBlock - 1) / kM8RowsPerBlock);  // the others wrote nothing
  const Match8Partial m =
      fold_partials(col_partials + (size_t)pc.pair * row_blocks * max_pts + j, max_pts, live, M8Merge{});
  m8_write_row<kL2>(rows_back + (size_t)pc.pair * max_pts + j, m.best, m.second, m.idx);
}

// ---- the quantiser --------------------------------------------------------------------------------------------------------
// 32 lanes per record: lane l reads floats 4 l .. 4 l + 3 (16 bytes; the 588-byte records are only 4-byte aligned),
// writes one packed word -- a record's 128 bytes are one 128-byte line -- and the 32 lanes' sums meet by
// shuffles inside the half wave.  8 records per workgroup; grid (record blocks, images).
typedef float f4u8 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ int quantize_one(float v) {
  const float t = 512.0f * v;  // exact
  const float u = t + 0.5f;    // one rounding
  return (v > 0.0f) ? (u < 255.0f ? (int)u : 255) : 0;
}

__global__ void __launch_bounds__(256) quantize_kernel(const cusift_point *__restrict__ points,
                                                      const unsigned int *__restrict__ counters, int max_pts,
                                                      unsigned char *__restrict__ q, int *__restrict__ sums) {
  const int img = blockIdx.y;
  const int n = frame_count(counters, img, max_pts);
  const int rec = blockIdx.x * 8 + (int)(threadIdx.x >> 5);
  const int l = threadIdx.x & 31;
  if (rec >= n) return;  // uniform over the record's 32 lanes: the shuffles below stay inside them
  const size_t at = (size_t)img * max_pts + rec;
  const f4u8 v = *reinterpret_cast<const f4u8 *>(points[at].data + 4 * l);
  unsigned int word = 0;
  int s = 0, s2 = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int b = quantize_one(v[j]);
    word |= (unsigned int)b << (8 * j);
    s += b;
    s2 += b * b;
  }
  reinterpret_cast<unsigned int *>(q + at * 128)[l] = word;
#pragma unroll
  for (int d = 16; d > 0; d >>= 1) {
    s += __shfl_xor(s, d, 32);
    s2 += __shfl_xor(s2, d, 32);
  }
  if (l == 0) *reinterpret_cast<int2 *>(sums + 2 * at) = int2{s, s2};
}

// 8 lanes per record, 16 bytes each
__global__ void __launch_bounds__(256) desc8_sums_kernel(const unsigned char *__restrict__ q, int n, int *__restrict__ sums) {
  const int rec = blockIdx.x * 32 + (int)(threadIdx.x >> 3);
  const int l = threadIdx.x & 7;
  if (rec >= n) return;  // uniform over the record's 8 lanes
  const u4 v = *reinterpret_cast<const u4 *>(q + (size_t)rec * 128 + 16 * l);
  int s = 0, s2 = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int b = (int)((v[j] >> (8 * k)) & 0xffu);
      s += b;
      s2 += b * b;
    }
#pragma unroll
  for (int d = 4; d > 0; d >>= 1) {
    s += __shfl_xor(s, d, 8);
    s2 += __shfl_xor(s2, d, 8);
  }
  if (l == 0) *reinterpret_cast<int2 *>(sums + 2 * (size_t)rec) = int2{s, s2};
}

}  // namespace cusift

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

static_assert(kMatcher8.rows_per_block == kM8RowsPerBlock && kMatcher8.tile_cols == kM8TileCols,
              "the split plan's shape (sift_host.h) is the kernels'");

extern "C" int cusift_quantize_descriptors(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters,
                                           int n_images, int max_pts, unsigned char *d_q, int *d_sums) {
  TRY(enter(ctx));
  if (n_images < 0 || n_images > 65535 || max_pts < 0 || max_pts > (1 << 24))
    return fail(CUSIFT_ERR_INVALID, "QuantizeDescriptors: n_images %d outside [0, 65535] or max_pts %d outside [0, 2^24]",
                n_images, max_pts);
  if (n_images == 0 || max_pts == 0) return CUSIFT_OK;
  if (!d_points || !d_q || !d_sums) return fail(CUSIFT_ERR_INVALID, "QuantizeDescriptors: missing data");
  if (!aligned16(d_q)) return fail(CUSIFT_ERR_INVALID, "QuantizeDescriptors: d_q must be 16-byte aligned");
  if (((uintptr_t)d_sums & 7) != 0) return fail(CUSIFT_ERR_INVALID, "QuantizeDescriptors: d_sums must be 8-byte aligned");
  hipLaunchKernelGGL(quantize_kernel, dim3(idiv_up(max_pts, 8), n_images), dim3(256), 0, ctx->stream, d_points, d_counters,
                     max_pts, d_q, d_sums);
  return check_launch("quantize_descriptors");
}

extern "C" int cusift_desc8_sums(cusift_ctx *ctx, const unsigned char *d_q, int n, int *d_sums) {
  TRY(enter(ctx));
  if (n <= 0) return CUSIFT_OK;
  if (!d_q || !d_sums) return fail(CUSIFT_ERR_INVALID, "Desc8Sums: missing data");
  if (!aligned16(d_q)) return fail(CUSIFT_ERR_INVALID, "Desc8Sums: d_q must be 16-byte aligned");
  if (((uintptr_t)d_sums & 7) != 0) return fail(CUSIFT_ERR_INVALID, "Desc8Sums: d_sums must be 8-byte aligned");
  hipLaunchKernelGGL(desc8_sums_kernel, dim3(idiv_up(n, 32)), dim3(256), 0, ctx->stream, d_q, n, d_sums);
  return check_launch("desc8_sums");
}

static int check_tables8(const char *who, const unsigned char *d_q, const int *d_sums) {
  if (!d_q || !d_sums) return fail(CUSIFT_ERR_INVALID, "%s: missing data", who);
  if (!aligned16(d_q)) return fail(CUSIFT_ERR_INVALID, "%s: a descriptor table must be 16-byte aligned", who);
  if (((uintptr_t)d_sums & 7) != 0) return fail(CUSIFT_ERR_INVALID, "%s: a sums table must be 8-byte aligned", who);
  return CUSIFT_OK;
}


// The matcher of one pair: one launch, plus the row-side merge when the columns are split.  d_back != NULL
// (cusift_match8_mutual): image 2's records again, to receive the column side, merged when there are several row blocks.
// Both counts >= 1, the arguments are checked.
static int match8_launch(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const unsigned char *d_q1,
                         const int *d_sums1, const cusift_point *d_sift2, int num_pts2, const unsigned char *d_q2,
                         const int *d_sums2, int distance, cusift_point *d_back) {
  const int row_blocks = idiv_up(num_pts1, kM8RowsPerBlock);
  int splits, cols_per_split;
  TRY(matcher_split_plan(ctx, kMatcher8, num_pts1, num_pts2, 1, &splits, &cols_per_split));
  const int n1_pad = row_blocks * kM8RowsPerBlock;
  Match8Partial *partials = nullptr, *col_partials = nullptr;
  if (splits > 1) {
    const size_t bytes = sizeof(Match8Partial) * (size_t)splits * n1_pad;
    TRY(grow_scratch(ctx, ctx->match_scratch, ctx->match_scratch_bytes, bytes, "", true));
    partials = reinterpret_cast<Match8Partial *>(ctx->match_scratch);
  }
  if (d_back && row_blocks > 1) {
    const size_t bytes = sizeof(Match8Partial) * (size_t)row_blocks * num_pts2;
    TRY(grow_scratch(ctx, ctx->match_col_scratch, ctx->match_col_scratch_bytes, bytes, "", false));
    col_partials = reinterpret_cast<Match8Partial *>(ctx->match_col_scratch);
  }
  if (d_back)
    hipLaunchKernelGGL(distance ? match8_mutual_kernel<true> : match8_mutual_kernel<false>, dim3(row_blocks, splits),
                       dim3(256), 0, ctx->stream, d_sift1, num_pts1, d_q1, d_sums1, d_back, num_pts2, d_q2, d_sums2,
                       cols_per_split, partials, n1_pad, col_partials);
  else
    hipLaunchKernelGGL(distance ? match8_kernel<true> : match8_kernel<false>, dim3(row_blocks, splits), dim3(256), 0,
                       ctx->stream, d_sift1, num_pts1, d_q1, d_sums1, d_sift2, num_pts2, d_q2, d_sums2, cols_per_split,
                       partials, n1_pad);
  if (splits > 1)
    hipLaunchKernelGGL(distance ? match8_merge_kernel<true> : match8_merge_kernel<false>, dim3(idiv_up(num_pts1, 256)),
                       dim3(256), 0, ctx->stream, d_sift1, num_pts1, d_sift2, num_pts2,
                       (const Match8Partial *)partials, n1_pad, splits);
  if (col_partials)
    hipLaunchKernelGGL(distance ? match8_mutual_merge_kernel<true> : match8_mutual_merge_kernel<false>,
                       dim3(idiv_up(num_pts2, 256)), dim3(256), 0, ctx->stream, d_back, num_pts2,
                       (const cusift_point *)d_sift1, num_pts1, (const Match8Partial *)col_partials, row_blocks);
  return check_launch(d_back ? "match8_mutual" : "match8");
}

extern "C" int cusift_match8(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const unsigned char *d_q1,
                             const int *d_sums1, const cusift_point *d_sift2, int num_pts2, const unsigned char *d_q2,
                             const int *d_sums2, int distance) {
  TRY(enter(ctx));
  if (num_pts1 <= 0 || num_pts2 <= 0) return CUSIFT_OK;  // as cusift_match: nothing to match
  if (!d_sift1 || !d_sift2) return fail(CUSIFT_ERR_INVALID, "Match8: missing data");
  TRY(check_tables8("Match8", d_q1, d_sums1));
  TRY(check_tables8("Match8", d_q2, d_sums2));
  TRY(check_distance("Match8", distance));
  return match8_launch(ctx, d_sift1, num_pts1, d_q1, d_sums1, d_sift2, num_pts2, d_q2, d_sums2, distance, nullptr);
}

// Both directions from one pass over the scores.  Both record sets are written, so their ranges must not overlap.
extern "C" int cusift_match8_mutual(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const unsigned char *d_q1,
                                    const int *d_sums1, cusift_point *d_sift2, int num_pts2, const unsigned char *d_q2,
                                    const int *d_sums2, int distance) {
  TRY(enter(ctx));
  if (num_pts1 <= 0 || num_pts2 <= 0) return CUSIFT_OK;  // nothing to match, on either side
  if (!d_sift1 || !d_sift2) return fail(CUSIFT_ERR_INVALID, "Match8Mutual: missing data");
  TRY(check_tables8("Match8Mutual", d_q1, d_sums1));
  TRY(check_tables8("Match8Mutual", d_q2, d_sums2));
  TRY(check_distance("Match8Mutual", distance));
  TRY(check_disjoint("Match8Mutual", d_sift1, num_pts1, d_sift2, num_pts2));
  return match8_launch(ctx, d_sift1, num_pts1, d_q1, d_sums1, d_sift2, num_pts2, d_q2, d_sums2, distance, d_sift2);
}

// Uploads the pair list and enqueues the matcher of every pair: one launch, plus a merge when the columns are split and
// -- with d_rows_back, the column side -- one more when max_pts spans several row blocks.  *d_pairs_out: the list on the
// device.  n_pairs >= 1, max_pts >= 1, the arguments are checked.
int match8_batch_launch(cusift_ctx *ctx, const unsigned char *d_q, const int *d_sums, const unsigned int *d_counters,
                        int max_pts, const int *h_pairs, int n_pairs, int distance, cusift_match_row *d_rows,
                        cusift_match_row *d_rows_back, const int **d_pairs_out) {
  const int row_blocks = idiv_up(max_pts, kM8RowsPerBlock);
  int splits, cols_per_split;
  TRY(matcher_split_plan(ctx, kMatcher8, max_pts, max_pts, n_pairs, &splits, &cols_per_split));
  const int n1_pad = row_blocks * kM8RowsPerBlock;
  const size_t list_b = align_up_sz(sizeof(int) * 2 * (size_t)n_pairs, 256);
  const size_t part_b = splits > 1 ? sizeof(Match8Partial) * (size_t)n_pairs * splits * n1_pad : 0;
  const size_t col_b = d_rows_back && row_blocks > 1 ? sizeof(Match8Partial) * (size_t)n_pairs * row_blocks * max_pts : 0;
  TRY(grow_scratch(ctx, ctx->pairs_scratch, ctx->pairs_scratch_bytes, list_b + part_b + col_b, "", false));
  int *d_pairs = (int *)ctx->pairs_scratch;
  Match8Partial *partials = splits > 1 ? (Match8Partial *)(ctx->pairs_scratch + list_b) : nullptr;
  Match8Partial *col_partials = col_b ? (Match8Partial *)(ctx->pairs_scratch + list_b + part_b) : nullptr;
  HIP_TRY(hipMemcpyAsync(d_pairs, h_pairs, sizeof(int) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice, ctx->stream));
  const dim3 grid(row_blocks, splits, n_pairs);
  if (d_rows_back)
    hipLaunchKernelGGL(distance ? match8_batch_mutual_kernel<true> : match8_batch_mutual_kernel<false>, grid, dim3(256), 0,
                       ctx->stream, d_q, d_sums, d_counters, max_pts, (const int *)d_pairs, cols_per_split, partials,
                       n1_pad, d_rows, col_partials, d_rows_back);
  else
    hipLaunchKernelGGL(distance ? match8_batch_kernel<true> : match8_batch_kernel<false>, grid, dim3(256), 0, ctx->stream,
                       d_q, d_sums, d_counters, max_pts, (const int *)d_pairs, cols_per_split, partials, n1_pad, d_rows);
  if (splits > 1)
    hipLaunchKernelGGL(distance ? match8_batch_merge_kernel<true> : match8_batch_merge_kernel<false>,
                       dim3(idiv_up(max_pts, 256), n_pairs), dim3(256), 0, ctx->stream, d_counters, max_pts,
                       (const int *)d_pairs, cols_per_split, (const Match8Partial *)partials, n1_pad, splits, d_rows);
  if (col_partials)
    hipLaunchKernelGGL(distance ? match8_batch_mutual_merge_kernel<true> : match8_batch_mutual_merge_kernel<false>,
                       dim3(idiv_up(max_pts, 256), n_pairs), dim3(256), 0, ctx->stream, d_counters, max_pts,
                       (const int *)d_pairs, (const Match8Partial *)col_partials, row_blocks, d_rows_back);
  if (d_pairs_out) *d_pairs_out = d_pairs;
  return check_launch(d_rows_back ? "match8_batch_mutual" : "match8_batch");
}

// every refusal of the 8-bit pair-list calls; *nothing: a list or a capacity of zero
static int check_batch8(const char *who, const unsigned char *d_q, const int *d_sums, int n_images, int max_pts,
                        const int *h_pairs, int n_pairs, int distance, const cusift_match_row *d_rows, bool *nothing) {
  *nothing = true;
  TRY(check_distance(who, distance));
  TRY(check_pair_list(h_pairs, n_pairs, n_images, max_pts, who));
  if (n_pairs == 0 || max_pts == 0) return CUSIFT_OK;
  if (!d_rows) return fail(CUSIFT_ERR_INVALID, "%s: missing data", who);
  TRY(check_tables8(who, d_q, d_sums));
  *nothing = false;
  return CUSIFT_OK;
}

extern "C" int cusift_match8_batch(cusift_ctx *ctx, const unsigned char *d_q, const int *d_sums,
                                   const unsigned int *d_counters, int n_images, int max_pts, const int *h_pairs,
                                   int n_pairs, int distance, cusift_match_row *d_rows) {
  TRY(enter(ctx));
  bool nothing;
  TRY(check_batch8("Match8Batch", d_q, d_sums, n_images, max_pts, h_pairs, n_pairs, distance, d_rows, &nothing));
  if (nothing) return CUSIFT_OK;
  return match8_batch_launch(ctx, d_q, d_sums, d_counters, max_pts, h_pairs, n_pairs, distance, d_rows, nullptr, nullptr);
}

extern "C" int cusift_match8_batch_mutual(cusift_ctx *ctx, const unsigned char *d_q, const int *d_sums,
                                          const unsigned int *d_counters, int n_images, int max_pts, const int *h_pairs,
                                          int n_pairs, int distance, cusift_match_row *d_rows,
                                          cusift_match_row *d_rows_back) {
  TRY(enter(ctx));
  bool nothing;
  if (!d_rows_back) return fail(CUSIFT_ERR_INVALID, "Match8BatchMutual: NULL d_rows_back");
  TRY(check_batch8("Match8BatchMutual", d_q, d_sums, n_images, max_pts, h_pairs, n_pairs, distance, d_rows, &nothing));
  if (nothing) return CUSIFT_OK;
  if (d_rows_back == d_rows) return fail(CUSIFT_ERR_INVALID, "Match8BatchMutual: d_rows_back must be distinct from d_rows");
  return match8_batch_launch(ctx, d_q, d_sums, d_counters, max_pts, h_pairs, n_pairs, distance, d_rows, d_rows_back,
                             nullptr);
}

// ---- the registrations' matcher front while cusift_ctx_set_match_bits is 8 (sift_register.hip) ---------------------------
// The byte tables live in the context: q [n][128] on a 256-byte boundary, the sums behind them on another.
static int tables8_scratch(cusift_ctx *ctx, size_t n, unsigned char **q, int **sums) {
  const size_t q_b = align_up_sz(128 * n, 256);
  TRY(grow_scratch(ctx, ctx->q8_scratch, ctx->q8_scratch_bytes, q_b + align_up_sz(8 * n, 256), "", false));
  *q = reinterpret_cast<unsigned char *>(ctx->q8_scratch);
  *sums = reinterpret_cast<int *>(ctx->q8_scratch + q_b);
  return CUSIFT_OK;
}

// cusift_quantize_descriptors of both record sets, then cusift_match8 -- d_back != NULL: cusift_match8_mutual.  Counts
// >= 1, the arguments are checked.
int match8_pair_enqueue(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2, int num_pts2,
                        int distance, cusift_point *d_back) {
  unsigned char *q;
  int *sums;
  const size_t n1_slots = align_up_sz((size_t)num_pts1, 32);  // keeps table 2 and its sums aligned
  TRY(tables8_scratch(ctx, n1_slots + (size_t)num_pts2, &q, &sums));
  unsigned char *q2 = q + 128 * n1_slots;
  int *sums2 = sums + 2 * n1_slots;
  hipLaunchKernelGGL(quantize_kernel, dim3(idiv_up(num_pts1, 8), 1), dim3(256), 0, ctx->stream,
                     (const cusift_point *)d_sift1, (const unsigned int *)nullptr, num_pts1, q, sums);
  hipLaunchKernelGGL(quantize_kernel, dim3(idiv_up(num_pts2, 8), 1), dim3(256), 0, ctx->stream, d_sift2,
                     (const unsigned int *)nullptr, num_pts2, q2, sums2);
  return match8_launch(ctx, d_sift1, num_pts1, q, sums, d_sift2, num_pts2, q2, sums2, distance, d_back);
}

// cusift_quantize_descriptors of the whole batch, then cusift_match8_batch -- d_rows_back != NULL: _batch_mutual.
int match8_batch_enqueue(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters, int n_images,
                         int max_pts, const int *h_pairs, int n_pairs, int distance, cusift_match_row *d_rows,
                         cusift_match_row *d_rows_back, const int **d_pairs_out) {
  unsigned char *q;
  int *sums;
  TRY(tables8_scratch(ctx, (size_t)n_images * max_pts, &q, &sums));
  hipLaunchKernelGGL(quantize_kernel, dim3(idiv_up(max_pts, 8), n_images), dim3(256), 0, ctx->stream, d_points, d_counters,
                     max_pts, q, sums);
  return match8_batch_launch(ctx, q, sums, d_counters, max_pts, h_pairs, n_pairs, distance, d_rows, d_rows_back,
                             d_pairs_out);
}
