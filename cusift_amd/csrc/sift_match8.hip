// sift_match8.hip -- 8-bit descriptors: the quantiser, the two sums of a byte descriptor, and the brute-force matcher on
// the int8 matrix pipe (v_mfma_i32_16x16x64_i8), for a pair and for a pair list.  The definitions, expression by
// expression, are in include/cusift_amd_extras.h (cusift_quantize_descriptors, cusift_desc8_sums, cusift_match8,
// cusift_match8_batch, cusift_match8_mutual, cusift_match8_batch_mutual); this text is how they are computed.  The block
// body is sift_match8_block.h, shared with the guided kernels of sift_match8_guided.hip, whose launches and entry points
// (cusift_match8_guided, cusift_match8_projected, their pair-list forms) are here too.  At the end: the registrations'
// matcher fronts while cusift_ctx_set_match_bits is 8.
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

#include "sift_match8_block.h"

namespace cusift {

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
// guide != NULL (cusift_match8_guided, cusift_match8_projected, never with d_back): the guided kernel, its model a kernel
// argument, and the none-aware merge.  Both counts >= 1, the arguments are checked.
static int match8_launch(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const unsigned char *d_q1,
                         const int *d_sums1, const cusift_point *d_sift2, int num_pts2, const unsigned char *d_q2,
                         const int *d_sums2, int distance, cusift_point *d_back, const GuideCall *guide = nullptr) {
  const int row_blocks = idiv_up(num_pts1, kM8RowsPerBlock);
  int splits, cols_per_split;
  TRY(matcher_split_plan(ctx, guide ? kMatcher8Guided : kMatcher8, num_pts1, num_pts2, 1, &splits, &cols_per_split));
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
  else if (guide && guide->camera) {
    const auto kernel = distance ? match8_guided_kernel<true, M8GuideP, ProjectModel> : match8_guided_kernel<false, M8GuideP, ProjectModel>;
    hipLaunchKernelGGL(kernel, dim3(row_blocks, splits), dim3(256), 0, ctx->stream, d_sift1, num_pts1, d_q1, d_sums1,
                       d_sift2, num_pts2, d_q2, d_sums2, cols_per_split, partials, n1_pad,
                       project_model(guide->h_models, *guide->camera), guide->r2);
  } else if (guide) {
    GuideModel model;
    memcpy(model.m, guide->h_models, sizeof(model.m));
    const auto kernel =
        guide->model == CUSIFT_GUIDE_EPIPOLAR
            ? (distance ? match8_guided_kernel<true, M8GuideF, GuideModel> : match8_guided_kernel<false, M8GuideF, GuideModel>)
            : (distance ? match8_guided_kernel<true, M8GuideH, GuideModel> : match8_guided_kernel<false, M8GuideH, GuideModel>);
    hipLaunchKernelGGL(kernel, dim3(row_blocks, splits), dim3(256), 0, ctx->stream, d_sift1, num_pts1, d_q1, d_sums1,
                       d_sift2, num_pts2, d_q2, d_sums2, cols_per_split, partials, n1_pad, model, guide->r2);
  } else
    hipLaunchKernelGGL(distance ? match8_kernel<true> : match8_kernel<false>, dim3(row_blocks, splits), dim3(256), 0,
                       ctx->stream, d_sift1, num_pts1, d_q1, d_sums1, d_sift2, num_pts2, d_q2, d_sums2, cols_per_split,
                       partials, n1_pad);
  if (splits > 1 && guide)
    hipLaunchKernelGGL(distance ? match8_guided_merge_kernel<true> : match8_guided_merge_kernel<false>,
                       dim3(idiv_up(num_pts1, 256)), dim3(256), 0, ctx->stream, d_sift1, num_pts1, d_sift2, num_pts2,
                       (const Match8Partial *)partials, n1_pad, splits);
  else if (splits > 1)
    hipLaunchKernelGGL(distance ? match8_merge_kernel<true> : match8_merge_kernel<false>, dim3(idiv_up(num_pts1, 256)),
                       dim3(256), 0, ctx->stream, d_sift1, num_pts1, d_sift2, num_pts2,
                       (const Match8Partial *)partials, n1_pad, splits);
  if (col_partials)
    hipLaunchKernelGGL(distance ? match8_mutual_merge_kernel<true> : match8_mutual_merge_kernel<false>,
                       dim3(idiv_up(num_pts2, 256)), dim3(256), 0, ctx->stream, d_back, num_pts2,
                       (const cusift_point *)d_sift1, num_pts1, (const Match8Partial *)col_partials, row_blocks);
  return check_launch(d_back ? "match8_mutual" : guide ? (guide->camera ? "match8_projected" : "match8_guided") : "match8");
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

// cusift_match8 where only the columns that pass the geometric test against a row count for it: cusift_match8's refusals,
// then cusift_match_guided's / cusift_match_projected's.
static int check_pair8(const char *who, const cusift_point *d_sift1, const unsigned char *d_q1, const int *d_sums1,
                       const cusift_point *d_sift2, const unsigned char *d_q2, const int *d_sums2, int distance) {
  if (!d_sift1 || !d_sift2) return fail(CUSIFT_ERR_INVALID, "%s: missing data", who);
  TRY(check_tables8(who, d_q1, d_sums1));
  TRY(check_tables8(who, d_q2, d_sums2));
  return check_distance(who, distance);
}

extern "C" int cusift_match8_guided(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const unsigned char *d_q1,
                                    const int *d_sums1, const cusift_point *d_sift2, int num_pts2,
                                    const unsigned char *d_q2, const int *d_sums2, int distance, int model,
                                    const double h_model[9], float radius) {
  TRY(enter(ctx));
  if (num_pts1 <= 0 || num_pts2 <= 0) return CUSIFT_OK;  // as cusift_match8: nothing to match
  TRY(check_pair8("Match8Guided", d_sift1, d_q1, d_sums1, d_sift2, d_q2, d_sums2, distance));
  TRY(check_guide("Match8Guided", model, h_model, radius));
  const GuideCall guide{model, radius * radius, h_model};
  return match8_launch(ctx, d_sift1, num_pts1, d_q1, d_sums1, d_sift2, num_pts2, d_q2, d_sums2, distance, nullptr, &guide);
}

extern "C" int cusift_match8_projected(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const unsigned char *d_q1,
                                       const int *d_sums1, const cusift_point *d_sift2, int num_pts2,
                                       const unsigned char *d_q2, const int *d_sums2, int distance, const double h_rt[12],
                                       const cusift_camera *camera2, float radius) {
  TRY(enter(ctx));
  if (num_pts1 <= 0 || num_pts2 <= 0) return CUSIFT_OK;  // as cusift_match8: nothing to match
  TRY(check_pair8("Match8Projected", d_sift1, d_q1, d_sums1, d_sift2, d_q2, d_sums2, distance));
  TRY(check_project("Match8Projected", h_rt, camera2, radius));
  const PnPCam cam = pnp_cam(camera2);
  const GuideCall guide{0, radius * radius, h_rt, &cam};
  return match8_launch(ctx, d_sift1, num_pts1, d_q1, d_sums1, d_sift2, num_pts2, d_q2, d_sums2, distance, nullptr, &guide);
}

// Uploads the pair list and enqueues the matcher of every pair: one launch, plus a merge when the columns are split and
// -- with d_rows_back, the column side -- one more when max_pts spans several row blocks.  *d_pairs_out: the list on the
// device.  guide != NULL (cusift_match8_batch_guided, cusift_match8_batch_projected, never with d_rows_back): the guided
// kernel over the frames' records d_points, its models -- GuideModel or ProjectModel [pair] -- uploaded behind the
// partials, and the none-aware merge.  n_pairs >= 1, max_pts >= 1, the arguments are checked.
int match8_batch_launch(cusift_ctx *ctx, const unsigned char *d_q, const int *d_sums, const unsigned int *d_counters,
                        int max_pts, const int *h_pairs, int n_pairs, int distance, cusift_match_row *d_rows,
                        cusift_match_row *d_rows_back, const int **d_pairs_out, const cusift_point *d_points = nullptr,
                        const GuideCall *guide = nullptr) {
  const int row_blocks = idiv_up(max_pts, kM8RowsPerBlock);
  int splits, cols_per_split;
  TRY(matcher_split_plan(ctx, guide ? kMatcher8Guided : kMatcher8, max_pts, max_pts, n_pairs, &splits, &cols_per_split));
  const int n1_pad = row_blocks * kM8RowsPerBlock;
  const size_t list_b = align_up_sz(sizeof(int) * 2 * (size_t)n_pairs, 256);
  const size_t part_b = splits > 1 ? sizeof(Match8Partial) * (size_t)n_pairs * splits * n1_pad : 0;
  const size_t col_b = d_rows_back && row_blocks > 1 ? sizeof(Match8Partial) * (size_t)n_pairs * row_blocks * max_pts : 0;
  const size_t model_at = align_up_sz(list_b + part_b + col_b, 256);
  const size_t model_b = guide ? (guide->camera ? sizeof(ProjectModel) : sizeof(GuideModel)) * (size_t)n_pairs : 0;
  TRY(grow_scratch(ctx, ctx->pairs_scratch, ctx->pairs_scratch_bytes, guide ? model_at + model_b : list_b + part_b + col_b,
                   "", false));
  int *d_pairs = (int *)ctx->pairs_scratch;
  Match8Partial *partials = splits > 1 ? (Match8Partial *)(ctx->pairs_scratch + list_b) : nullptr;
  Match8Partial *col_partials = col_b ? (Match8Partial *)(ctx->pairs_scratch + list_b + part_b) : nullptr;
  HIP_TRY(hipMemcpyAsync(d_pairs, h_pairs, sizeof(int) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice, ctx->stream));
  const dim3 grid(row_blocks, splits, n_pairs);
  if (d_rows_back)
    hipLaunchKernelGGL(distance ? match8_batch_mutual_kernel<true> : match8_batch_mutual_kernel<false>, grid, dim3(256), 0,
                       ctx->stream, d_q, d_sums, d_counters, max_pts, (const int *)d_pairs, cols_per_split, partials,
                       n1_pad, d_rows, col_partials, d_rows_back);
  else if (guide && guide->camera) {
    ProjectModel *d_models = (ProjectModel *)(ctx->pairs_scratch + model_at);
    ctx->project_models.resize(n_pairs);  // stays allocated behind this call, whenever the upload reads it
    for (int p = 0; p < n_pairs; ++p)
      ctx->project_models[p] = project_model(guide->h_models + 12 * (size_t)p, *guide->camera);
    HIP_TRY(hipMemcpyAsync(d_models, ctx->project_models.data(), model_b, hipMemcpyHostToDevice, ctx->stream));
    const auto kernel =
        distance ? match8_batch_guided_kernel<true, M8GuideP, ProjectModel> : match8_batch_guided_kernel<false, M8GuideP, ProjectModel>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, d_points, d_q, d_sums, d_counters, max_pts,
                       (const int *)d_pairs, cols_per_split, partials, n1_pad, d_rows, (const ProjectModel *)d_models,
                       guide->r2);
  } else if (guide) {
    // straight from the caller's array, as the pair list above: a copy from pageable memory is staged before
    // hipMemcpyAsync returns, which is what "read before the call returns" rests on (cusift_match_batch_guided does the
    // same).  The projected models are BUILT here, pose beside camera, so they need a home that outlives this frame.
    GuideModel *d_models = (GuideModel *)(ctx->pairs_scratch + model_at);
    HIP_TRY(hipMemcpyAsync(d_models, guide->h_models, model_b, hipMemcpyHostToDevice, ctx->stream));
    const auto kernel =
        guide->model == CUSIFT_GUIDE_EPIPOLAR
            ? (distance ? match8_batch_guided_kernel<true, M8GuideF, GuideModel> : match8_batch_guided_kernel<false, M8GuideF, GuideModel>)
            : (distance ? match8_batch_guided_kernel<true, M8GuideH, GuideModel> : match8_batch_guided_kernel<false, M8GuideH, GuideModel>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, d_points, d_q, d_sums, d_counters, max_pts,
                       (const int *)d_pairs, cols_per_split, partials, n1_pad, d_rows, (const GuideModel *)d_models,
                       guide->r2);
  } else
    hipLaunchKernelGGL(distance ? match8_batch_kernel<true> : match8_batch_kernel<false>, grid, dim3(256), 0, ctx->stream,
                       d_q, d_sums, d_counters, max_pts, (const int *)d_pairs, cols_per_split, partials, n1_pad, d_rows);
  if (splits > 1 && guide)
    hipLaunchKernelGGL(distance ? match8_batch_guided_merge_kernel<true> : match8_batch_guided_merge_kernel<false>,
                       dim3(idiv_up(max_pts, 256), n_pairs), dim3(256), 0, ctx->stream, d_counters, max_pts,
                       (const int *)d_pairs, cols_per_split, (const Match8Partial *)partials, n1_pad, splits, d_rows);
  else if (splits > 1)
    hipLaunchKernelGGL(distance ? match8_batch_merge_kernel<true> : match8_batch_merge_kernel<false>,
                       dim3(idiv_up(max_pts, 256), n_pairs), dim3(256), 0, ctx->stream, d_counters, max_pts,
                       (const int *)d_pairs, cols_per_split, (const Match8Partial *)partials, n1_pad, splits, d_rows);
  if (col_partials)
    hipLaunchKernelGGL(distance ? match8_batch_mutual_merge_kernel<true> : match8_batch_mutual_merge_kernel<false>,
                       dim3(idiv_up(max_pts, 256), n_pairs), dim3(256), 0, ctx->stream, d_counters, max_pts,
                       (const int *)d_pairs, (const Match8Partial *)col_partials, row_blocks, d_rows_back);
  if (d_pairs_out) *d_pairs_out = d_pairs;
  return check_launch(d_rows_back ? "match8_batch_mutual"
                      : guide     ? (guide->camera ? "match8_batch_projected" : "match8_batch_guided")
                                  : "match8_batch");
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

// cusift_match8_batch under one model per pair: the refusals of cusift_match_batch_guided / _projected -- a bad model or
// radius is refused with an empty list too -- then cusift_match8_batch's
extern "C" int cusift_match8_batch_guided(cusift_ctx *ctx, const cusift_point *d_points, const unsigned char *d_q,
                                          const int *d_sums, const unsigned int *d_counters, int n_images, int max_pts,
                                          const int *h_pairs, int n_pairs, int distance, int model,
                                          const double *h_models, float radius, cusift_match_row *d_rows) {
  TRY(enter(ctx));
  bool nothing;
  TRY(check_guide("Match8BatchGuided", model, h_models, radius));
  TRY(check_batch8("Match8BatchGuided", d_q, d_sums, n_images, max_pts, h_pairs, n_pairs, distance, d_rows, &nothing));
  if (nothing) return CUSIFT_OK;
  if (!d_points) return fail(CUSIFT_ERR_INVALID, "Match8BatchGuided: missing data");
  const GuideCall guide{model, radius * radius, h_models};
  return match8_batch_launch(ctx, d_q, d_sums, d_counters, max_pts, h_pairs, n_pairs, distance, d_rows, nullptr, nullptr,
                             d_points, &guide);
}

extern "C" int cusift_match8_batch_projected(cusift_ctx *ctx, const cusift_point *d_points, const unsigned char *d_q,
                                             const int *d_sums, const unsigned int *d_counters, int n_images, int max_pts,
                                             const int *h_pairs, int n_pairs, int distance, const double *h_rts,
                                             const cusift_camera *camera2, float radius, cusift_match_row *d_rows) {
  TRY(enter(ctx));
  bool nothing;
  TRY(check_project("Match8BatchProjected", h_rts, camera2, radius));
  TRY(check_batch8("Match8BatchProjected", d_q, d_sums, n_images, max_pts, h_pairs, n_pairs, distance, d_rows, &nothing));
  if (nothing) return CUSIFT_OK;
  if (!d_points) return fail(CUSIFT_ERR_INVALID, "Match8BatchProjected: missing data");
  const PnPCam cam = pnp_cam(camera2);
  const GuideCall guide{0, radius * radius, h_rts, &cam};
  return match8_batch_launch(ctx, d_q, d_sums, d_counters, max_pts, h_pairs, n_pairs, distance, d_rows, nullptr, nullptr,
                             d_points, &guide);
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

// cusift_quantize_descriptors of both record sets, then cusift_match8 -- d_back != NULL: cusift_match8_mutual; guide !=
// NULL: cusift_match8_guided or cusift_match8_projected.  Counts >= 1, the arguments are checked.
int match8_pair_enqueue(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2, int num_pts2,
                        int distance, cusift_point *d_back, const GuideCall *guide) {
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
  return match8_launch(ctx, d_sift1, num_pts1, q, sums, d_sift2, num_pts2, q2, sums2, distance, d_back, guide);
}

// The second matching pass of a registration staged on bytes: a caller with records alone.
// cusift_quantize_descriptors of both record sets into tables of the context's, then cusift_match8_guided /
// cusift_match8_projected on them: the same bytes, the fp32 guided calls' refusals.
extern "C" int cusift_match8_guided_records(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1,
                                            const cusift_point *d_sift2, int num_pts2, int distance, int model,
                                            const double h_model[9], float radius) {
  TRY(enter(ctx));
  if (num_pts1 <= 0 || num_pts2 <= 0) return CUSIFT_OK;  // as cusift_match_guided: nothing to match
  if (!d_sift1 || !d_sift2) return fail(CUSIFT_ERR_INVALID, "Match8GuidedRecords: missing data");
  TRY(check_distance("Match8GuidedRecords", distance));
  TRY(check_guide("Match8GuidedRecords", model, h_model, radius));
  const GuideCall guide{model, radius * radius, h_model};
  return match8_pair_enqueue(ctx, d_sift1, num_pts1, d_sift2, num_pts2, distance, nullptr, &guide);
}

extern "C" int cusift_match8_projected_records(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1,
                                               const cusift_point *d_sift2, int num_pts2, int distance,
                                               const double h_rt[12], const cusift_camera *camera2, float radius) {
  TRY(enter(ctx));
  if (num_pts1 <= 0 || num_pts2 <= 0) return CUSIFT_OK;  // as cusift_match_projected: nothing to match
  if (!d_sift1 || !d_sift2) return fail(CUSIFT_ERR_INVALID, "Match8ProjectedRecords: missing data");
  TRY(check_distance("Match8ProjectedRecords", distance));
  TRY(check_project("Match8ProjectedRecords", h_rt, camera2, radius));
  const PnPCam cam = pnp_cam(camera2);
  const GuideCall guide{0, radius * radius, h_rt, &cam};
  return match8_pair_enqueue(ctx, d_sift1, num_pts1, d_sift2, num_pts2, distance, nullptr, &guide);
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
