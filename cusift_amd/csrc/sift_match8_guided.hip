// sift_match8_guided.hip -- the int8 matcher under a geometric guide (cusift_match8_guided, cusift_match8_projected,
// cusift_match8_batch_guided, cusift_match8_batch_projected): sift_match8.hip's matcher from the same text (m8_block,
// sift_match8_block.h) -- the same grids, staging, LDS tiles and sinks -- with the predicate of the fp32 guided matchers in
// its update.  The definition, expression by expression, is in include/cusift_amd_extras.h; the launches are
// sift_match8.hip's (match8_launch, match8_batch_launch).
#include "sift_match8_block.h"

namespace cusift {

// ---- the geometric guides (cusift_match8_guided, cusift_match8_projected and their pair-list forms) -----------------------
// cusift_match8 with one more rule: a column whose coords2D fail the geometric test against a row enters that row's update
// as kM8Init, which changes nothing there (min leaves best alone, med3(best, second, kM8Init) is second, v < best is
// false).  The tests are those of the fp32 matchers, expression for expression -- GuideH / GuideF (sift_match.hip) and
// GuideP (sift_match_project.hip); the definition is in include/cusift_amd_extras.h -- and so is their split: per row fp64,
// evaluated once in front of the column loop, per (row, column) a handful of fp32 operations.  Here a wave has 64 rows and
// a lane 16 of them (16 i + 4 g + j): lane l evaluates row l of its wave and one round of 16 shuffles per float leaves
// every lane with the terms of its rows.  The coordinates come from the records, which the tables do not carry: the rows'
// from `sift1`, the columns' from `sift2` through a range-checked buffer load into bytes 136..143 of the LDS column, the
// pad behind its term -- no new LDS.  A column past the split's end reads (0, 0) there, which can pass a test, so "the
// column is real" stays in the update's condition.  A row that nothing passes ends the scan as (kM8Init, kM8Init, -1).
struct M8GuideColumns {
  static constexpr bool kOn = true;
  struct Column {
    float x, y;
  };
  const cusift_point *sift1, *sift2;  // the records of the rows and of the columns
  float r2;                           // radius * radius
  u2 staged;                          // threads 0..63: coords2D of column c0 + threadIdx.x of the tile in flight

  // the columns [col_begin, col_end) span less than 2^31 bytes of records (kMatcher8Guided, sift_host.h)
  __device__ __forceinline__ void fetch(int c0, int col_begin, int col_end) {
    if (threadIdx.x < kM8TileCols) {
      constexpr int kRec = (int)sizeof(cusift_point);
      const __amdgpu_buffer_rsrc_t rsrc =
          __builtin_amdgcn_make_buffer_rsrc((void *)(sift2 + col_begin), 0, (col_end - col_begin) * kRec, kBufFlags);
      staged = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)threadIdx.x * kRec + (int)offsetof(cusift_point, coords2D),
                                                    __builtin_amdgcn_readfirstlane((c0 - col_begin) * kRec), 0);
    }
  }
  __device__ __forceinline__ void store(unsigned char *buf) const {
    if (threadIdx.x < kM8TileCols) *reinterpret_cast<u2 *>(buf + threadIdx.x * kM8Stride + 136) = staged;
  }
  __device__ __forceinline__ Column column(const unsigned char *buf, int j) const {
    const f2 v = *reinterpret_cast<const f2 *>(buf + j * kM8Stride + 136);
    return Column{v[0], v[1]};
  }
  // the record of the row this lane evaluates (a row past n1 is a copy of the last one), and what the lane of this
  // lane's row 16 i + 4 g + j evaluated
  __device__ __forceinline__ const cusift_point *row(int n1, int p1_base, int lane) const {
    return sift1 + min(p1_base + lane, n1 - 1);
  }
  static __device__ __forceinline__ float from_row(float v, int lane, int i, int j) {
    return __shfl(v, 16 * i + 4 * (lane >> 4) + j);
  }
};

// x2 ~ H x1 (GuideH): the row's image (px, py), then |x2 - p|^2 < r2.  W == 0 gives an infinity or a NaN: no pass.
struct M8GuideH : M8GuideColumns {
  const double *m;
  float px[4][4], py[4][4];
  __device__ __forceinline__ void model(const GuideModel *k) { m = k->m; }
  __device__ __forceinline__ void rows(int n1, int p1_base, int lane) {
    const float *xy = row(n1, p1_base, lane)->coords2D;
    const double x1 = xy[0], y1 = xy[1];
    const double X = (m[0] * x1 + m[1] * y1) + m[2];
    const double Y = (m[3] * x1 + m[4] * y1) + m[5];
    const double W = (m[6] * x1 + m[7] * y1) + m[8];
    const float x = (float)(X / W), y = (float)(Y / W);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        px[i][j] = from_row(x, lane, i, j);
        py[i][j] = from_row(y, lane, i, j);
      }
  }
  __device__ __forceinline__ bool pass(int i, int j, Column c) const {
    const float dx = c.x - px[i][j], dy = c.y - py[i][j];
    return dx * dx + dy * dy < r2;
  }
};

// x2^T F x1 = 0 (GuideF): the row's epipolar line scaled to a unit normal (a, b, c), then (a x2 + b y2 + c)^2 < r2.  A
// line whose normal has length 0 or that is not finite is three NaNs: no pass for the whole row.
struct M8GuideF : M8GuideColumns {
  const double *m;
  float a[4][4], b[4][4], c[4][4];
  __device__ __forceinline__ void model(const GuideModel *k) { m = k->m; }
  __device__ __forceinline__ void rows(int n1, int p1_base, int lane) {
    const float *xy = row(n1, p1_base, lane)->coords2D;
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
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[i][j] = from_row(la, lane, i, j);
        b[i][j] = from_row(lb, lane, i, j);
        c[i][j] = from_row(lc, lane, i, j);
      }
  }
  __device__ __forceinline__ bool pass(int i, int j, Column p) const {
    const float d = (a[i][j] * p.x + b[i][j] * p.y) + c[i][j];
    return d * d < r2;
  }
};

// X1 = R X2 + t (GuideP): the row's coords3D in camera 2's frame (a, b, c), its pixel (px, py), then M8GuideH's test.  A
// row without depth (Z == 0), behind camera 2 or on its principal plane (c <= 0, or a NaN) is two NaNs: no pass for the
// whole row.
struct M8GuideP : M8GuideColumns {
  const ProjectModel *k;
  float px[4][4], py[4][4];
  __device__ __forceinline__ void model(const ProjectModel *k_) { k = k_; }
  __device__ __forceinline__ void rows(int n1, int p1_base, int lane) {
    const float *X1 = row(n1, p1_base, lane)->coords3D;
    const double X = X1[0], Y = X1[1], Z = X1[2];
    const double *rt = k->rt;
    const double dx = X - rt[3], dy = Y - rt[7], dz = Z - rt[11];
    const double a = (rt[0] * dx + rt[4] * dy) + rt[8] * dz;
    const double b = (rt[1] * dx + rt[5] * dy) + rt[9] * dz;
    const double c = (rt[2] * dx + rt[6] * dy) + rt[10] * dz;
    const bool usable = Z != 0.0 && c > 0.0;
    const float kNaN = __builtin_nanf("");
    const float x = usable ? (float)((k->fx * a) / c + k->px) : kNaN;
    const float y = usable ? (float)((k->fy * b) / c + k->py) : kNaN;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        px[i][j] = from_row(x, lane, i, j);
        py[i][j] = from_row(y, lane, i, j);
      }
  }
  __device__ __forceinline__ bool pass(int i, int j, Column c) const {
    const float dx = c.x - px[i][j], dy = c.y - py[i][j];
    return dx * dx + dy * dy < r2;
  }
};

// ---- under a guide --------------------------------------------------------------------------------------------------------
// match8_kernel under Guide: the model is a kernel argument.  The sinks and the merges are the none-aware ones: a row that
// nothing passes, in a split or in all of them, is (kM8Init, kM8Init, -1) and is written as cusift_match's initial values.
// __launch_bounds__(256, 2): the guides keep 32 (H, P) or 48 (F) registers of per-row terms on top of m8_block's, and
// without the second argument F compiles to 248 VGPRs + 12 AGPRs -- past 256, one wave per SIMD.  With it: 218 / 234, two.
template <bool kL2, class Guide, class Model>
__global__ void __launch_bounds__(256, 2) match8_guided_kernel(cusift_point *__restrict__ sift1, int n1,
                                                           const unsigned char *__restrict__ q1,
                                                           const int *__restrict__ sums1,
                                                           const cusift_point *__restrict__ sift2, int n2,
                                                           const unsigned char *__restrict__ q2,
                                                           const int *__restrict__ sums2, int cols_per_split,
                                                           Match8Partial *__restrict__ partials, int n1_pad,
                                                           Model model, float r2) {
  __shared__ __attribute__((aligned(16))) unsigned char sB[2 * kM8TileCols * kM8Stride];
  const int col_begin = blockIdx.y * cols_per_split;
  const int col_end = min(col_begin + cols_per_split, n2);
  if (col_begin >= col_end) return;  // uniform; the host sizes the splits so that this never happens
  Guide guide;
  guide.sift1 = sift1;
  guide.sift2 = sift2;
  guide.r2 = r2;
  guide.model(&model);
  m8_block<kL2>(q1, sums1, n1, q2, sums2, col_begin, col_end, sB,
                m8_point_sink<kL2, true>(partials, (size_t)blockIdx.y * n1_pad, sift1, sift2, n2), M8NoCols{}, guide);
}

template <bool kL2>
__global__ void __launch_bounds__(256) match8_guided_merge_kernel(cusift_point *__restrict__ sift1, int n1,
                                                                 const cusift_point *__restrict__ sift2, int n2,
                                                                 const Match8Partial *__restrict__ partials, int n1_pad,
                                                                 int n_splits) {
  const int p1 = blockIdx.x * 256 + threadIdx.x;
  if (p1 >= n1) return;
  const Match8Partial m = fold_partials(partials + p1, n1_pad, n_splits, M8Merge{});
  m8_write_point<kL2, true>(sift1 + p1, sift2, n2, m.best, m.second, m.idx);
}

// match8_batch_kernel under Guide: pair blockIdx.z's model from models[pair] (a device copy of the caller's array), the
// coordinates from the frames' records in `points`
template <bool kL2, class Guide, class Model>
__global__ void __launch_bounds__(256, 2) match8_batch_guided_kernel(const cusift_point *__restrict__ points,
                                                                 const unsigned char *__restrict__ q,
                                                                 const int *__restrict__ sums,
                                                                 const unsigned int *__restrict__ counters, int max_pts,
                                                                 const int *__restrict__ pairs, int cols_per_split,
                                                                 Match8Partial *__restrict__ partials, int n1_pad,
                                                                 cusift_match_row *__restrict__ rows,
                                                                 const Model *__restrict__ models,
                                                                 float r2) {
  __shared__ __attribute__((aligned(16))) unsigned char sB[2 * kM8TileCols * kM8Stride];
  const PairFrame fr(counters, pairs, max_pts, cols_per_split, kM8RowsPerBlock);
  if (fr.empty) return;
  Guide guide;
  guide.sift1 = points + (size_t)fr.f1 * max_pts;
  guide.sift2 = points + (size_t)fr.f2 * max_pts;
  guide.r2 = r2;
  guide.model(models + fr.pair);
  m8_block<kL2>(q + (size_t)fr.f1 * max_pts * 128, sums + (size_t)fr.f1 * max_pts * 2, fr.n1,
                q + (size_t)fr.f2 * max_pts * 128, sums + (size_t)fr.f2 * max_pts * 2, fr.col_begin, fr.col_end, sB,
                m8_row_sink<kL2, true>(partials, ((size_t)fr.pair * gridDim.y + blockIdx.y) * n1_pad,
                                       rows + (size_t)fr.pair * max_pts),
                M8NoCols{}, guide);
}

template <bool kL2>
__global__ void __launch_bounds__(256) match8_batch_guided_merge_kernel(const unsigned int *__restrict__ counters,
                                                                       int max_pts, const int *__restrict__ pairs,
                                                                       int cols_per_split,
                                                                       const Match8Partial *__restrict__ partials,
                                                                       int n1_pad, int n_splits,
                                                                       cusift_match_row *__restrict__ rows) {
  const PairCounts pc(blockIdx.y, counters, pairs, max_pts);
  const int p1 = blockIdx.x * 256 + threadIdx.x;
  if (p1 >= pc.n1 || pc.n2 <= 0) return;
  const int live = min(n_splits, (pc.n2 + cols_per_split - 1) / cols_per_split);  // the others wrote nothing
  const Match8Partial m = fold_partials(partials + (size_t)pc.pair * n_splits * n1_pad + p1, n1_pad, live, M8Merge{});
  m8_write_row<kL2, true>(rows + (size_t)pc.pair * max_pts + p1, m.best, m.second, m.idx);
}

#define CUSIFT_GUIDED8_KERNELS(kL2, Guide, Model)                                                                        \
  template __global__ void match8_guided_kernel<kL2, Guide, Model>(                                                       \
      cusift_point *, int, const unsigned char *, const int *, const cusift_point *, int, const unsigned char *,          \
      const int *, int, Match8Partial *, int, Model, float);                                                              \
  template __global__ void match8_batch_guided_kernel<kL2, Guide, Model>(                                                 \
      const cusift_point *, const unsigned char *, const int *, const unsigned int *, int, const int *, int,              \
      Match8Partial *, int, cusift_match_row *, const Model *, float);
#define CUSIFT_GUIDED8_MERGES(kL2)                                                                                       \
  template __global__ void match8_guided_merge_kernel<kL2>(cusift_point *, int, const cusift_point *, int,                \
                                                           const Match8Partial *, int, int);                              \
  template __global__ void match8_batch_guided_merge_kernel<kL2>(const unsigned int *, int, const int *, int,             \
                                                                 const Match8Partial *, int, int, cusift_match_row *);
CUSIFT_GUIDED8_KERNELS(false, M8GuideH, GuideModel)
CUSIFT_GUIDED8_KERNELS(true, M8GuideH, GuideModel)
CUSIFT_GUIDED8_KERNELS(false, M8GuideF, GuideModel)
CUSIFT_GUIDED8_KERNELS(true, M8GuideF, GuideModel)
CUSIFT_GUIDED8_KERNELS(false, M8GuideP, ProjectModel)
CUSIFT_GUIDED8_KERNELS(true, M8GuideP, ProjectModel)
CUSIFT_GUIDED8_MERGES(false)
CUSIFT_GUIDED8_MERGES(true)
#undef CUSIFT_GUIDED8_KERNELS
#undef CUSIFT_GUIDED8_MERGES

}  // namespace cusift
