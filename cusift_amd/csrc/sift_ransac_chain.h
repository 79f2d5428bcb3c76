// sift_ransac_chain.h -- the bodies that the kernels of the homography, fundamental-matrix and PnP chains share
// (sift_planar.hip, sift_epipolar.hip, sift_pnp.hip, sift_sequence.hip): mark, gather + draw, null vector, score.  The
// host runs the three models as one chain told apart by data (RansacModel, sift_register.hip); here each kernel is a thin
// wrapper that names its model.  Inline templates only: the LDS arrays stay declared in the kernels and are passed in.
// The build contracts nothing (-ffp-contract=off), so an expression gives the same bits wherever it stands.
#pragma once

#include "sift_ransac.h"

namespace cusift {

constexpr int kRansacTile = 64;  // hypotheses per workgroup of the solve and scoring kernels (one per lane), points per LDS tile

// ---- marking ---------------------------------------------------------------------------------------------------------
// The mark byte of a record (planar_marks) from its coordinates: all four finite and -- kDepth, the PnP chain -- three
// finite coords3D floats with Z != 0.  valid: the partner exists; mutual: it names this record (read when has_cross).
template <bool kDepth>
__device__ __forceinline__ unsigned char mark_record(int rule, float score, float amb, float lo, float hi, float x1,
                                                     float y1, float x2, float y2, float X, float Y, float Z, bool valid,
                                                     bool has_cross, bool mutual) {
  bool finite = planar_finite(x1) && planar_finite(y1) && planar_finite(x2) && planar_finite(y2);
  if (kDepth) finite = finite && planar_finite(X) && planar_finite(Y) && planar_finite(Z) && Z != 0.0f;
  return planar_marks(rule, score, amb, lo, hi, finite, valid, has_cross, mutual);
}

// Record i's column of the SoA coordinate rows, `stride` floats apart: [x1 | y1 | x2 | y2], kDepth [X | Y | Z | x2 | y2].
template <bool kDepth>
__device__ __forceinline__ void write_coord_rows(float *__restrict__ coord, int stride, int i, float x1, float y1, float x2,
                                                 float y2, float X, float Y, float Z) {
  coord[i] = kDepth ? X : x1;
  coord[i + stride] = kDepth ? Y : y1;
  coord[i + 2 * (size_t)stride] = kDepth ? Z : x2;
  coord[i + 3 * (size_t)stride] = kDepth ? x2 : y2;
  if (kDepth) coord[i + 4 * (size_t)stride] = y2;
}

// planar_mark_kernel and pnp_mark_kernel (kDepth): the marking of a pair call's records from their own match fields.
// coord [4 or 5][num_pts], marks [num_pts], block_counts [ceil(num_pts / 256)]: the candidates of each 256-record
// workgroup.  pts2 != NULL (cusift_ctx_set_cross_check): the num_pts2 records of image 2 with cusift_match_mutual's
// fields; a record that is not its partner's match is neither a candidate nor in the refit set, under either rule.
// s_wave [4].
template <bool kDepth>
__device__ __forceinline__ void pair_mark(const cusift_point *__restrict__ pts, int num_pts, int num_pts2, int rule,
                                          float lo, float hi, float *__restrict__ coord,
                                          unsigned char *__restrict__ marks, int *__restrict__ block_counts,
                                          PlanarBatch nb, const cusift_point *__restrict__ pts2, int *s_wave) {
  pts += (size_t)blockIdx.z * nb.records;
  coord = pair_ptr(coord, nb.scratch), marks = pair_ptr(marks, nb.scratch);
  block_counts = pair_ptr(block_counts, nb.scratch);
  const int tx = threadIdx.x;
  const int i = blockIdx.x * kRansacThreads + tx;
  bool cand = false;
  if (i < num_pts) {
    const cusift_point *p = pts + i;
    const float x1 = p->coords2D[0], y1 = p->coords2D[1], x2 = p->match_xpos, y2 = p->match_ypos;
    float X = 0.0f, Y = 0.0f, Z = 0.0f;
    if (kDepth) X = p->coords3D[0], Y = p->coords3D[1], Z = p->coords3D[2];
    const float score = p->score, amb = p->ambiguity;
    const int m = p->match;
    write_coord_rows<kDepth>(coord, num_pts, i, x1, y1, x2, y2, X, Y, Z);
    const bool inside = m >= 0 && m < num_pts2;
    // the cross-check: the partner's own match (cusift_match_mutual's column side) must name record i
    const bool mutual = pts2 && inside && pts2[m].match == i;
    const unsigned char mk = mark_record<kDepth>(rule, score, amb, lo, hi, x1, y1, x2, y2, X, Y, Z,
                                                 num_pts2 < 0 || inside, pts2 != nullptr, mutual);
    marks[i] = mk;
    cand = mk & 1;
  }
  const int keeps = keep_count_256(cand, s_wave);
  if (tx == 0) block_counts[blockIdx.x] = keeps;
}

// ---- solving ---------------------------------------------------------------------------------------------------------
// The front of epipolar_solve_kernel and pnp_solve_kernel.  The launch's threads together gather the candidates'
// coordinates into ccoord [kRows][num_pts], candidate k at column k, which is all the scoring and the refit read; then
// hypothesis idx (one per lane) draws its N samples from the candidate list, pair p from seed + p, leaves their record
// indices in drawn [N][num_loops] and rec, and zeroes counts[idx] for the scoring kernel.  coord and model come back as
// the pair's own.  false: fewer than N candidates (uniform: nothing is done) or a lane past the last hypothesis -- two
// exits, so that the first stays a scalar branch.
template <int N, int kRows>
__device__ __forceinline__ bool draw_and_gather(const float *__restrict__ &coord, int num_pts,
                                                const int *__restrict__ cand, const int *__restrict__ head,
                                                unsigned long long seed, int num_loops, int *__restrict__ drawn,
                                                double *__restrict__ &model, int *__restrict__ counts,
                                                float *__restrict__ ccoord, PlanarBatch nb, int &idx, int (&rec)[N]) {
  coord = pair_ptr(coord, nb.scratch), cand = pair_ptr(cand, nb.scratch);
  drawn = pair_ptr(drawn, nb.scratch), model = pair_ptr(model, nb.scratch);
  counts = pair_ptr(counts, nb.scratch), ccoord = pair_ptr(ccoord, nb.scratch);
  head = pair_ptr(head, nb.head);
  const int tx = threadIdx.x;
  const int n = min(head[kPlanarHeadCand], pair_count(head, num_pts, nb));
  if (n < N) return false;  // uniform
  // the launch's threads together: candidate k's coordinates to column k (k < n <= num_pts)
  for (int k = blockIdx.x * kRansacTile + tx; k < n; k += gridDim.x * kRansacTile) {
    const int r = clampi(cand[k], 0, num_pts - 1);  // memory safety only: the list holds record indices
#pragma unroll
    for (int c = 0; c < kRows; ++c) ccoord[(size_t)c * num_pts + k] = coord[(size_t)c * num_pts + r];
  }
  idx = blockIdx.x * kRansacTile + tx;
  if (idx >= num_loops) return false;  // no barrier below: every thread touches only its own LDS column
  int p[N];  // positions in the candidate list
  seed += blockIdx.z;  // 64-bit and wrapping
  ransac_sample<N>(seed, idx, n, p);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    rec[i] = clampi(cand[p[i]], 0, num_pts - 1);
    drawn[(size_t)i * num_loops + idx] = rec[i];
  }
  counts[idx] = 0;
  return true;
}

// Lane tx's linear system in LDS, one column of the array per lane: the pivot search indexes it dynamically, and
// consecutive lanes are consecutive doubles, so every access is conflict-free.
template <int kCols>
struct LaneSystem {
  double *m;
  int tx;
  __device__ __forceinline__ double &operator()(int i, int j) const { return m[(i * kCols + j) * kRansacTile + tx]; }
};

// The null vector x of lane tx's kRows x kCols system M, kCols = kRows + 1: Gaussian elimination with complete pivoting
// (rows and columns), back substitution from x[kCols - 1] = 1 with static indices.  Exact rank kRows has a
// one-dimensional null space, and nothing squares the condition number as a normal matrix would.  A pivot of 0 or NaN
// divides into something not finite, which the caller's finish turns into zeros.  s_col [kCols][kRansacTile]: the column
// permutation of the pivoting.  M is destroyed.
template <int kRows, int kCols>
__device__ __forceinline__ void null_vector(const LaneSystem<kCols> M, int *s_col, double (&out)[kCols]) {
  const auto COL = [&](int j) -> int & { return s_col[j * kRansacTile + M.tx]; };
#pragma unroll
  for (int j = 0; j < kCols; ++j) COL(j) = j;
#pragma unroll 1
  for (int k = 0; k < kRows; ++k) {
    double big = -1.0;
    int pi = k, pj = k;
    for (int i = k; i < kRows; ++i)
      for (int j = k; j < kCols; ++j) {
        const double t = fabs(M(i, j));
        const bool more = t > big;
        big = more ? t : big;
        pi = more ? i : pi;
        pj = more ? j : pj;
      }
    for (int j = k; j < kCols; ++j) {  // rows k and pi, from column k on (in front of it the rows are done with)
      const double a = M(k, j), b = M(pi, j);
      M(k, j) = b, M(pi, j) = a;
    }
    for (int i = 0; i < kRows; ++i) {  // columns k and pj, in every row: the rows above belong to the triangle
      const double a = M(i, k), b = M(i, pj);
      M(i, k) = b, M(i, pj) = a;
    }
    const int ck = COL(k), cj = COL(pj);
    COL(k) = cj, COL(pj) = ck;
    const double piv = M(k, k);
    for (int i = k + 1; i < kRows; ++i) {
      const double f = M(i, k) / piv;
      for (int j = k + 1; j < kCols; ++j) M(i, j) -= f * M(k, j);
    }
  }
  // back through the column permutation by way of row 0 of the system, which nothing reads any more once x is complete
  double x[kCols];
  x[kCols - 1] = 1.0;
#pragma unroll
  for (int k = kRows - 1; k >= 0; --k) {
    double s = 0.0;
#pragma unroll
    for (int j = k + 1; j < kCols; ++j) s += M(k, j) * x[j];
    x[k] = -s / M(k, k);
  }
  int col[kCols];
#pragma unroll
  for (int j = 0; j < kCols; ++j) col[j] = clampi(COL(j), 0, kCols - 1);
#pragma unroll
  for (int j = 0; j < kCols; ++j) M(0, col[j]) = x[j];
#pragma unroll
  for (int j = 0; j < kCols; ++j) out[j] = M(0, j);
}

// ---- scoring ---------------------------------------------------------------------------------------------------------
// The scoring kernel of every model.  blockIdx.x: 64 hypotheses, one per lane, its kValues numbers (as doubles) and its
// count in registers; a lane past the end scores a copy and drops the result.  blockIdx.y: the points [y * per_split,
// (y + 1) * per_split) -- the splits are sized from the capacity num_pts, and one that lies past the walk's end adds
// nothing.  The points pass through LDS in 64-point tiles, SoA rows of doubles: every lane reads the same point (a
// broadcast).  The splits' partial counts meet in one integer atomic add per lane (order-free); counts were zeroed by the
// solve kernel.  Fewer candidates than the model fits: nothing was solved, the select kernel answers alone.
// Model: kValues, kRows (coordinate rows), kMin, kUnroll (of the broadcast walk), kCandidates (the walk runs over the
// compacted candidates, not over all records), value_t (of the stored hypotheses), stage(s_pt, coord, num_pts, tile, tx)
// (column tx of a tile into LDS) and inlier(hypothesis, s_pt, j).  s_pt [kRows][kRansacTile].
template <int kRows>
__device__ __forceinline__ void stage_rows(double (*s_pt)[kRansacTile], const float *__restrict__ coord, int num_pts,
                                           int tile, int tx) {  // the staging of a model that takes the rows as they are
#pragma unroll
  for (int c = 0; c < kRows; ++c) s_pt[c][tx] = (double)coord[(size_t)c * num_pts + tile + tx];
}

template <class Model>
__device__ __forceinline__ void ransac_score(const Model model, const float *__restrict__ coord, int num_pts,
                                             int per_split, const typename Model::value_t *__restrict__ hyp,
                                             int num_loops, int *__restrict__ counts, const int *__restrict__ head,
                                             PlanarBatch nb, double (*s_pt)[kRansacTile]) {
  coord = pair_ptr(coord, nb.scratch), hyp = pair_ptr(hyp, nb.scratch);
  counts = pair_ptr(counts, nb.scratch), head = pair_ptr(head, nb.head);
  const int n_pts = pair_count(head, num_pts, nb);
  const int n_cand = min(head[kPlanarHeadCand], n_pts);
  if (n_cand < Model::kMin) return;  // uniform
  const int tx = threadIdx.x;
  const int loop = blockIdx.x * kRansacTile + tx;
  const int src = loop < num_loops ? loop : num_loops - 1;
  double v[Model::kValues];
#pragma unroll
  for (int i = 0; i < Model::kValues; ++i) v[i] = (double)hyp[(size_t)i * num_loops + src];
  const int begin = blockIdx.y * per_split;
  const int end = min(Model::kCandidates ? n_cand : n_pts, begin + per_split);
  int cnt = 0;
  for (int tile = begin; tile < end; tile += kRansacTile) {
    const int n = min(kRansacTile, end - tile);
    __syncthreads();
    if (tx < n) model.stage(s_pt, coord, num_pts, tile, tx);
    __syncthreads();
#pragma unroll Model::kUnroll
    for (int j = 0; j < n; ++j) cnt += model.inlier(v, s_pt, j) ? 1 : 0;
  }
  if (loop < num_loops && cnt) atomicAdd(&counts[loop], cnt);
}

// ---- the refits' small solve -------------------------------------------------------------------------------------------
// A x = b for a symmetric A whose lower triangle is read, by Cholesky: A = L L^T, L y = b, L^T x = y, fully unrolled so
// that every index is static.  Element (i, j) of L subtracts its products in ascending k, whatever order the elements
// are visited in.  false: a pivot is not > 0 (NaN included) -- x is then not to be used.
template <int N>
__device__ __forceinline__ bool cholesky_lower(const double (&A)[N][N], const double (&b)[N], double (&x)[N]) {
  double L[N][N], y[N];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      if (i == j) {
        ok = ok && (s > 0.0);
        L[i][i] = sqrt(s);
      } else {
        L[i][j] = s / L[j][j];
      }
    }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double s = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < N; ++k) s -= L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
  return ok;
}

}  // namespace cusift
