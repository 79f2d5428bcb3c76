// sift_epipolar.hip -- epipolar registration on the device: from matched SiftData to a refined fundamental matrix without
// a host decision.  The reference has no fundamental-matrix code: the definition is this library's own, written out in
// include/cusift_amd_extras.h, and all of it is fp64.  cusift_estimate_fundamental / cusift_register_epipolar enqueue, on
// the context's stream, with no host round trip in between:
//
//   planar_mark_kernel      (sift_planar.hip, unchanged) candidate?  SoA coordinates [x1 | y1 | x2 | y2] of all records
//   planar_compact_kernel   (sift_planar.hip, unchanged) the candidates' record indices in ascending order, their number
//   epipolar_solve_kernel   one hypothesis per lane: draw_and_gather (sift_ransac_chain.h: the candidates' coordinates
//                           compacted, eight samples drawn from the candidate list), Hartley normalisation, the
//                           null_vector of the 8 x 9 system, rank 2, denormalisation, unit norm and sign
//   epipolar_score_kernel   ransac_score (sift_ransac_chain.h) over the candidates with epipolar_inlier; grid (loops /
//                           64, candidate splits)
//   epipolar_select_kernel  one workgroup: the winner (ransac_winner<true>: among equals the first), its
//                           inlier flags, the refit rounds (normalised 9 x 9 sums over the current inliers, cyclic Jacobi,
//                           rank 2), then match_error of every record and the number of candidates that fit
// Every kernel has a pair index, blockIdx.z, and PlanarBatch's strides; one pair is gridDim.z == 1 with every stride 0.
//
// CANDIDATES ONLY.  Counts, flags, the refit set and num_fit run over the candidates, not over all records as the planar
// path does: the epipolar constraint is one-dimensional, so a rejected match lies within a pixel of a random epipolar
// line far more often than within a pixel of a homography's image of its point.  The scoring's cost follows n_cand.
//
// THE NULL VECTOR of the 8 x 9 system is null_vector's (sift_ransac_chain.h): Gaussian elimination with complete
// pivoting in LDS, about 500 flops; everything else is in registers with static indices.  The refit's 9 x 9 matrix is a sum
// over many points: there the eigenvector of the smallest eigenvalue is taken by cyclic Jacobi, kEpiSweeps9 sweeps over
// the 36 pairs in row-major order, whatever the data.  RANK 2: F' = F (I - v v^T) with v the eigenvector of the smallest
// eigenvalue of F^T F (3 x 3 cyclic Jacobi, kEpiSweeps3 sweeps) -- the nearest rank-2 matrix in the Frobenius norm.
// The partial sums of the refit are reduced in a fixed order (wave_tree_sum of sift_ransac.h), so every run gives the
// same bits.  Kernels use no scratch memory and write with vector stores only.
// The pinned inlier test and the Jacobi live in sift_epipolar.h: sift_pose.hip, the stage behind the selection, shares them.
// COST (profiles/epipolar.json, 10,000 loops): solve 42 us, scoring 58 us at 4,096 candidates and 511 us at 32,768, select
// 819 us and 1,580 us.  The select kernel carries the call: every refit round ends in one lane's Jacobi (288 rotations,
// each two divisions and two square roots in fp64, 126 doubles of state that overflow into AGPRs) while 255 lanes wait.
#include "sift_epipolar.h"
#include "sift_ransac_chain.h"

namespace cusift {

constexpr int kEpiThreads = 256;  // select
constexpr int kEpiTile = 64;      // hypotheses per workgroup of the solve and scoring kernels, candidates per LDS tile
static_assert(kEpiTile == kRansacTile && kEpiThreads == kRansacThreads, "the shared bodies' geometry");
constexpr int kEpiSums = 45;      // the upper triangle of the 9 x 9 normal matrix

// Column of v that belongs to the smallest a[j][j]; among equals the first.
template <int N>
__device__ __forceinline__ void epipolar_smallest(const double (&a)[N][N], const double (&v)[N][N], double (&x)[N]) {
  double best = a[0][0];
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] = v[i][0];
#pragma unroll
  for (int j = 1; j < N; ++j) {
    const bool take = a[j][j] < best;
    best = take ? a[j][j] : best;
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = take ? v[i][j] : x[i];
  }
}

// A Hartley normalisation x~ = (x - cx) * s of one image.
struct EpiNorm {
  double cx, cy, s;
};

// From the null vector fh of the normalised system to F: rank 2, F = T2^T F^ T1, Frobenius norm 1, the largest-magnitude
// entry positive (the first in row-major order among equals).  false: the result is not finite or all zero, F is nine
// zeros.
__device__ __forceinline__ bool epipolar_finish(const double (&fh)[9], EpiNorm n1, EpiNorm n2, double (&F)[9]) {
  // rank 2: remove the right singular vector of the smallest singular value
  double g[3][3], v[3][3], w[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) g[i][j] = (fh[i] * fh[j] + fh[3 + i] * fh[3 + j]) + fh[6 + i] * fh[6 + j];
  epipolar_jacobi<3>(g, v, kEpiSweeps3);
  epipolar_smallest<3>(g, v, w);
  double r[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double d = (fh[3 * i] * w[0] + fh[3 * i + 1] * w[1]) + fh[3 * i + 2] * w[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) r[3 * i + j] = fh[3 * i + j] - d * w[j];
  }
  // B = F^ T1, then F = T2^T B
  const double tx1 = -(n1.s * n1.cx), ty1 = -(n1.s * n1.cy), tx2 = -(n2.s * n2.cx), ty2 = -(n2.s * n2.cy);
  double b[9];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    b[3 * i] = r[3 * i] * n1.s;
    b[3 * i + 1] = r[3 * i + 1] * n1.s;
    b[3 * i + 2] = (r[3 * i] * tx1 + r[3 * i + 1] * ty1) + r[3 * i + 2];
  }
  double f[9];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    f[j] = n2.s * b[j];
    f[3 + j] = n2.s * b[3 + j];
    f[6 + j] = (tx2 * b[j] + ty2 * b[3 + j]) + b[6 + j];
  }
  double sq = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) sq += f[i] * f[i];
  const double norm = sqrt(sq);
  const bool ok = norm > 0.0 && norm < __builtin_inf();  // NaN fails both
  double big = -1.0;
  bool neg = false;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    f[i] = f[i] / norm;
    const bool more = fabs(f[i]) > big;
    big = more ? fabs(f[i]) : big;
    neg = more ? f[i] < 0.0 : neg;
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) F[i] = ok ? (neg ? -f[i] : f[i]) : 0.0;
  return ok;
}

// drawn [8][num_loops] (record indices), fund [9][num_loops], counts [num_loops] (zeroed here for the scoring kernel),
// ccoord [4][num_pts]: the coordinates of candidate k at column k.  Fewer than 8 candidates: nothing is done.
__global__ void __launch_bounds__(kEpiTile) epipolar_solve_kernel(const float *__restrict__ coord, int num_pts,
                                                                  const int *__restrict__ cand,
                                                                  const int *__restrict__ head, unsigned long long seed,
                                                                  int num_loops, int *__restrict__ drawn,
                                                                  double *__restrict__ fund, int *__restrict__ counts,
                                                                  float *__restrict__ ccoord, PlanarBatch nb) {
  __shared__ double s_m[72 * kEpiTile];  // the 8 x 9 system, one column of the array per lane
  __shared__ int s_col[9 * kEpiTile];    // the column permutation of the pivoting
  int idx, rec[8];
  if (!draw_and_gather<8, 4>(coord, num_pts, cand, head, seed, num_loops, drawn, fund, counts, ccoord, nb, idx, rec)) return;
  double x1[8], y1[8], x2[8], y2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = rec[i];
    x1[i] = (double)coord[r], y1[i] = (double)coord[(size_t)num_pts + r];
    x2[i] = (double)coord[2 * (size_t)num_pts + r], y2[i] = (double)coord[3 * (size_t)num_pts + r];
  }
  // Hartley: centroid to 0, mean distance sqrt(2), per image
  EpiNorm n1, n2;
  {
    double sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) sx1 += x1[i], sy1 += y1[i], sx2 += x2[i], sy2 += y2[i];
    n1.cx = sx1 / 8.0, n1.cy = sy1 / 8.0, n2.cx = sx2 / 8.0, n2.cy = sy2 / 8.0;
    double d1 = 0.0, d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const double ax = x1[i] - n1.cx, ay = y1[i] - n1.cy, bx = x2[i] - n2.cx, by = y2[i] - n2.cy;
      d1 += sqrt(ax * ax + ay * ay);
      d2 += sqrt(bx * bx + by * by);
    }
    n1.s = sqrt(2.0) / (d1 / 8.0), n2.s = sqrt(2.0) / (d2 / 8.0);
  }
  const LaneSystem<9> M{s_m, (int)threadIdx.x};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const double u1 = (x1[i] - n1.cx) * n1.s, v1 = (y1[i] - n1.cy) * n1.s;
    const double u2 = (x2[i] - n2.cx) * n2.s, v2 = (y2[i] - n2.cy) * n2.s;
    M(i, 0) = u2 * u1, M(i, 1) = u2 * v1, M(i, 2) = u2;
    M(i, 3) = v2 * u1, M(i, 4) = v2 * v1, M(i, 5) = v2;
    M(i, 6) = u1, M(i, 7) = v1, M(i, 8) = 1.0;
  }
  double fh[9], F[9];
  null_vector<8, 9>(M, s_col, fh);
  epipolar_finish(fh, n1, n2, F);
#pragma unroll
  for (int i = 0; i < 9; ++i) fund[(size_t)i * num_loops + idx] = F[i];
}

// ransac_score's model (sift_ransac_chain.h): 9 doubles per hypothesis, counted over the candidates.
struct EpipolarScore {
  static constexpr int kValues = 9, kRows = 4, kMin = 8, kUnroll = 4;
  static constexpr bool kCandidates = true;
  typedef double value_t;
  double t2;
  __device__ __forceinline__ void stage(double (*s_pt)[kEpiTile], const float *__restrict__ coord, int num_pts, int tile,
                                        int tx) const {
    stage_rows<4>(s_pt, coord, num_pts, tile, tx);
  }
  __device__ __forceinline__ bool inlier(const double (&F)[9], const double (*p)[kEpiTile], int j) const {
    return epipolar_inlier(F, p[0][j], p[1][j], p[2][j], p[3][j], t2);
  }
};

__global__ void __launch_bounds__(kEpiTile) epipolar_score_kernel(const float *__restrict__ ccoord, int num_pts,
                                                                  int per_split, const double *__restrict__ fund,
                                                                  int num_loops, float thresh, int *__restrict__ counts,
                                                                  const int *__restrict__ head, PlanarBatch nb) {
  __shared__ double s_pt[4][kEpiTile];
  ransac_score(EpipolarScore{(double)thresh * (double)thresh}, ccoord, num_pts, per_split, fund, num_loops, counts, head,
               nb, s_pt);
}

// head: words kPlanarHeadCand .. kPlanarHeadCount as the planar head's (planar_compact_kernel writes the first); then as
// doubles F[9] (refined) at kEpiHeadF and R[9] (the winner) at kEpiHeadR.  errors == NULL: match_error goes into the
// records; otherwise into errors[] (a batch, whose records stay as they are).
__global__ void __launch_bounds__(kEpiThreads) epipolar_select_kernel(cusift_point *__restrict__ pts, int num_pts,
                                                                      const float *__restrict__ coord,
                                                                      const float *__restrict__ ccoord,
                                                                      const unsigned char *__restrict__ marks,
                                                                      const double *__restrict__ fund,
                                                                      const int *__restrict__ counts, int num_loops,
                                                                      float thresh, int refine_loops, float refine_thresh,
                                                                      int *__restrict__ head, char *__restrict__ flags,
                                                                      float *__restrict__ errors, PlanarBatch nb) {
  __shared__ unsigned long long s_key[kEpiThreads];
  __shared__ double s_part[kEpiThreads / 64][kEpiSums];
  __shared__ double s_sum[kEpiSums];
  __shared__ double s_f[9];
  __shared__ int s_ok;
  __shared__ int s_cnt[kEpiThreads];
  pts += (size_t)blockIdx.z * nb.records;
  coord = pair_ptr(coord, nb.scratch), ccoord = pair_ptr(ccoord, nb.scratch);
  marks = pair_ptr(marks, nb.scratch), fund = pair_ptr(fund, nb.scratch);
  counts = pair_ptr(counts, nb.scratch), head = pair_ptr(head, nb.head);
  flags += (size_t)blockIdx.z * nb.flags;
  if (errors) errors += (size_t)blockIdx.z * nb.flags;
  const float *__restrict__ cx1 = coord, *__restrict__ cy1 = coord + num_pts;
  const float *__restrict__ cx2 = coord + 2 * (size_t)num_pts, *__restrict__ cy2 = coord + 3 * (size_t)num_pts;
  const float *__restrict__ kx1 = ccoord, *__restrict__ ky1 = ccoord + num_pts;
  const float *__restrict__ kx2 = ccoord + 2 * (size_t)num_pts, *__restrict__ ky2 = ccoord + 3 * (size_t)num_pts;
  const int tx = threadIdx.x;
  double *dhead = (double *)head;
  const int n = pair_count(head, num_pts, nb);
  const int n_cand = min(head[kPlanarHeadCand], n);
  if (n_cand < 8) {  // uniform: nine zeros in both matrices, no inlier, the records stay as they are
    for (int i = tx; i < n; i += kEpiThreads) flags[i] = 0;
    if (tx < 9) dhead[kEpiHeadF + tx] = 0.0, dhead[kEpiHeadR + tx] = 0.0;
    if (tx >= kPlanarHeadMatches && tx <= kPlanarHeadLoop) head[tx] = 0;
    return;
  }
  // ---- the first hypothesis with the most inliers ----
  int best, best_count;
  ransac_winner<true>(counts, num_loops, s_key, best, best_count);
  double R[9], F[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) F[i] = R[i] = fund[(size_t)i * num_loops + best];
  const double t2 = (double)thresh * (double)thresh, rt2 = (double)refine_thresh * (double)refine_thresh;
  for (int i = tx; i < n; i += kEpiThreads)  // a record that is no candidate is no inlier
    flags[i] = (marks[i] & 1) && epipolar_inlier(R, (double)cx1[i], (double)cy1[i], (double)cx2[i], (double)cy2[i], t2)
                   ? 1
                   : 0;
  // ---- the refit: thread tx owns candidates tx, tx + 256, ... ----
#pragma unroll 1
  for (int round = 0; round < refine_loops; ++round) {
    // S = the candidates that pass under the current F; its size and centroids
    double a5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = tx; k < n_cand; k += kEpiThreads) {
      const double x1 = kx1[k], y1 = ky1[k], x2 = kx2[k], y2 = ky2[k];
      if (!epipolar_inlier(F, x1, y1, x2, y2, rt2)) continue;
      a5[0] += 1.0, a5[1] += x1, a5[2] += y1, a5[3] += x2, a5[4] += y2;
    }
    wave_tree_sum<5>(a5, s_part, s_sum, tx);
    const double size = s_sum[0];
    if (size < 8.0) break;  // uniform: keep F
    EpiNorm n1, n2;
    n1.cx = s_sum[1] / size, n1.cy = s_sum[2] / size, n2.cx = s_sum[3] / size, n2.cy = s_sum[4] / size;
    double d2[2] = {0.0, 0.0};
    for (int k = tx; k < n_cand; k += kEpiThreads) {
      const double x1 = kx1[k], y1 = ky1[k], x2 = kx2[k], y2 = ky2[k];
      if (!epipolar_inlier(F, x1, y1, x2, y2, rt2)) continue;
      const double ax = x1 - n1.cx, ay = y1 - n1.cy, bx = x2 - n2.cx, by = y2 - n2.cy;
      d2[0] += sqrt(ax * ax + ay * ay);
      d2[1] += sqrt(bx * bx + by * by);
    }
    wave_tree_sum<2>(d2, s_part, s_sum, tx);
    n1.s = sqrt(2.0) / (s_sum[0] / size), n2.s = sqrt(2.0) / (s_sum[1] / size);
    double s[kEpiSums];
#pragma unroll
    for (int q = 0; q < kEpiSums; ++q) s[q] = 0.0;
    for (int k = tx; k < n_cand; k += kEpiThreads) {
      const double x1 = kx1[k], y1 = ky1[k], x2 = kx2[k], y2 = ky2[k];
      if (!epipolar_inlier(F, x1, y1, x2, y2, rt2)) continue;
      const double u1 = (x1 - n1.cx) * n1.s, v1 = (y1 - n1.cy) * n1.s;
      const double u2 = (x2 - n2.cx) * n2.s, v2 = (y2 - n2.cy) * n2.s;
      const double a[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.0};
      int q = 0;
#pragma unroll
      for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j) s[q++] += a[i] * a[j];
    }
    wave_tree_sum<kEpiSums>(s, s_part, s_sum, tx);
    if (tx == 0) {  // one lane solves, everybody reads the answer
      double m[9][9], v[9][9], fh[9], G[9];
      int q = 0;
#pragma unroll
      for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j) m[i][j] = s_sum[q++];
      epipolar_jacobi<9>(m, v, kEpiSweeps9);
      epipolar_smallest<9>(m, v, fh);
      const bool ok = epipolar_finish(fh, n1, n2, G);
#pragma unroll
      for (int i = 0; i < 9; ++i) s_f[i] = G[i];
      s_ok = ok ? 1 : 0;
    }
    __syncthreads();
    if (!s_ok) break;  // uniform: a result that is not finite keeps the previous F and ends the refit
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = s_f[i];
  }
  // ---- match_error of every record, the number of candidates that fit ----
  for (int i = tx; i < n; i += kEpiThreads) {
    double e2, den;
    epipolar_inlier(F, (double)cx1[i], (double)cy1[i], (double)cx2[i], (double)cy2[i], rt2, &e2, &den);
    const float err = (float)sqrt(e2 / den);
    if (errors)
      errors[i] = err;
    else
      pts[i].match_error = err;
  }
  int fit = 0;
  for (int k = tx; k < n_cand; k += kEpiThreads)
    fit += epipolar_inlier(F, (double)kx1[k], (double)ky1[k], (double)kx2[k], (double)ky2[k], rt2) ? 1 : 0;
  fit = block_sum_256(fit, s_cnt);
  if (tx == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      dhead[kEpiHeadF + i] = F[i];
      dhead[kEpiHeadR + i] = R[i];
    }
    head[kPlanarHeadMatches] = best_count;
    head[kPlanarHeadFit] = fit;
    head[kPlanarHeadLoop] = best;
  }
}

}  // namespace cusift
