// sift_rigid.hip -- RANSAC rigid transform from matched 3-D points: x ~ R y + t (coord[num_pts][6] = reference-frame
// xyz, then moving-frame xyz).  Reference: EstimateRigidTransformH, extras/rigidTransform.cu:388-520, with
// estimateRigidTransform3D (:15-209, Horn's quaternion estimate through dsvd of extras/math_utils.cu),
// estimateRigidTransform2D (:222-290, two points in the x-z plane) and testRigidTransform (:292-329).
//
// Three launches on the context's stream, no host round trip between them:
//   rigid_solve_kernel   one hypothesis per lane: draw its three samples (only when the caller gave none), solve, write
//                        Rt[loop][12] and zero counts[loop]
//   rigid_score_kernel   grid (loops / 256, point splits): 256-point tiles in LDS as SoA rows, every lane of a wave
//                        reads the same point (a broadcast), its own 12 coefficients and its count stay in registers;
//                        the splits' partial counts meet in one integer atomic add per lane (order-free)
//   rigid_select_kernel  one workgroup: the winner (64-bit max over count << 32 | loop: the highest count and, among
//                        equals, the highest loop -- the reference's `>=` at :450), its inlier flags, and for the 3-D
//                        type the refit over all its inliers in a fixed reduction order (same bits every run)
// Every kernel has a pair dimension, blockIdx.z: pair p works on its own coordinates, point count, samples, hypotheses,
// counts, head and flags, RigidBatch's strides apart, and draws from seed + p (64-bit, wrapping).  One pair
// (cusift_estimate_rigid, cusift_register_rgbd) is gridDim.z == 1; cusift_register_rgbd_batch runs all its pairs in
// the same three launches.
// The reference's num_loops x num_pts byte matrix of flags (:427) does not exist here: only the winner's row is read.
//
// PRECISION.  Scoring is fp32 like the reference (fused multiply-adds written out).  Both solves and the refit are
// fp64: the 4x4 matrix B of a 3-point sample has a smallest eigenvalue of exactly 0 and its eigenvector is as
// well-conditioned as the gap to the next one allows, so everything an fp32 eigen-solve loses is lost for good; in
// fp64 the answer is the float64 answer rounded once to fp32.  What that costs is part of the timing record of
// tools/bench_rigid.py.
// The reference mixes float and double inside a general Golub-Kahan SVD with new/delete per thread (:22-138,
// math_utils.cu:12-264); B is symmetric positive semi-definite, so a cyclic Jacobi with a fixed number of sweeps and
// selects instead of branches gives the same eigenvector up to sign (the sign does not change R), in registers, with
// all 64 lanes converged.
//
// SAMPLING.  The reference seeds cuRAND with time(0) (:411), which cannot be reproduced: the three samples of a loop
// are ransac_sample<3> of sift_ransac.h, drawn from the point indices.
//
// NOT reproduced from the reference:
//   * testRigidTransform writes the counts into d_indices while other threads still read their samples from it
//     (:373 passes d_indices as d_counts) -- a race; counts have their own array here.
//   * the read-back of the counts overwrites the caller's h_indices (:444); h_indices is const here.
//   * num_pts < 3 spins forever in the redraw loop (:348-349); it is CUSIFT_ERR_INVALID here.
//   * a winner without inliers is refitted over zero points (0/0); a 3-D winner with fewer than 3 inliers keeps its
//     own hypothesis here.
// Kernels use no scratch memory and write with vector stores only.
#include "sift_ransac.h"

namespace cusift {

constexpr int kRigidThreads = 256;  // hypotheses per workgroup of the scoring kernel, threads of the select kernel
constexpr int kRigidTile = 256;     // points per LDS tile
constexpr int kRigidSweeps = 6;     // cyclic Jacobi sweeps over the 6 off-diagonal pairs (fp64 4x4: converged after 5)

// One Jacobi rotation that annihilates a[P][Q] of the symmetric a (upper triangle kept, P < Q) and rotates columns
// P, Q of v.  No branch: an off-diagonal entry that is already zero (or a NaN matrix) takes the identity rotation.
template <int P, int Q>
__device__ __forceinline__ void rigid_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q], d = a[Q][Q] - a[P][P];
  const double den = fabs(d) + sqrt(d * d + 4.0 * apq * apq);
  const double t = den > 0.0 ? (d >= 0.0 ? 2.0 * apq : -2.0 * apq) / den : 0.0;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  a[P][P] -= t * apq;
  a[Q][Q] += t * apq;
  a[P][Q] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r != P && r != Q) {
      double &arp = r < P ? a[r][P] : a[P][r];
      double &arq = r < Q ? a[r][Q] : a[Q][r];
      const double x = arp, y = arq;
      arp = c * x - s * y;
      arq = s * x + c * y;
    }
    const double x = v[r][P], y = v[r][Q];
    v[r][P] = c * x - s * y;
    v[r][Q] = s * x + c * y;
  }
}

// B += A A^T for one centred pair (x, y): A = [0, (y-x)^T; -(y-x), cross(y+x)], extras/rigidTransform.cu:97-133
__device__ __forceinline__ void rigid_accumulate(double (&b)[4][4], const double (&x)[3], const double (&y)[3]) {
  const double d0 = y[0] - x[0], d1 = y[1] - x[1], d2 = y[2] - x[2];
  const double s0 = y[0] + x[0], s1 = y[1] + x[1], s2 = y[2] + x[2];
  const double A[4][4] = {{0.0, d0, d1, d2}, {-d0, 0.0, -s2, s1}, {-d1, s2, 0.0, -s0}, {-d2, -s1, s0, 0.0}};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j) {
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) sum += A[i][k] * A[j][k];
      b[i][j] += sum;
    }
}

// The quaternion = eigenvector of the smallest eigenvalue of B (upper triangle), quat2rot (math_utils.cu:266-280),
// t = xc - R yc (:170-192); rounded to fp32 once, at the end.
__device__ __forceinline__ void rigid_from_b(double (&b)[4][4], const double (&xc)[3], const double (&yc)[3],
                                             float (&rt)[12]) {
  double v[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
#pragma unroll 1
  for (int sweep = 0; sweep < kRigidSweeps; ++sweep) {
    rigid_rotate<0, 1>(b, v);
    rigid_rotate<0, 2>(b, v);
    rigid_rotate<0, 3>(b, v);
    rigid_rotate<1, 2>(b, v);
    rigid_rotate<1, 3>(b, v);
    rigid_rotate<2, 3>(b, v);
  }
  double q[4] = {v[0][0], v[1][0], v[2][0], v[3][0]};
  double low = b[0][0];
#pragma unroll
  for (int i = 1; i < 4; ++i) {  // the first smallest, like :153-160
    const bool take = b[i][i] < low;
    low = take ? b[i][i] : low;
#pragma unroll
    for (int r = 0; r < 4; ++r) q[r] = take ? v[r][i] : q[r];
  }
  const double R[9] = {1.0 - 2.0 * (q[2] * q[2] + q[3] * q[3]), 2.0 * (q[1] * q[2] - q[0] * q[3]),
                       2.0 * (q[1] * q[3] + q[0] * q[2]),       2.0 * (q[1] * q[2] + q[0] * q[3]),
                       1.0 - 2.0 * (q[1] * q[1] + q[3] * q[3]), 2.0 * (q[2] * q[3] - q[0] * q[1]),
                       2.0 * (q[1] * q[3] - q[0] * q[2]),       2.0 * (q[2] * q[3] + q[0] * q[1]),
                       1.0 - 2.0 * (q[1] * q[1] + q[2] * q[2])};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    rt[4 * i + 0] = (float)R[3 * i + 0];
    rt[4 * i + 1] = (float)R[3 * i + 1];
    rt[4 * i + 2] = (float)R[3 * i + 2];
    rt[4 * i + 3] = (float)(xc[i] - (R[3 * i + 0] * yc[0] + R[3 * i + 1] * yc[1] + R[3 * i + 2] * yc[2]));
  }
}

// extras/rigidTransform.cu:222-290: rotation about y and an x-z translation from samples A and B; y is ignored and
// coincident samples give NaN (0/0), which then counts no inlier because every comparison with NaN is false.
__device__ __forceinline__ void rigid_solve_2d(const float *__restrict__ a, const float *__restrict__ b,
                                               float (&rt)[12]) {
  const double wax = a[0], waz = a[2], cax = a[3], caz = a[5];
  const double wbx = b[0], wbz = b[2], cbx = b[3], cbz = b[5];
  const double dxw = wax - wbx, dzw = waz - wbz, lw = sqrt(dxw * dxw + dzw * dzw);
  const double dxc = cax - cbx, dzc = caz - cbz, lc = sqrt(dxc * dxc + dzc * dzc);
  const double uxw = dxw / lw, uzw = dzw / lw, uxc = dxc / lc, uzc = dzc / lc;
  const double cs = uxw * uxc + uzw * uzc, sn = uzw * uxc - uxw * uzc;
  const double sxw = wax + wbx, szw = waz + wbz, sxc = cax + cbx, szc = caz + cbz;
  rt[0] = (float)cs, rt[1] = 0.0f, rt[2] = (float)-sn;
  rt[3] = (float)((sxw - cs * sxc + sn * szc) / 2.0);
  rt[4] = 0.0f, rt[5] = 1.0f, rt[6] = 0.0f, rt[7] = 0.0f;
  rt[8] = (float)sn, rt[9] = 0.0f, rt[10] = (float)cs;
  rt[11] = (float)((szw - sn * sxc - cs * szc) / 2.0);
}

// The number of points when only the device knows it (the matches cusift_register_rgbd selected): *count, never more
// than the capacity the grids were sized by.  count == NULL: the host's num_pts, as cusift_estimate_rigid passes it.
__device__ __forceinline__ int rigid_num_pts(const int *__restrict__ count, int capacity) {
  return count ? min(max(*count, 0), capacity) : capacity;
}

template <bool k3D>
__global__ void __launch_bounds__(64) rigid_solve_kernel(const float *__restrict__ coord, int num_pts,
                                                         int *__restrict__ indices, int num_loops, int draw,
                                                         unsigned long long seed, float *__restrict__ rt_all,
                                                         int *__restrict__ counts, const int *__restrict__ count,
                                                         RigidBatch nb) {
  const int loop = blockIdx.x * 64 + threadIdx.x;
  if (loop >= num_loops) return;
  {
    const size_t pz = blockIdx.z;
    coord += pz * nb.coord, indices += pz * nb.indices, rt_all += pz * nb.rt, counts += pz * nb.counts;
    if (count) count += pz * nb.count;
    seed += pz;
  }
  if (count) {  // the point count is on the device (see rigid_num_pts); too few: rigid_select_kernel answers alone
    num_pts = rigid_num_pts(count, num_pts);
    if (num_pts < (k3D ? 3 : 2)) return;
  }
  int p[3];
  if (draw) {
    ransac_sample<3>(seed, loop, num_pts, p);
    indices[3 * loop + 0] = p[0];
    indices[3 * loop + 1] = p[1];
    indices[3 * loop + 2] = p[2];
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) p[i] = clampi(indices[3 * loop + i], 0, num_pts - 1);  // memory safety only
  }
  float rt[12];
  if (k3D) {
    double x[3][3], y[3][3], xc[3], yc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        x[i][c] = coord[6 * (size_t)p[i] + c];
        y[i][c] = coord[6 * (size_t)p[i] + 3 + c];
      }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      xc[c] = (x[0][c] + x[1][c] + x[2][c]) / 3.0;
      yc[c] = (y[0][c] + y[1][c] + y[2][c]) / 3.0;
    }
    double b[4][4] = {};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double xi[3] = {x[i][0] - xc[0], x[i][1] - xc[1], x[i][2] - xc[2]};
      const double yi[3] = {y[i][0] - yc[0], y[i][1] - yc[1], y[i][2] - yc[2]};
      rigid_accumulate(b, xi, yi);
    }
    rigid_from_b(b, xc, yc, rt);
  } else {
    rigid_solve_2d(coord + 6 * (size_t)p[0], coord + 6 * (size_t)p[1], rt);
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) rt_all[12 * (size_t)loop + i] = rt[i];
  counts[loop] = 0;
}

// |R y + t - x|^2 < thresh2, strictly (extras/rigidTransform.cu:313-319); the one expression both the scoring and the
// winner's flags use, so the flags add up to the winner's count.
__device__ __forceinline__ bool rigid_inlier(const float (&rt)[12], float x0, float x1, float x2, float y0, float y1,
                                             float y2, float thresh2) {
  const float e0 = fmaf(rt[0], y0, fmaf(rt[1], y1, fmaf(rt[2], y2, rt[3]))) - x0;
  const float e1 = fmaf(rt[4], y0, fmaf(rt[5], y1, fmaf(rt[6], y2, rt[7]))) - x1;
  const float e2 = fmaf(rt[8], y0, fmaf(rt[9], y1, fmaf(rt[10], y2, rt[11]))) - x2;
  return fmaf(e0, e0, fmaf(e1, e1, e2 * e2)) < thresh2;
}

// blockIdx.x: 256 hypotheses (one per lane); blockIdx.y: the points [y * pts_per_split, (y + 1) * pts_per_split).
__global__ void __launch_bounds__(kRigidThreads) rigid_score_kernel(const float *__restrict__ coord, int num_pts,
                                                                    int pts_per_split,
                                                                    const float *__restrict__ rt_all, int num_loops,
                                                                    float thresh2, int *__restrict__ counts,
                                                                    const int *__restrict__ count,
                                                                    RigidBatch nb) {
  __shared__ float s_pt[6][kRigidTile + 1];
  {
    const size_t pz = blockIdx.z;
    coord += pz * nb.coord, rt_all += pz * nb.rt, counts += pz * nb.counts;
    if (count) count += pz * nb.count;
  }
  num_pts = rigid_num_pts(count, num_pts);
  const int tx = threadIdx.x;
  const int loop = blockIdx.x * kRigidThreads + tx;
  const int src = loop < num_loops ? loop : num_loops - 1;  // lanes past the end score a copy and drop the result
  float rt[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) rt[i] = rt_all[12 * (size_t)src + i];
  const int begin = blockIdx.y * pts_per_split;
  const int end = min(num_pts, begin + pts_per_split);
  int cnt = 0;
  for (int tile = begin; tile < end; tile += kRigidTile) {
    const int n = min(kRigidTile, end - tile);
    __syncthreads();
    for (int e = tx; e < 6 * n; e += kRigidThreads) s_pt[e % 6][e / 6] = coord[6 * (size_t)tile + e];
    __syncthreads();
#pragma unroll 4
    for (int j = 0; j < n; ++j)
      cnt += rigid_inlier(rt, s_pt[0][j], s_pt[1][j], s_pt[2][j], s_pt[3][j], s_pt[4][j], s_pt[5][j], thresh2) ? 1 : 0;
  }
  if (loop < num_loops && cnt) atomicAdd(&counts[loop], cnt);
}

// Sum of one double per thread over the workgroup in a fixed tree order; every thread gets the sum.
__device__ __forceinline__ double rigid_block_sum(double v, double *s_red) {
  const int tx = threadIdx.x;
  __syncthreads();
  s_red[tx] = v;
  __syncthreads();
#pragma unroll
  for (int half = kRigidThreads / 2; half > 0; half >>= 1) {
    if (tx < half) s_red[tx] += s_red[tx + half];
    __syncthreads();
  }
  return s_red[0];
}

// head: Rt[12] as float, then count and winning loop as int and, with a device-side point count, that count
// (16 words).
template <bool k3D>
__global__ void __launch_bounds__(kRigidThreads) rigid_select_kernel(const float *__restrict__ coord, int num_pts,
                                                                     const float *__restrict__ rt_all,
                                                                     const int *__restrict__ counts, int num_loops,
                                                                     float thresh2, float *__restrict__ head,
                                                                     char *__restrict__ flags,
                                                                     const int *__restrict__ count,
                                                                     RigidBatch nb) {
  __shared__ unsigned long long s_key[kRigidThreads];
  __shared__ double s_red[kRigidThreads];
  const int tx = threadIdx.x;
  {
    const size_t pz = blockIdx.z;
    coord += pz * nb.coord, rt_all += pz * nb.rt, counts += pz * nb.counts, head += pz * nb.head, flags += pz * nb.flags;
    if (count) count += pz * nb.count;
  }
  if (count) {
    num_pts = rigid_num_pts(count, num_pts);
    if (tx == 0) ((int *)head)[kRigidHeadCount] = num_pts;
    if (num_pts < (k3D ? 3 : 2)) {  // uniform; nothing was solved: the identity, no inlier
      for (int i = tx; i < num_pts; i += kRigidThreads) flags[i] = 0;
      if (tx < kRigidHeadInliers) head[tx] = (tx % 5 == 0) ? 1.0f : 0.0f;
      if (tx == 0) ((int *)head)[kRigidHeadInliers] = 0, ((int *)head)[kRigidHeadLoop] = 0;
      return;
    }
  }
  int best, best_count;
  ransac_winner<false>(counts, num_loops, s_key, best, best_count);
  float rt[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) rt[i] = rt_all[12 * (size_t)best + i];
  // the winner's flags; for the refit, the inliers' centroids (thread tx owns points tx, tx + 256, ...)
  double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tx; i < num_pts; i += kRigidThreads) {
    const float *c = coord + 6 * (size_t)i;
    const bool in = rigid_inlier(rt, c[0], c[1], c[2], c[3], c[4], c[5], thresh2);
    flags[i] = in ? 1 : 0;
    if (k3D && in) {
#pragma unroll
      for (int k = 0; k < 6; ++k) sum[k] += (double)c[k];
    }
  }
  if (k3D && best_count >= 3) {  // uniform: extras/rigidTransform.cu:477-479, the same estimator over all inliers
    double xc[3], yc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      xc[k] = rigid_block_sum(sum[k], s_red) / (double)best_count;
      yc[k] = rigid_block_sum(sum[3 + k], s_red) / (double)best_count;
    }
    double b[4][4] = {};
    for (int i = tx; i < num_pts; i += kRigidThreads) {
      if (!flags[i]) continue;  // written by this thread above
      const float *c = coord + 6 * (size_t)i;
      const double xi[3] = {c[0] - xc[0], c[1] - xc[1], c[2] - xc[2]};
      const double yi[3] = {c[3] - yc[0], c[4] - yc[1], c[5] - yc[2]};
      rigid_accumulate(b, xi, yi);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i; j < 4; ++j) b[i][j] = rigid_block_sum(b[i][j], s_red);
    rigid_from_b(b, xc, yc, rt);
  }
  if (tx == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) head[i] = rt[i];
    ((int *)head)[kRigidHeadInliers] = best_count;  // the winner's count before the refit, like :455
    ((int *)head)[kRigidHeadLoop] = best;
  }
}

template __global__ void rigid_solve_kernel<false>(const float *, int, int *, int, int, unsigned long long, float *,
                                                   int *, const int *, RigidBatch);
template __global__ void rigid_solve_kernel<true>(const float *, int, int *, int, int, unsigned long long, float *,
                                                  int *, const int *, RigidBatch);
template __global__ void rigid_select_kernel<false>(const float *, int, const float *, const int *, int, float,
                                                    float *, char *, const int *, RigidBatch);
template __global__ void rigid_select_kernel<true>(const float *, int, const float *, const int *, int, float, float *,
                                                   char *, const int *, RigidBatch);

}  // namespace cusift
