// sift_planar.hip -- planar registration on the device: from matched SiftData to a refined homography without a host
// decision.  Reference: FindHomography (extras/homography.cu:182-269) followed by ImproveHomography (:271-336), the
// chain its demo runs (main.cpp:331-335).  cusift_estimate_homography / cusift_register_planar enqueue, on the context's
// stream, with no host round trip in between:
//
//   planar_mark_kernel      per record: candidate? member of the refit set?  SoA coordinates [x1 | y1 | x2 | y2] of ALL
//                           records (TestHomographies counts over all of them); candidates per 256-record workgroup
//                           (pair_mark of sift_ransac_chain.h, the body the PnP chain's marking shares)
//   planar_compact_kernel   the candidates' record indices in ASCENDING order and their number.  No atomics: the
//                           workgroups before this one are summed, the own keeps are ranked by keep_rank_256
//   homography_solve_kernel (sift_homography.hip) drawing its own four samples per hypothesis from the candidate list
//   planar_score_kernel     TestHomographies: ransac_score (sift_ransac_chain.h, the scoring body of all three models)
//                           over all records with planar_inlier; grid (loops / 64, point splits)
//   planar_select_kernel    one workgroup: the winner (the most inliers and, among equals, the FIRST, :249-254:
//                           ransac_winner<true>), its inlier flags, ImproveHomography's rounds of weighted normal
//                           equations, then match_error of every record and the number of records with err < limit
// Every kernel has a pair index, blockIdx.z: pair p's arrays lie PlanarBatch's strides further and it draws from seed + p.
// One pair (cusift_estimate_homography, cusift_register_planar) is gridDim.z == 1 with every stride 0.
// cusift_register_planar_batch runs all its pairs in the same launches: sequence_mark_kernel (sift_sequence.hip) takes
// planar_mark_kernel's place -- it reads the match rows of cusift_match_batch instead of the records' match fields and
// leaves each pair's record count in its head -- and the other kernels read that count (pair_count): num_pts is then
// the capacity of a pair, the stride of its coordinate rows.  The refit's lane and wave assignment depends on the record
// index alone, so a pair of a batch sums in the order of the pair call.  A batch's planar_select_kernel writes
// match_error to an array of its own: the records are read only.
//
// CANDIDATES.  rule 0: score > lo && ambiguity < hi (FindHomography, :218-219; dot-product distance).  rule 1: score <
// lo^2 && ambiguity < hi^2 (cusift_select_matches type 0; L2 distance; the squares arrive computed in fp32).  Both: finite
// coords2D / match_xpos / match_ypos and, when num_pts2 >= 0, 0 <= match < num_pts2.  With the context's cross-check on,
// the registrations add `mutual`: 0 <= match < num_pts2 and record `match` of image 2 names this record as ITS best (the
// column side of cusift_match_mutual; an exactly tied best keeps the lowest record of image 1) -- for the candidates and
// for the refit set, rule 0's literal predicate included.
//
// SAMPLING.  The four samples of a loop are cand[ransac_sample<4>] (sift_ransac.h): positions in the candidate list.
//
// PRECISION.  Hypotheses and counts are fp32 with the arithmetic of sift_homography.hip (bit for bit the oracle's; the
// inlier test multiplies with round-toward-zero like __fmul_rz: the double product of two floats is exact, so keeping
// the operands as doubles changes no bit).  The refit's 8x8 sums and its Cholesky solve are fp64 like the reference's
// host code: the normal matrix of the UNNORMALISED system has a condition number of 1.4e13 .. 2.2e13 on the planted sets
// of tests/test_homography.py (measured with numpy), so fp32 sums are useless; in fp64 two different summation orders
// move the mapped corners of a 1280 x 960 frame by about 1e-10 px.  The partial sums are reduced in a fixed order
// (wave_tree_sum), so every run gives the same bits.  Only the structurally non-zero entries are
// summed: Yx = [x, y, 1, 0, 0, 0, -x mx, -y mx] and Yy = [0, 0, 0, x, y, 1, -x my, -y my] have three zeros each, the
// [3..5][3..5] block of M equals the [0..2][0..2] block and the [0..2][3..5] block is 0 -- 21 sums of M, 8 of X.
// A normal matrix that is not positive definite (NaN included) keeps the previous A, as cholesky_solve8 of
// include/homography.h does.
// Kernels use no scratch memory and write with vector stores only.
#include "sift_ransac_chain.h"

namespace cusift {

constexpr int kPlanarThreads = 256;  // mark / compact / select
constexpr int kPlanarTile = 64;      // hypotheses per workgroup of the scoring kernel, points per LDS tile
static_assert(kPlanarTile == kRansacTile && kPlanarThreads == kRansacThreads, "the shared bodies' geometry");
constexpr int kPlanarSums = 29;

// coord [4][num_pts], marks [num_pts], block_counts [ceil(num_pts / 256)]: pair_mark<false> (sift_ransac_chain.h).
__global__ void __launch_bounds__(kPlanarThreads) planar_mark_kernel(const cusift_point *__restrict__ pts, int num_pts,
                                                                     int num_pts2, int rule, float lo, float hi,
                                                                     float *__restrict__ coord,
                                                                     unsigned char *__restrict__ marks,
                                                                     int *__restrict__ block_counts, PlanarBatch nb,
                                                                     const cusift_point *__restrict__ pts2) {
  __shared__ int s_wave[kPlanarThreads / 64];
  pair_mark<false>(pts, num_pts, num_pts2, rule, lo, hi, coord, marks, block_counts, nb, pts2, s_wave);
}

// cand[k] = record index of the k-th candidate; the last workgroup writes their number into head[kPlanarHeadCand].
__global__ void __launch_bounds__(kPlanarThreads) planar_compact_kernel(const unsigned char *__restrict__ marks,
                                                                        int num_pts,
                                                                        const int *__restrict__ block_counts,
                                                                        int *__restrict__ cand, int *__restrict__ head,
                                                                        PlanarBatch nb) {
  __shared__ int s_red[kPlanarThreads];
  __shared__ int s_wave[kPlanarThreads / 64];
  marks = pair_ptr(marks, nb.scratch), block_counts = pair_ptr(block_counts, nb.scratch);
  cand = pair_ptr(cand, nb.scratch), head = pair_ptr(head, nb.head);
  const int tx = threadIdx.x;
  const int n = pair_count(head, num_pts, nb);
  int before = 0;
  for (int b = tx; b < (int)blockIdx.x; b += kPlanarThreads) before += block_counts[b];
  const int base = block_sum_256(before, s_red);
  const int i = blockIdx.x * kPlanarThreads + tx;
  const bool keep = i < n && (marks[i] & 1);
  int total;
  const int rank = keep_rank_256(keep, s_wave, total);
  if (keep) cand[base + rank] = i;  // < n: every keep before this one is a distinct record below i
  // a pair of a batch with fewer records than its model fits (8 for H and F, 6 for PnP) reports no candidate, as the
  // pair call answers before it counts
  if (blockIdx.x == gridDim.x - 1 && tx == 0) head[kPlanarHeadCand] = (nb.count && n < nb.min_pts) ? 0 : base + total;
}

// a * b rounded toward zero for a, b that hold fp32 values: the product is exact in fp64; round it to nearest, then step
// back towards zero if that overshot (f != 0 there, so the step is one off the magnitude bits -- nextafterf(f, 0)).
__device__ __forceinline__ float planar_mul_rz(double a, double b) {
  const double p = a * b;
  const float f = (float)p;
  const unsigned int bits = __builtin_bit_cast(unsigned int, f);
  return fabs((double)f) > fabs(p) ? __builtin_bit_cast(float, bits - 1u) : f;
}

// TestHomographies' inlier test (extras/homography.cu:160-171), the expressions of homography_test_kernel; the one
// function both the scoring and the winner's flags use, so the flags add up to the winner's count.
__device__ __forceinline__ bool planar_inlier(const double (&a)[8], float a2, float a5, double x1, double y1, double x2,
                                              double y2, double thresh2) {
  const float nomx = planar_mul_rz(a[0], x1) + planar_mul_rz(a[1], y1) + a2;
  const float nomy = planar_mul_rz(a[3], x1) + planar_mul_rz(a[4], y1) + a5;
  const float deno = planar_mul_rz(a[6], x1) + planar_mul_rz(a[7], y1) + 1.0f;
  const double dd = (double)deno;
  const float errx = planar_mul_rz(x2, dd) - nomx;
  const float erry = planar_mul_rz(y2, dd) - nomy;
  const float err2 = planar_mul_rz((double)errx, (double)errx) + planar_mul_rz((double)erry, (double)erry);
  return err2 < planar_mul_rz(thresh2, (double)planar_mul_rz(dd, dd));
}

// ransac_score's model (sift_ransac_chain.h): 8 floats per hypothesis, counted over ALL records as TestHomographies
// does; the threshold arrives squared in fp32 from the host.
struct PlanarScore {
  static constexpr int kValues = 8, kRows = 4, kMin = 8, kUnroll = 2;
  static constexpr bool kCandidates = false;
  typedef float value_t;
  double t2;
  __device__ __forceinline__ void stage(double (*s_pt)[kPlanarTile], const float *__restrict__ coord, int num_pts, int tile,
                                        int tx) const {
    stage_rows<4>(s_pt, coord, num_pts, tile, tx);
  }
  __device__ __forceinline__ bool inlier(const double (&a)[8], const double (*p)[kPlanarTile], int j) const {
    return planar_inlier(a, (float)a[2], (float)a[5], p[0][j], p[1][j], p[2][j], p[3][j], t2);
  }
};

__global__ void __launch_bounds__(kPlanarTile) planar_score_kernel(const float *__restrict__ coord, int num_pts,
                                                                   int pts_per_split, const float *__restrict__ homo,
                                                                   int num_loops, float thresh2,
                                                                   int *__restrict__ counts,
                                                                   const int *__restrict__ head, PlanarBatch nb) {
  __shared__ double s_pt[4][kPlanarTile];
  ransac_score(PlanarScore{(double)thresh2}, coord, num_pts, pts_per_split, homo, num_loops, counts, head, nb, s_pt);
}

// The reprojection error of ImproveHomography, include/homography.h:116-120 and :134-137 (the same expressions).
__device__ __forceinline__ float planar_err(const double (&A)[8], float px, float py, float mx, float my) {
  const float den = (float)(A[6] * px + A[7] * py + 1.0);
  const float dx = (float)((A[0] * px + A[1] * py + A[2]) / den - mx);
  const float dy = (float)((A[3] * px + A[4] * py + A[5]) / den - my);
  return dx * dx + dy * dy;
}

// head: H[9] (refined), R[9] (the winner) as float, then n_cand, the winner's count, num_fit, the winning loop as int.
// errors == NULL: match_error goes into the records; otherwise into errors[] (a batch, whose records stay as they are).
__global__ void __launch_bounds__(kPlanarThreads) planar_select_kernel(cusift_point *__restrict__ pts, int num_pts,
                                                                       const float *__restrict__ coord,
                                                                       const unsigned char *__restrict__ marks,
                                                                       const float *__restrict__ homo,
                                                                       const int *__restrict__ counts, int num_loops,
                                                                       float thresh2, int refine_loops, float limit,
                                                                       float *__restrict__ head,
                                                                       char *__restrict__ flags,
                                                                       float *__restrict__ errors, PlanarBatch nb) {
  __shared__ unsigned long long s_key[kPlanarThreads];
  __shared__ double s_part[kPlanarThreads / 64][kPlanarSums];
  __shared__ double s_sum[kPlanarSums];
  __shared__ double s_a[8];
  __shared__ int s_cnt[kPlanarThreads];
  pts += (size_t)blockIdx.z * nb.records;
  coord = pair_ptr(coord, nb.scratch), marks = pair_ptr(marks, nb.scratch), homo = pair_ptr(homo, nb.scratch);
  counts = pair_ptr(counts, nb.scratch), head = pair_ptr(head, nb.head);
  flags += (size_t)blockIdx.z * nb.flags;
  if (errors) errors += (size_t)blockIdx.z * nb.flags;
  const float *__restrict__ cx1 = coord, *__restrict__ cy1 = coord + num_pts;
  const float *__restrict__ cx2 = coord + 2 * (size_t)num_pts, *__restrict__ cy2 = coord + 3 * (size_t)num_pts;
  const int tx = threadIdx.x;
  int *ihead = (int *)head;
  const int n = pair_count(ihead, num_pts, nb);
  if (ihead[kPlanarHeadCand] < 8) {  // uniform; extras/homography.cu:220: the identity, no inlier, the records stay as they are
    for (int i = tx; i < n; i += kPlanarThreads) flags[i] = 0;
    if (tx < kPlanarHeadCand) head[tx] = (tx % 9 == 0 || tx % 9 == 4 || tx % 9 == 8) ? 1.0f : 0.0f;
    if (tx >= kPlanarHeadMatches && tx <= kPlanarHeadLoop) ihead[tx] = 0;
    return;
  }
  // ---- the first hypothesis with the most inliers ----
  int best, best_count;
  ransac_winner<true>(counts, num_loops, s_key, best, best_count);
  float win[8];
  double A[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    win[i] = homo[(size_t)i * num_loops + best];
    A[i] = (double)win[i];
  }
  for (int i = tx; i < n; i += kPlanarThreads)
    flags[i] = planar_inlier(A, win[2], win[5], (double)cx1[i], (double)cy1[i], (double)cx2[i], (double)cy2[i],
                             (double)thresh2)
                   ? 1
                   : 0;
  // ---- ImproveHomography: refine_loops rounds of weighted least squares, A starts as the winner (h[8] = 1) ----
#pragma unroll 1
  for (int round = 0; round < refine_loops; ++round) {
    double s[kPlanarSums];
#pragma unroll
    for (int q = 0; q < kPlanarSums; ++q) s[q] = 0.0;
    for (int i = tx; i < n; i += kPlanarThreads) {  // thread tx owns records tx, tx + 256, ...
      if (!(marks[i] & 2)) continue;
      const float px = cx1[i], py = cy1[i], mx = cx2[i], my = cy2[i];
      const float err = planar_err(A, px, py, mx, my);
      const double w = (double)(limit / (err + limit));
      const double x = px, y = py, u = mx, v = my;
      const double x6 = -(double)(px * mx), x7 = -(double)(py * mx), y6 = -(double)(px * my), y7 = -(double)(py * my);
      s[0] += x * x * w, s[1] += x * y * w, s[2] += x * w, s[3] += y * y * w, s[4] += y * w, s[5] += w;
      s[6] += x * x6 * w, s[7] += x * x7 * w, s[8] += y * x6 * w, s[9] += y * x7 * w, s[10] += x6 * w, s[11] += x7 * w;
      s[12] += x * y6 * w, s[13] += x * y7 * w, s[14] += y * y6 * w, s[15] += y * y7 * w, s[16] += y6 * w, s[17] += y7 * w;
      s[18] += x6 * x6 * w + y6 * y6 * w, s[19] += x6 * x7 * w + y6 * y7 * w, s[20] += x7 * x7 * w + y7 * y7 * w;
      s[21] += x * u * w, s[22] += y * u * w, s[23] += u * w;
      s[24] += x * v * w, s[25] += y * v * w, s[26] += v * w;
      s[27] += x6 * u * w + y6 * v * w, s[28] += x7 * u * w + y7 * v * w;
    }
    wave_tree_sum<kPlanarSums>(s, s_part, s_sum, tx);
    if (tx == 0) {  // one lane solves, everybody reads the answer
      double t[kPlanarSums];
#pragma unroll
      for (int q = 0; q < kPlanarSums; ++q) t[q] = s_sum[q];
      const double M[8][8] = {{t[0], t[1], t[2], 0.0, 0.0, 0.0, t[6], t[7]},
                              {t[1], t[3], t[4], 0.0, 0.0, 0.0, t[8], t[9]},
                              {t[2], t[4], t[5], 0.0, 0.0, 0.0, t[10], t[11]},
                              {0.0, 0.0, 0.0, t[0], t[1], t[2], t[12], t[13]},
                              {0.0, 0.0, 0.0, t[1], t[3], t[4], t[14], t[15]},
                              {0.0, 0.0, 0.0, t[2], t[4], t[5], t[16], t[17]},
                              {t[6], t[8], t[10], t[12], t[14], t[16], t[18], t[19]},
                              {t[7], t[9], t[11], t[13], t[15], t[17], t[19], t[20]}};
      const double X[8] = {t[21], t[22], t[23], t[24], t[25], t[26], t[27], t[28]};
      double r[8];
      const bool ok = cholesky_lower<8>(M, X, r);  // cholesky_solve8 of include/homography.h
#pragma unroll
      for (int i = 0; i < 8; ++i) s_a[i] = ok ? r[i] : A[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) A[i] = s_a[i];
  }
  // ---- match_error of every record, the number that fit (include/homography.h:131-140) ----
  int fit = 0;
  for (int i = tx; i < n; i += kPlanarThreads) {
    const float err = planar_err(A, cx1[i], cy1[i], cx2[i], cy2[i]);
    fit += err < limit ? 1 : 0;
    if (errors)
      errors[i] = sqrtf(err);
    else
      pts[i].match_error = sqrtf(err);
  }
  fit = block_sum_256(fit, s_cnt);
  if (tx == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      head[kPlanarHeadH + i] = (float)A[i];
      head[kPlanarHeadR + i] = win[i];
    }
    head[kPlanarHeadH + 8] = 1.0f;
    head[kPlanarHeadR + 8] = 1.0f;
    ihead[kPlanarHeadMatches] = best_count;
    ihead[kPlanarHeadFit] = fit;
    ihead[kPlanarHeadLoop] = best;
  }
}

}  // namespace cusift
