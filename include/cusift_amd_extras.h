/*
 * cusift_amd_extras.h -- the next rows of SURVEY 8f behind the C ABI: the brute-force matcher, the RANSAC homography, the
 * planar registration built on both (seeded RANSAC + refit on the device), the RANSAC rigid transform and the RGB-D
 * registration built on them (depth lift, match selection, the fused call for one frame pair and for a pair list over a
 * batch of frames), the epipolar registration, the calibrated pose behind it and the absolute pose
 * from 3-D/2-D matches (PnP), the 8-bit descriptors (quantiser, int8 matcher).
 * Part of the C ABI of libcusift_amd.so; conventions and the map of the four headers: cusift_amd.h.
 */
#ifndef CUSIFT_AMD_EXTRAS_H
#define CUSIFT_AMD_EXTRAS_H

#include <stdint.h>

#include "cusift_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- matcher (first consumer of SiftData) ----------------------------- */
/* MatchSiftData(data1, data2, distance, ...), extras/matching.cu:232-362: for every point of d_sift1 the best
 * and second-best point of d_sift2 under `distance` (0 = MatchSiftDistanceDotProduct, 1 = MatchSiftDistanceL2,
 * extras/matching.h:10-13); writes score, ambiguity, match, match_xpos, match_ypos of d_sift1 (extras/matching.cu:
 * 140-150,219-229).  The score/ambiguity thresholds of the reference are a host-side filter over those fields
 * (:318-349) and stay on the caller's side (include/matching.h does it).  Asynchronous on the context's stream. */
int cusift_match(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2, int num_pts2,
                 int distance);
/* Mutual nearest neighbours: both directions from ONE pass over the scores S[i][j] (the k-ordered MFMA chain of
 * cusift_match, from the same text; for distance 1 the same 2 - 2 dot / 999 transform).
 * ROW SIDE: score, ambiguity, match, match_xpos, match_ypos of d_sift1[0 .. num_pts1) receive exactly the bytes
 * cusift_match(d_sift1, num_pts1, d_sift2, num_pts2, distance) writes (the same scan, tree and column splits;
 * CUSIFT_POLICY_MATCH_SPLITS is honoured the same way).
 * COLUMN SIDE: the same five fields of d_sift2[j], j in [0, num_pts2), by this model: scan the rows i = 0, 1, ...,
 * num_pts1 - 1 in ascending order from (best, second, match) = (init, init, -1), init = 999 for distance 1 and -1 for
 * distance 0, with strict compares -- a score that beats best moves best to second and takes its place, otherwise a
 * score that beats second replaces it; a NaN score changes nothing.  So `match` is the LOWEST row among exactly tied best
 * scores, and a tie for best gives second == best.  score = best; ambiguity as cusift_match computes it (the 1e-6 is a
 * double); match_xpos / match_ypos = coords2D of d_sift1[match], of record 0 when match is outside [0, num_pts1).  The
 * result does not depend on the split count or the grid: the same input gives the same bytes on every run (no atomics).
 * Nothing but these fields of these records is written.  A count <= 0 on either side: CUSIFT_OK, nothing enqueued, no
 * record of either set touched.  Scratch (12 bytes per row block of 64 and column) lives in the context.
 * CUSIFT_ERR_INVALID (nothing enqueued): what cusift_match refuses, and record ranges of d_sift1 and d_sift2 that overlap
 * -- both are written; match a set against a copy of itself.  Asynchronous on the context's stream. */
int cusift_match_mutual(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, cusift_point *d_sift2, int num_pts2,
                        int distance);
/* Guided matching: nearest neighbours under a model that is already known -- the second matching pass of a registration.
 * On repeated structure the best and the second-best descriptor are near-equal, `ambiguity` is close to 1 and the ratio
 * test discards the match; once H or F is known the look-alike usually lies far from where the model puts the partner.
 * THE RESULT is cusift_match's with one more rule: a column j that fails the geometric test below against row i scores
 * the initial value for that row -- 999 for distance 1, -1 for distance 0 -- which changes nothing in the strict-compare
 * scan.  The scan, the tree over the lanes, the column splits (CUSIFT_POLICY_MATCH_SPLITS included), the merge and the
 * five fields written are cusift_match's, from the same text.
 * A ROW FOR WHICH NO COLUMN PASSES receives score = the initial value, match = -1, the ambiguity that two initial values
 * give (999 / (999 + 1e-6), or 2 / (2 + 1e-6)) and match_xpos / match_ypos of record 0, as cusift_match answers for a row
 * that no column can win.  The candidate marking of the estimate / register calls rejects match = -1 whenever num_pts2 >=
 * 0 is given.
 * A ROW WITH EXACTLY ONE PASSING COLUMN has second = the initial value and therefore a tiny ambiguity.  That is intended
 * -- it is the only compatible partner; the caller's score threshold is what guards against a bad descriptor distance.
 * THE TEST uses x1 = coords2D of row i and x2 = coords2D of column j, floats, and is pinned to these expressions (the
 * build uses -ffp-contract=off), so that a restatement in float64 / float32 gives the same bit.
 * CUSIFT_GUIDE_HOMOGRAPHY: M = H row-major, x2 ~ H x1, the direction of cusift_register_planar's output (widen its floats).
 *   per row, fp64 (x1, y1 widened):   X = (H0*x1 + H1*y1) + H2;  Y = (H3*x1 + H4*y1) + H5;  W = (H6*x1 + H7*y1) + H8;
 *                                     px = (float)(X / W);  py = (float)(Y / W)
 *   per pair, fp32:                   dx = x2 - px;  dy = y2 - py;  pass <=> dx*dx + dy*dy < r2,  r2 = radius * radius
 *   A NaN anywhere is no pass; so is W == 0, which gives an infinity or a NaN.
 * CUSIFT_GUIDE_EPIPOLAR: M = F row-major with x2^T F x1 = 0, the convention of cusift_estimate_fundamental.
 *   per row, fp64:   l0, l1, l2 exactly as in the Sampson test above;  n = sqrt(l0*l0 + l1*l1);
 *                    a = (float)(l0 / n);  b = (float)(l1 / n);  c = (float)(l2 / n)
 *   per pair, fp32:  d = (a*x2 + b*y2) + c;  pass <=> d*d < r2
 *   A row whose line is not usable -- unless n > 0, n < infinity and |l2| < infinity -- has a = b = c = NaN: no column
 *   passes.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing written): everything cusift_match refuses, an unknown model, a NULL
 * h_model, radius not > 0 (NaN included).  +infinity is a legal radius (every finite test passes).  A model that is not
 * finite is no error: it passes nothing.  A count <= 0 on either side: CUSIFT_OK, nothing enqueued, as cusift_match.
 * h_model is read before the call returns.  Asynchronous on the context's stream; writes what cusift_match writes and
 * nothing else. */
#define CUSIFT_GUIDE_HOMOGRAPHY 0
#define CUSIFT_GUIDE_EPIPOLAR 1
int cusift_match_guided(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2, int num_pts2,
                        int distance, int model, const double h_model[9], float radius);
/* Matching by projection: nearest neighbours under a known pose -- the guided pass behind cusift_register_pnp, and the
 * search a tracker runs per frame (ORB-SLAM's SearchByProjection, COLMAP's guided matching after image registration).
 * The records of d_sift1 carry map points in coords3D (cusift_lift_depth, cusift_register_pose); a pose of camera 2,
 * predicted or just estimated, says where each lands in image 2, and only the records of d_sift2 that lie there count.
 * THE RESULT is cusift_match's with one more rule, exactly as cusift_match_guided states it: a column j that fails the
 * test below against row i scores the initial value for that row.  A row that no column passes receives match = -1, the
 * initial score, the ambiguity of two initial values and match_xpos / match_ypos of record 0; a row with exactly one
 * passing column has a tiny ambiguity.  The scan, the tree, the column splits (CUSIFT_POLICY_MATCH_SPLITS included), the
 * merge and the five fields written are cusift_match's, from the same text.
 * CONVENTIONS are cusift_estimate_pnp's: X1 = (X, Y, Z) = coords3D of row i, widened to double; h_rt = [R | t] row-major
 * with X1 = R X2 + t; fx, fy, px = cx - origin, py = cy - origin of camera2, each widened first; (x2, y2) = coords2D of
 * column j.  THE TEST is pinned to these expressions (the build uses -ffp-contract=off):
 *   per row, fp64:   dx = X - rt[3];  dy = Y - rt[7];  dz = Z - rt[11]
 *                    a = (rt[0]*dx + rt[4]*dy) + rt[8]*dz;  b = (rt[1]*dx + rt[5]*dy) + rt[9]*dz;
 *                    c = (rt[2]*dx + rt[6]*dy) + rt[10]*dz                  (the a, b, c of the PnP inlier test)
 *                    usable <=> Z != 0 && c > 0
 *                    qx = (float)((fx*a)/c + px);  qy = (float)((fy*b)/c + py)       -- both NaN when not usable
 *   per pair, fp32:  ex = x2 - qx;  ey = y2 - qy;  pass <=> ex*ex + ey*ey < r2,  r2 = radius * radius
 * A NaN anywhere is no pass.  A row with no depth (Z == 0, the "no depth" mark of cusift_lift_depth), a row behind camera
 * 2 or on its principal plane, and a row with a coordinate that is not finite pass nothing.  +infinity is a legal radius.
 * A pose that is not finite is no error: it passes nothing.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing written): everything cusift_match refuses; a NULL h_rt or camera2; fx or
 * fy zero or not finite, cx, cy or origin not finite (the checks of cusift_estimate_pnp); radius not > 0 (NaN included).
 * A count <= 0 on either side: CUSIFT_OK, nothing enqueued, as cusift_match.  h_rt and camera2 are read before the call
 * returns.  Asynchronous on the context's stream, no synchronisation; writes what cusift_match writes and nothing else:
 * coords3D is read, never written. */
struct cusift_camera; /* defined below, with the RGB-D calls */
int cusift_match_projected(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                           int num_pts2, int distance, const double h_rt[12], const struct cusift_camera *camera2,
                           float radius);
/* cudaMemcpy2D device->host (extras/matching.cu:311-315 copies the 5 match fields of every record); blocking. */
int cusift_memcpy2d_d2h(cusift_ctx *ctx, void *h_dst, size_t dst_pitch, const void *d_src, size_t src_pitch,
                        size_t width_bytes, size_t rows);

/* ---- RANSAC homography from matched SiftData ------------------------------ */
/* The device part and the final selection of FindHomography(data, homography, numMatches, numLoops, minScore,
 * maxAmbiguity, thresh), extras/homography.cu:182-269: for num_loops hypotheses -- h_rand_pts[i*num_loops + l] is
 * the i-th (of 4) sample of hypothesis l, an index into d_sift; the reference draws them on the host with rand()
 * from the points that pass minScore/maxAmbiguity (:208-235), and so does include/homography.h -- solve the 8x8
 * system (ComputeHomographies :89-130), count the points with reprojection error < thresh (TestHomographies
 * :135-178, over coords2D -> match_xpos/ypos of ALL num_pts records) and return the first hypothesis with the
 * most inliers: h_homography[0..7], h_homography[8] = 1, *num_matches = its count.  h_all_homo ([8][num_loops])
 * and h_all_counts ([num_loops]) may be NULL.  Blocking. */
int cusift_find_homography(cusift_ctx *ctx, const cusift_point *d_sift, int num_pts, const int *h_rand_pts,
                           int num_loops, float thresh, float h_homography[9], int *num_matches, float *h_all_homo,
                           int *h_all_counts);

/* ---- planar registration on the device: seeded homography RANSAC + refit (sift_planar.hip) ------------------- */
/* FindHomography followed by ImproveHomography (extras/homography.cu:182-336, the chain of main.cpp:331-335) on device
 * records that already carry match fields: records in, H out, reproducible from `seed`, no host decision and no host
 * round trip between the stages.
 * CANDIDATES, in ASCENDING record order (ordered compaction without atomics, as cusift_select_matches: the same input
 * gives the same list), by `rule`:
 *     0: score > lo && ambiguity < hi          FindHomography's predicate (:218-219), for the dot-product distance
 *     1: score < lo^2 && ambiguity < hi^2      cusift_select_matches' type-0 predicate, for the L2 distance
 *   under both rules also: coords2D, match_xpos and match_ypos finite and, when num_pts2 >= 0, 0 <= match < num_pts2.
 * SAMPLES are drawn on the device, four distinct candidates per hypothesis, integer arithmetic only:
 *     draw k of loop l:  cand[(mix(seed ^ mix((l << 32) | k)) >> 32) mod n_cand]
 *     mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *             z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)              (64-bit unsigned, wrapping)
 *     p1..p4 = draws 0..3; then with k = 4, 5, ...: while p2 == p1 redraw p2; while p3 is p1 or p2 redraw p3; while p4
 *     is p1, p2 or p3 redraw p4 (the reference's order, :222-235); a slot redrawn 64 times takes the lowest candidate
 *     not taken yet.
 * HYPOTHESES AND COUNTS are ComputeHomographies (:89-130) and TestHomographies (:135-178) with the arithmetic of
 * cusift_find_homography, counted over ALL num_pts records.  The WINNER is the first hypothesis with the most inliers
 * (:237-258), selected on the device: h_ransac[0..7], h_ransac[8] = 1, *num_matches = its count, *best_loop its index,
 * h_inliers[i] = 1 for its inliers.
 * REFIT is ImproveHomography (:271-336) on the device, starting from the winner: refine_loops rounds of the weighted
 * normal equations, weight limit / (err + limit) with limit = refine_thresh^2, over the records with !(score < lo ||
 * ambiguity > hi) under rule 0 (ImproveHomography's literal predicate) and over the candidates under rule 1.  The 8x8
 * sums and the Cholesky solve are fp64 (the unnormalised normal matrix has a condition number above 1e13); the partial
 * sums are reduced in a fixed order, so every run gives the same bits.  A matrix that is not positive definite keeps the
 * previous estimate.  Afterwards match_error = sqrtf(err) is written into EVERY device record (the reference writes the
 * host records) and *num_fit = the number of records with err < limit; h_homography[0..7] is the refined estimate,
 * h_homography[8] = 1.  refine_loops == 0 skips the refit: h_homography = h_ransac, match_error and *num_fit are
 * evaluated with the winner.
 * *num_candidates = the candidates.  Optional (may be NULL): best_loop, h_inliers [num_pts], h_drawn [4][num_loops]
 * (the samples as record indices, the layout cusift_find_homography takes), h_all_homo [8][num_loops], h_all_counts
 * [num_loops].  The same seed gives the same bytes in every output and in the records.
 * num_pts < 8 or fewer than 8 candidates (the reference's own limits, :205,220): identity in both matrices, every count
 * 0 (*num_candidates still reports the candidates), the optional arrays zeroed, CUSIFT_OK; the records are untouched.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing written): a NULL h_homography / h_ransac / num_candidates / num_matches
 * / num_fit, num_loops < 1, thresh or refine_thresh not > 0 (NaN included), a NaN lo / hi, an unknown rule, refine_loops
 * < 0, missing buffers.  Any num_loops >= 1 is accepted (the rounding to 16 of :200 belongs to the C++ wrapper).
 * Scratch lives in the context and grows on demand.  Blocking: ONE stream synchronisation, at the one read-back. */
int cusift_estimate_homography(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, int num_pts2 /* < 0: no check */,
                               int rule, float lo, float hi, int num_loops, float thresh, int refine_loops,
                               float refine_thresh, uint64_t seed, float h_homography[9], float h_ransac[9],
                               int *num_candidates, int *num_matches, int *num_fit, int *best_loop /* may be NULL */,
                               char *h_inliers /* may be NULL */, int *h_drawn /* may be NULL */,
                               float *h_all_homo /* may be NULL */, int *h_all_counts /* may be NULL */);

/* cusift_match(d_sift1, d_sift2, distance) followed by cusift_estimate_homography(d_sift1, num_pts1, num_pts2, ...) with
 * ONE synchronisation, at the read-back: the same bits as the staged route in every output and in the records.  Also
 * CUSIFT_ERR_INVALID for an unknown distance.
 * While cusift_ctx_set_cross_check is on, the matcher is cusift_match_mutual: THE MATCH FIELDS OF d_sift2 ARE WRITTEN
 * (score, ambiguity, match, match_xpos, match_ypos; the parameter keeps its const spelling for source compatibility),
 * overlapping record ranges are refused with CUSIFT_ERR_INVALID before anything is enqueued or written, and a record
 * that is not mutual is neither a candidate nor a member of the refit set (see cusift_ctx_set_cross_check). */
int cusift_register_planar(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                           int num_pts2, int distance, int rule, float lo, float hi, int num_loops, float thresh,
                           int refine_loops, float refine_thresh, uint64_t seed, float h_homography[9],
                           float h_ransac[9], int *num_candidates, int *num_matches, int *num_fit,
                           int *best_loop /* may be NULL */, char *h_inliers /* may be NULL */,
                           int *h_drawn /* may be NULL */, float *h_all_homo /* may be NULL */,
                           int *h_all_counts /* may be NULL */);

/* ---- epipolar registration on the device: seeded fundamental-matrix RANSAC + refit (sift_epipolar.hip) --------- */
/* Two views of a general 3-D scene from an ordinary camera: device records that carry match fields in, the fundamental
 * matrix out, reproducible from `seed`, no host decision and no host round trip between the stages.  The reference has no
 * fundamental-matrix code; this definition is the library's own, and ALL OF IT IS FP64 (an fp32 normalised 8-point solve
 * moved the unit-norm F by up to 3e-4 on planted scenes; vector fp64 runs at the unpacked fp32 rate on this device).
 * CONVENTION: x1 = (coords2D, 1), x2 = (match_xpos, match_ypos, 1), floats widened to double; F is row-major 3 x 3 and
 * x2^T F x1 = 0.
 * CANDIDATES are those of cusift_estimate_homography, by the same kernels: rule 0 / 1, finite coordinates, when num_pts2
 * >= 0 also 0 <= match < num_pts2, the cross-check of cusift_register_epipolar, ascending record order, no atomics.
 * EVERYTHING BELOW RUNS OVER THE CANDIDATES ONLY -- counts, flags, the refit set, *num_fit -- not over all records as the
 * planar path does: the epipolar constraint is one-dimensional, so a rejected match lies near a random epipolar line far
 * more often than near a homography's image of its point.
 * SAMPLES: cusift_estimate_homography's recipe (same draw, same mix) with eight slots: p1..p8 = draws 0..7; then, with k
 * counting on from 8, for slot s = 2..8 in order: while p_s equals an earlier slot redraw it; a slot redrawn 64 times
 * takes the lowest candidate not taken yet.  Integer arithmetic only.
 * HYPOTHESIS of one loop: Hartley-normalise the eight samples per image (centroid to 0, mean distance sqrt 2: x~ = (x -
 * c) * s), build the 8 x 9 system with rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1], take its null vector
 * (Gaussian elimination with complete pivoting, back substitution), project to rank 2 (remove the right singular vector
 * of the smallest singular value), denormalise F = T2^T F^ T1, scale to Frobenius norm 1 with the largest-magnitude entry
 * positive (among equals the first in row-major order decides).  A result that is not finite or all zero is nine zeros
 * and counts nothing.
 * INLIER TEST, the Sampson distance, pinned to these expressions (the build uses -ffp-contract=off) so that a float64
 * restatement gives the same bit:
 *     l0 = (F0*x1 + F1*y1) + F2;  l1 = (F3*x1 + F4*y1) + F5;  l2 = (F6*x1 + F7*y1) + F8;
 *     m0 = (F0*x2 + F3*y2) + F6;  m1 = (F1*x2 + F4*y2) + F7;  e = (x2*l0 + y2*l1) + l2;
 *     den = ((l0*l0 + l1*l1) + m0*m0) + m1*m1;    inlier <=> e*e < t2*den,   t2 = (double)thresh * (double)thresh
 * No division, no square root; a NaN or den == 0 is no inlier.  One device function serves the scoring, the winner's
 * flags and the refit's membership.  match_error = (float)sqrt(e*e / den), as IEEE gives it.
 * WINNER: the most inliers, among equals the first loop: h_ransac its matrix, *num_matches its count, *best_loop its
 * index, h_inliers its flags (0 for a record that is no candidate).  When no hypothesis is solvable every count is 0
 * and the first rule still holds: *best_loop = 0, *num_matches = 0, h_ransac nine zeros.
 * REFIT, starting from the winner, refine_loops rounds: S = the candidates that pass the inlier test under the current
 * F at refine_thresh; |S| < 8 ends the refit and keeps F; normalise over S, accumulate the 45 sums of the 9 x 9 matrix
 * sum a a^T (reduced in a fixed order: lane tree, then waves 0..3), take the eigenvector of its smallest eigenvalue by
 * cyclic Jacobi with a fixed sweep schedule, project to rank 2, denormalise, fix norm and sign; a result that is not
 * finite keeps the previous F and ends the refit.  Afterwards match_error is written into EVERY device record [0,
 * num_pts), *num_fit = the candidates that pass at refine_thresh and h_fundamental = F.  refine_loops == 0: h_fundamental
 * equals h_ransac byte for byte.  Under nine zeros e*e / den is 0 / 0: when nothing was solvable match_error of every
 * record is NaN, *num_fit = 0 and h_fundamental is nine zeros.
 * Optional (may be NULL): best_loop, h_inliers [num_pts], h_drawn [8][num_loops] (record indices), h_all_f
 * [9][num_loops], h_all_counts [num_loops].  The same seed gives the same bytes in every output and in the records.
 * num_pts < 8 or fewer than 8 candidates: nine zeros in both matrices, every count 0, the optional arrays zeroed,
 * CUSIFT_OK; the records are untouched.  *num_candidates still reports the candidates when num_pts >= 8; with fewer than
 * 8 records nothing is marked and it is 0, as cusift_estimate_homography answers.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing written): every case of cusift_estimate_homography.
 * Scratch lives in the context and grows on demand.  Blocking: ONE stream synchronisation, at the one read-back. */
int cusift_estimate_fundamental(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, int num_pts2 /* < 0: no check */,
                                int rule, float lo, float hi, int num_loops, float thresh, int refine_loops,
                                float refine_thresh, uint64_t seed, double h_fundamental[9], double h_ransac[9],
                                int *num_candidates, int *num_matches, int *num_fit, int *best_loop /* may be NULL */,
                                char *h_inliers /* may be NULL */, int *h_drawn /* may be NULL */,
                                double *h_all_f /* may be NULL */, int *h_all_counts /* may be NULL */);

/* cusift_match(d_sift1, d_sift2, distance) followed by cusift_estimate_fundamental(d_sift1, num_pts1, num_pts2, ...) with
 * ONE synchronisation, at the read-back: the same bytes as the staged route in every output and in the records.  Also
 * CUSIFT_ERR_INVALID for an unknown distance.  It honours cusift_ctx_set_cross_check exactly as cusift_register_planar
 * does: while it is on, the matcher is cusift_match_mutual, THE MATCH FIELDS OF d_sift2 ARE WRITTEN (the parameter keeps
 * its const spelling), overlapping record ranges are refused with CUSIFT_ERR_INVALID before anything is enqueued or
 * written, and a record that is not mutual is no candidate. */
int cusift_register_epipolar(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                             int num_pts2, int distance, int rule, float lo, float hi, int num_loops, float thresh,
                             int refine_loops, float refine_thresh, uint64_t seed, double h_fundamental[9],
                             double h_ransac[9], int *num_candidates, int *num_matches, int *num_fit,
                             int *best_loop /* may be NULL */, char *h_inliers /* may be NULL */,
                             int *h_drawn /* may be NULL */, double *h_all_f /* may be NULL */,
                             int *h_all_counts /* may be NULL */);

/* ---- RANSAC rigid transform from matched 3-D points -------------------------- */
/* EstimateRigidTransformH(h_coord, Rt, numInliers, numLoops, numPts, thresh2, type, h_indices, h_inliers),
 * extras/rigidTransform.cu:388-520.  h_coord[i] = reference-frame xyz, then moving-frame xyz of match i (coords3D of
 * SiftMatch::pt1 and ::pt2); the result maps the moving frame into the reference frame, x ~ R y + t, as h_rt = [R | t]
 * row-major 3x4.  Every hypothesis l is estimated from the samples h_indices[3 l .. 3 l + 2] -- type 1 (3D): Horn's
 * quaternion estimate from three pairs (:15-209); type 0 (2D): a rotation about y and an x-z translation from the
 * first two (:222-290; coincident samples give a NaN hypothesis that counts no inlier) -- and scored by the number of
 * points with |R y + t - x|^2 < thresh2 (:292-329).  The winner is the hypothesis with the most inliers, among equals
 * the LAST one (the reference's `>=`, :450): *num_inliers is its count, *best_loop its index, h_inliers[i] = 1 for its
 * inliers.  For type 1 h_rt is the same estimate over all the winner's inliers (:477-479) -- unless it has fewer than
 * three, then h_rt is the winner itself; for type 0 h_rt is the winner itself (:472-475).
 * h_indices == NULL: the samples are drawn on the device, three distinct indices per hypothesis, from `seed`:
 *     draw k of loop l:  u = mix(seed ^ mix((l << 32) | k)),  index = (u >> 32) mod num_pts
 *     mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *             z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)              (64-bit unsigned, wrapping)
 *     p1, p2, p3 = draws 0, 1, 2; then with k = 3, 4, ...: while p2 == p1 redraw p2; while p3 is p1 or p2 redraw p3;
 *     a slot redrawn 64 times takes the lowest index not taken yet.
 * The same seed gives the same samples and the same bits in every output.  h_drawn receives the samples that were
 * used (drawn or given).  h_all_rt [num_loops][12], h_all_counts [num_loops]: every hypothesis and its count.
 * CUSIFT_ERR_INVALID: num_pts < 3 (< 2 for type 0 with h_indices), num_loops < 1, thresh2 not > 0, a sample that is
 * read out of [0, num_pts), a NULL h_coord / h_rt / num_inliers.  Nothing of the caller's is written except the
 * outputs.  Blocking: one read-back at the end, no host round trip between the stages. */
int cusift_estimate_rigid(cusift_ctx *ctx, const float *h_coord /* [num_pts][6] */, int num_pts,
                          const int *h_indices /* [num_loops][3], or NULL */, int num_loops, float thresh2,
                          int type /* 0 = 2D (x-z), 1 = 3D */, uint64_t seed, float h_rt[12], int *num_inliers,
                          int *best_loop /* may be NULL */, char *h_inliers /* [num_pts], may be NULL */,
                          float *h_all_rt /* may be NULL */, int *h_all_counts /* may be NULL */,
                          int *h_drawn /* [num_loops][3], may be NULL */);

/* ---- RGB-D registration: depth lift, match selection on the device, the fused frame-pair call (sift_rgbd.hip) --- */
/* A pinhole camera and the encoding of its 16-bit depth image.  The reference ships the inputs of this step
 * (test/data/depth1.png, depth2.png, INTRINSICS, match/match1_2) but no code for it; the convention is the one that
 * reproduces match/match1_2 from the VLFeat keypoints: SUN3D frames, MATLAB (1-based) intrinsics. */
typedef struct cusift_camera {
  float fx, fy, cx, cy;  /* focal lengths and principal point in pixels */
  float origin;          /* pixel-centre convention of cx / cy: 0 = 0-based, 1 = MATLAB 1-based (the fixture) */
  float units_per_metre; /* depth samples per metre: 1000 for millimetres */
  int encoding;          /* 0: the sample is the depth; 1: SUN3D PNG, the depth rotated left by 3 bits */
} cusift_camera;

/* ---- calibrated two-view pose on the device: [R | t] and triangulated points from F (sift_pose.hip) ------------- */
/* The stage behind cusift_estimate_fundamental for a calibrated camera: from F and the intrinsics to the relative pose
 * and to a 3-D point in coords3D of every record that fits, as the RGB-D path ends -- without reading F back, decomposing
 * the essential matrix, testing cheirality and triangulating on the host.  The definition is the library's own and ALL OF
 * IT IS FP64; every expression is evaluated in the order written (the build uses -ffp-contract=off).
 * CAMERAS: K = [[fx, 0, px], [0, fy, py], [0, 0, 1]], px = cx - origin, py = cy - origin, the cusift_camera's floats
 * widened to double first; units_per_metre and encoding are ignored.  camera1 belongs to the records' own image (x1 =
 * coords2D), camera2 to the matches' (x2 = match_xpos / match_ypos); camera2 == NULL: both views use camera1.
 * ESSENTIAL MATRIX: E = K2^T (F K1) with F row-major, x2^T F x1 = 0, the epipolar calls' convention:
 *     A[i][0] = F[3i]*fx1;  A[i][1] = F[3i+1]*fy1;  A[i][2] = (F[3i]*px1 + F[3i+1]*py1) + F[3i+2]
 *     E[0][j] = fx2*A[0][j];  E[1][j] = fy2*A[1][j];  E[2][j] = (px2*A[0][j] + py2*A[1][j]) + A[2][j]
 * DECOMPOSITION: G = E^T E, G[i][j] = (E[0][i]*E[0][j] + E[1][i]*E[1][j]) + E[2][i]*E[2][j]; its eigenpairs by the cyclic
 * Jacobi of the epipolar refit's rank-2 step (3 x 3, the same fixed sweep schedule), ordered l1 >= l2 >= l3, the first
 * among equals; sigma_i = sqrt(l_i > 0 ? l_i : 0);  v3 = v1 x v2;  u1 = E v1 / sigma_1;  u2 = w / |w| with w = E v2 -
 * (E v2 . u1) u1;  u3 = u1 x u2 -- U = [u1 u2 u3] and V = [v1 v2 v3] are proper rotations by construction (dot products
 * and matrix-vector rows are (a0*b0 + a1*b1) + a2*b2).  sigma_3 is then replaced by |u3 . (E v3)| where that is finite:
 * l3 of a rank-2 F is rounding noise of size eps * l1, and its root would keep only half the digits of a value whose
 * distance from 0 is what the caller looks at.  With W = [[0,-1,0],[1,0,0],[0,0,1]] the four candidates (R21,
 * t21), each meaning X2 = R21 X1 + t21, are in this order
 *     (Ra, +u3), (Ra, -u3), (Rb, +u3), (Rb, -u3)
 *     Ra = U W V^T:    Ra[i][j] = (u2[i]*v1[j] - u1[i]*v2[j]) + u3[i]*v3[j]
 *     Rb = U W^T V^T:  Rb[i][j] = (u1[i]*v2[j] - u2[i]*v1[j]) + u3[i]*v3[j]
 * FIT SET: the candidates -- marked exactly as cusift_estimate_fundamental marks them: rule, lo, hi, finite coordinates,
 * 0 <= match < num_pts2 when num_pts2 >= 0 -- that pass the epipolar calls' inlier test under F at `thresh`.
 * DEPTHS of one record under one candidate (R21, t21):
 *     d1 = ((x1 - px1) / fx1, (y1 - py1) / fy1, 1);  d2 = ((x2 - px2) / fx2, (y2 - py2) / fy2, 1)
 *     a[i] = (R21[i][0]*d1x + R21[i][1]*d1y) + R21[i][2]
 *     aa = (a0*a0 + a1*a1) + a2*a2;  bb = (d2x*d2x + d2y*d2y) + 1;  ab = (a0*d2x + a1*d2y) + a2
 *     at = (a0*t0 + a1*t1) + a2*t2;  bt = (d2x*t0 + d2y*t1) + t2
 *     det = aa*bb - ab*ab;  z1 = (ab*bt - bb*at) / det;  z2 = (aa*bt - ab*at) / det
 * the least-squares solution of z1 a + t21 = z2 d2.  IN FRONT: z1 > 0 && z2 > 0; a NaN fails.  (Under -t21 both depths
 * change sign and nothing else, exactly.)
 * WINNER: the candidate with the most records of the fit set in front, among equals the first.  h_votes[4] (may be NULL)
 * = the four counts, *num_front = the winner's.
 * h_rt is double [12], row-major [R | t] in the direction of cusift_register_rgbd, X1 = R X2 + t: R = R21^T, t[i] =
 * -((R21[0][i]*t0 + R21[1][i]*t1) + R21[2][i]*t2), |t| = 1 -- the baseline is the unit of length.  h_sigma[3] (may be
 * NULL) = the singular values of E as computed above: sigma_2 / sigma_1 far from 1 says that F and the intrinsics
 * disagree or that F is poorly determined.
 * coords3D IS WRITTEN FOR EVERY RECORD in [0, num_pts): ((float)(z1*d1x), (float)(z1*d1y), (float)z1) under the winner
 * if the record is in the fit set, in front, and the three floats are finite with z > 0; (0, 0, 0) otherwise.  The point
 * lies on the record's own pixel ray in the camera coordinates of frame 1, cusift_lift_depth's convention, z == 0 its
 * "no depth" mark.  No other byte of any record changes.
 * DEGENERATE ANSWERS, CUSIFT_OK: F is nine zeros or not finite, sigma_2 is not > 0, an entry of Ra, Rb, u3 or sigma is
 * not finite, or the best vote is 0 (num_pts == 0 included) -- h_rt = [I | 0], *num_front = 0, coords3D of every record in
 * [0, num_pts) zeros; the votes are 0 in all these cases, h_sigma is what was computed.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing written): a NULL camera1 / h_rt / num_front / h_fundamental_in; fx or fy
 * zero or not finite, cx, cy or origin not finite, in either camera; thresh not > 0 (NaN included); what
 * cusift_estimate_fundamental refuses of d_sift, num_pts, rule, lo, hi.
 * Launches: the marking, then pose_vote_kernel and pose_write_kernel (the candidate list itself is not needed, so the
 * compaction is not run).  Blocking: ONE stream synchronisation, at the read-back.  The same input gives the same bytes. */
int cusift_estimate_pose(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, int num_pts2 /* < 0: no check */, int rule,
                         float lo, float hi, const double h_fundamental_in[9], float thresh,
                         const cusift_camera *camera1, const cusift_camera *camera2 /* NULL: camera1 */,
                         double h_rt[12], int *num_front, int *h_votes /* [4], may be NULL */,
                         double *h_sigma /* [3], may be NULL */);

/* cusift_register_epipolar followed by cusift_estimate_pose(d_sift1, num_pts1, num_pts2, rule, lo, hi, the returned
 * h_fundamental, refine_thresh, ...) with ONE synchronisation: the two pose launches follow the selection kernel on the
 * stream and read F where it left it.  Every epipolar output and every record byte other than coords3D of d_sift1 equals
 * cusift_register_epipolar's (cross-check included: the marks are the fused call's, so with it on a record that is not
 * mutual is not in the fit set); the pose outputs and coords3D equal the staged call's.  With fewer than 8 records or
 * candidates F is nine zeros: the degenerate answer, coords3D of d_sift1 zeroed.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing written): every case of cusift_register_epipolar and of the cameras and
 * pose outputs above. */
int cusift_register_pose(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2, int num_pts2,
                         int distance, int rule, float lo, float hi, int num_loops, float thresh, int refine_loops,
                         float refine_thresh, uint64_t seed, const cusift_camera *camera1,
                         const cusift_camera *camera2 /* NULL: camera1 */, double h_fundamental[9], double h_ransac[9],
                         int *num_candidates, int *num_matches, int *num_fit, int *best_loop /* may be NULL */,
                         char *h_inliers /* may be NULL */, int *h_drawn /* may be NULL */,
                         double *h_all_f /* may be NULL */, int *h_all_counts /* may be NULL */, double h_rt[12],
                         int *num_front, int *h_votes /* [4], may be NULL */, double *h_sigma /* [3], may be NULL */);

/* ---- absolute pose on the device from 3-D/2-D matches: seeded PnP RANSAC and refit (sift_pnp.hip) ---------------- */
/* The step behind cusift_register_pose or cusift_lift_depth: the records carry a point in coords3D, their matches carry
 * pixels of an ordinary image, and the answer is that image's pose in the unit the points are in -- metres, or the first
 * baseline -- so that a third view, or a colour-only frame, joins the frame of the first.  The definition is the
 * library's own and ALL OF IT IS FP64; every expression is evaluated in the order written (-ffp-contract=off).
 * CONVENTION: X1 = coords3D of the record, in frame 1's camera coordinates; x2 = (match_xpos, match_ypos); floats are
 * widened first.  camera2 is the cusift_camera of the matches' image: px = cx - origin, py = cy - origin (widened
 * first); units_per_metre and encoding are ignored.  A POSE is twelve doubles rt[12], row-major [R | t] with X1 = R X2 +
 * t, the direction of cusift_register_rgbd and cusift_register_pose, t in the unit of coords3D -- h_rt, h_ransac and
 * every column of h_all_rt alike; the hypotheses, the refit and the test below work on this one form.
 * CANDIDATES: the records cusift_estimate_fundamental marks (rule, lo, hi, finite coords2D and match position, 0 <=
 * match < num_pts2 when num_pts2 >= 0, the fused call's cross-check) whose three coords3D floats are finite with
 * coords3D[2] != 0 (0 is the "no depth" mark).  Everything below runs over the candidates only, in ascending record
 * order, without atomics; *num_candidates is their number.
 * SAMPLES: cusift_estimate_homography's recipe with six slots: draws 0 .. 5 of loop l out of the candidate list, then
 * slots 2 .. 6 redrawn while they equal an earlier one, k counting on from 6.
 * HYPOTHESIS from the six samples (X_i, x2_i):
 *     c = (sum X_i) / 6 per coordinate;  d = (sum sqrt((ax*ax + ay*ay) + az*az)) / 6 with a = X_i - c;  s = sqrt(3) / d
 *     X~ = (X - c) * s;   u = (x2 - px) / fx;   v = (y2 - py) / fy
 *     row 2i   = [X~ Y~ Z~ 1   0 0 0 0   -(u*X~) -(u*Y~) -(u*Z~) -u]
 *     row 2i+1 = [0 0 0 0   X~ Y~ Z~ 1   -(v*X~) -(v*Y~) -(v*Z~) -v]
 * the first ELEVEN rows (both of samples 1 to 5, the u row of sample 6).  The null vector of the 11 x 12 system exactly
 * as cusift_estimate_fundamental takes that of its 8 x 9 system: Gaussian elimination with complete pivoting (the pivot
 * of step k is the first entry of largest magnitude in rows k.. and columns k.., searched row by row; rows k and pi are
 * swapped, then columns k and pj; f = M[i][k] / M[k][k], M[i][j] -= f * M[k][j]), back substitution from x[11] = 1 with
 * x[k] = -(sum_{j>k} M[k][j]*x[j]) / M[k][k] summed in ascending j, the column permutation undone.  x is P~, row-major
 * 3 x 4.  Denormalise, with tx = -(s*cx), ty = -(s*cy), tz = -(s*cz):
 *     P[i][j] = P~[i][j] * s (j < 3);   P[i][3] = ((P~[i][0]*tx + P~[i][1]*ty) + P~[i][2]*tz) + P~[i][3]
 * SIGN: det = (P00*(P11*P22 - P12*P21) - P01*(P10*P22 - P12*P20)) + P02*(P10*P21 - P11*P20) of the left 3 x 3 block M; det
 * < 0 negates all twelve.  ROTATION nearest M, by the pose block's construction: G = M^T M, G[i][j] = (M[0][i]*M[0][j] +
 * M[1][i]*M[1][j]) + M[2][i]*M[2][j]; its eigenpairs by the same 3 x 3 cyclic Jacobi with the fixed sweep schedule,
 * ordered l1 >= l2 >= l3, the first among equals; s1 = sqrt(l1 > 0 ? l1 : 0), s2 likewise; v3 = v1 x v2; u1 = M v1 / s1;
 * u2 = w / |w| with w = M v2 - (M v2 . u1) u1; u3 = u1 x u2; s3 = |u3 . (M v3)|;
 *     R21[i][j] = (u1[i]*v1[j] + u2[i]*v2[j]) + u3[i]*v3[j];   scale = ((s1 + s2) + s3) / 3;   t21[i] = P[i][3] / scale
 * (dot products and matrix-vector rows are (a0*b0 + a1*b1) + a2*b2) -- X2 = R21 X1 + t21.  The pose: R = R21^T, t[i] =
 * -((R21[0][i]*t21[0] + R21[1][i]*t21[1]) + R21[2][i]*t21[2]).  scale not > 0 or an entry that is not finite: the
 * hypothesis is twelve zeros and counts nothing.
 * INLIER TEST of (X, Y, Z), (x2, y2) under rt at a threshold t (pixels), t2 = (double)t * (double)t, no division:
 *     dx = X - rt[3];  dy = Y - rt[7];  dz = Z - rt[11]
 *     a = (rt[0]*dx + rt[4]*dy) + rt[8]*dz;  b = (rt[1]*dx + rt[5]*dy) + rt[9]*dz;  c = (rt[2]*dx + rt[6]*dy) + rt[10]*dz
 *     ex = fx*a - (x2 - px)*c;   ey = fy*b - (y2 - py)*c
 *     inlier  <=>  c > 0 && ex*ex + ey*ey < t2 * (c*c)
 * A NaN fails; a point behind the camera fails.  The same expressions serve the scoring, the winner's flags, the refit's
 * membership and *num_fit.  match_error = (float)sqrt((ex*ex + ey*ey) / (c*c)), the reprojection error in pixels, NaN
 * where c > 0 fails.
 * WINNER: the most inliers at `thresh`, among equals the first loop: h_ransac its pose, *num_matches its count,
 * *best_loop its index, h_inliers its flags (0 for a record that is no candidate).
 * REFIT, starting from the winner, refine_loops rounds of Gauss-Newton on the reprojection error: S = the candidates
 * that pass at refine_thresh under the current pose; |S| < 6 ends the refit.  Per member, with a, b, c as above, xs = x2
 * - px, ys = y2 - py:
 *     ic = 1 / c;  ua = a*ic;  vb = b*ic;  g0 = fx*ic;  g2 = -(g0*ua);  h1 = fy*ic;  h2 = -(h1*vb)
 *     ru = fx*ua - xs;   rv = fy*vb - ys
 *     Ju = [g2*b, g0*c - g2*a, -(g0*b), g0, 0, g2];   Jv = [h2*b - h1*c, -(h2*a), h1*a, 0, h1, h2]
 * the 2 x 6 Jacobian with respect to a left rotation increment w and a translation increment d of X2 = R21 X1 + t21.
 * The 21 sums A[i][j] += Ju[i]*Ju[j] + Jv[i]*Jv[j] (i <= j), the 6 sums g[i] += Ju[i]*ru + Jv[i]*rv and |S| are reduced
 * in a fixed order (lane tree, then waves 0..3); A p = -g is solved by Cholesky on one lane (no pivot search; a pivot
 * that is not > 0 ends the refit), p = (w, d).  Rodrigues: th2 = (w0*w0 + w1*w1) + w2*w2, th = sqrt(th2), A = sin(th) /
 * th, B = (1 - cos(th)) / th2 (1 and 0.5 when th2 < 1e-20), E = I + A [w]x + B [w]x^2 written out as E00 = 1 - B*(w1*w1 +
 * w2*w2), E01 = B*(w0*w1) - A*w2, E02 = B*(w0*w2) + A*w1, ...  R21 <- E R21 and t21 <- E t21 + d are, on the pose:
 *     R'[i][j] = (R[i][0]*E[j][0] + R[i][1]*E[j][1]) + R[i][2]*E[j][2];   t'[i] = t[i] - ((R'[i][0]*d0 + R'[i][1]*d1) + R'[i][2]*d2)
 * A step that is not finite keeps the previous pose and ends the refit.  There is no damping and no step control.
 * Afterwards match_error is written into EVERY device record [0, num_pts), *num_fit = the candidates that pass at
 * refine_thresh under the final pose and h_rt = that pose.  refine_loops == 0: h_rt equals h_ransac byte for byte.
 * Optional (may be NULL): best_loop, h_inliers [num_pts], h_drawn [6][num_loops] (record indices), h_all_rt
 * [12][num_loops], h_all_counts [num_loops].  The same seed gives the same bytes in every output and in the records.
 * DEGENERATE ANSWERS, CUSIFT_OK: num_pts < 6, fewer than 6 candidates, or a winner that counts nothing (no hypothesis was
 * solvable): [I | 0] in both matrices, every count 0 except *num_candidates (0 when num_pts < 6: nothing is marked), the
 * optional arrays zeroed; the records are untouched.
 * KNOWN LIMIT: a coplanar point set makes the null space of the DLT system more than one-dimensional.  The call still
 * answers CUSIFT_OK with a rotation that is orthonormal to rounding, and makes no promise about the pose: planar scenes
 * belong to cusift_register_planar.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing written): every case of cusift_estimate_fundamental; a NULL camera2, fx or
 * fy zero or not finite, cx, cy or origin not finite; a NULL h_rt / h_ransac / num_candidates / num_matches / num_fit.
 * No other byte of any record than match_error changes; coords3D is read, never written.
 * Scratch lives in the context and grows on demand.  Blocking: ONE stream synchronisation, at the one read-back. */
int cusift_estimate_pnp(cusift_ctx *ctx, cusift_point *d_sift, int num_pts, int num_pts2 /* < 0: no check */, int rule,
                        float lo, float hi, const cusift_camera *camera2, int num_loops, float thresh, int refine_loops,
                        float refine_thresh, uint64_t seed, double h_rt[12], double h_ransac[12], int *num_candidates,
                        int *num_matches, int *num_fit, int *best_loop /* may be NULL */,
                        char *h_inliers /* may be NULL */, int *h_drawn /* may be NULL */,
                        double *h_all_rt /* may be NULL */, int *h_all_counts /* may be NULL */);

/* cusift_match(d_sift1, d_sift2, distance) followed by cusift_estimate_pnp(d_sift1, num_pts1, num_pts2, ...) with ONE
 * synchronisation, at the read-back: the same bytes as the staged route in every output and in the records.  The matcher
 * leaves coords3D of both record sets alone.  Also CUSIFT_ERR_INVALID for an unknown distance.  It honours
 * cusift_ctx_set_cross_check exactly as cusift_register_epipolar does: while it is on, the matcher is
 * cusift_match_mutual, THE MATCH FIELDS OF d_sift2 ARE WRITTEN (the parameter keeps its const spelling), overlapping
 * record ranges are refused with CUSIFT_ERR_INVALID before anything is enqueued or written, and a record that is not
 * mutual is no candidate. */
int cusift_register_pnp(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2, int num_pts2,
                        int distance, int rule, float lo, float hi, const cusift_camera *camera2, int num_loops,
                        float thresh, int refine_loops, float refine_thresh, uint64_t seed, double h_rt[12],
                        double h_ransac[12], int *num_candidates, int *num_matches, int *num_fit,
                        int *best_loop /* may be NULL */, char *h_inliers /* may be NULL */,
                        int *h_drawn /* may be NULL */, double *h_all_rt /* may be NULL */,
                        int *h_all_counts /* may be NULL */);

/* Writes coords3D of every record from its coords2D = (x, y) (0-based pixels at base-image scale) and the depth image
 * of its frame, all in fp32:
 *     u = roundf(x), v = roundf(y);  not finite or outside [0, width) x [0, height)  ->  (0, 0, 0)
 *     r = depth[v][u];  encoding 1: r = (r >> 3) | (r << 13) in 16 bits;  r == 0  ->  (0, 0, 0)
 *     z = (float)r / units_per_metre;  X = ((u + origin) - cx) * z / fx;  Y = ((v + origin) - cy) * z / fy
 * z == 0 is the "no depth" mark that MatchSiftData(..., MatchType3D) and cusift_select_matches test.  The batch is laid
 * out like the output of cusift_extract_batch: d_points[n_images][max_pts], frame k's depth image at d_depth +
 * k * image_stride_elems, rows pitch_elems samples apart.  d_counters (may be NULL: every frame has max_pts records)
 * gives the records per frame; records past the count and every byte of a record other than coords3D are untouched.
 * Asynchronous on the context's stream. */
int cusift_lift_depth(cusift_ctx *ctx, cusift_point *d_points, const unsigned int *d_counters /* or NULL */, int n_images,
                      int max_pts, const uint16_t *d_depth, int width, int height, int pitch_elems,
                      size_t image_stride_elems, const cusift_camera *camera);

/* The threshold filter of MatchSiftData (extras/matching.cu:318-349) on the device, after cusift_match: record i of
 * d_sift1 is kept iff score < score_thresh^2, ambiguity < ambiguity_thresh^2, 0 <= match < num_pts2 and, for type 1
 * (MatchType3D), coords3D[2] != 0 in the record and in its partner d_sift2[match].  In ASCENDING i (the order of the
 * reference's host loop): d_pairs[k] = (i, match), d_coord[k] = coords3D of record i, then of its partner -- the
 * [n][6] rows cusift_estimate_rigid takes -- and *d_count = the number kept.  d_pairs [num_pts1][2], d_coord
 * [num_pts1][6] and d_count are device memory; rows past the count are not written.  No atomics: the same input gives
 * the same output.  Asynchronous on the context's stream. */
int cusift_select_matches(cusift_ctx *ctx, const cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                          int num_pts2, float score_thresh, float ambiguity_thresh, int type /* 0 = 2D, 1 = 3D */,
                          int *d_pairs, float *d_coord, int *d_count);
/* cusift_select_matches with the cross-check as one more condition: record i is kept only if, besides the above,
 * d_sift2[match].match == i (the fields as they stand, whatever wrote them: cusift_match_mutual, or cusift_match in both
 * directions).  The same outputs, order, argument checks and absence of atomics. */
int cusift_select_mutual(cusift_ctx *ctx, const cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                         int num_pts2, float score_thresh, float ambiguity_thresh, int type /* 0 = 2D, 1 = 3D */,
                         int *d_pairs, float *d_coord, int *d_count);
/* The selection behind cusift_ctx_set_keep_strongest (cusift_amd.h has the total order) as a stage of its own, on lists
 * of 64-byte record heads (the first 16 floats of a cusift_point: coords2D .. subsampling) as the staged detections leave them.
 * d_heads is [list][image][capacity] x 64 B; d_counts is [list][image]: on input the counts held (the call clamps them at
 * `capacity`), on output the counts kept.  Per image the `keep` (>= 1) first heads of all its lists together survive, each
 * list compacted to its kept heads in unspecified order -- heads at and beyond a list's new count hold nothing in
 * particular -- and d_kept[image] = min(keep, heads held).  Uses the context's arena as scratch (8 bytes per head of
 * capacity); asynchronous on the context's stream: the call does not synchronise. */
int cusift_select_strongest(cusift_ctx *ctx, void *d_heads, int n_lists, int n_images, int capacity,
                            unsigned int *d_counts, int keep, unsigned int *d_kept);

/* The cross-check of the registrations, a setting of the context (0 = off, the default; 1 = on; anything else:
 * CUSIFT_ERR_INVALID, the setting unchanged).  It affects cusift_register_planar, cusift_register_rgbd,
 * cusift_register_planar_batch, cusift_register_rgbd_batch, cusift_register_epipolar, cusift_register_pose,
 * cusift_register_pnp and their pair-list forms (cusift_register_epipolar_batch, _pose_batch, _pnp_batch) and nothing else; with 0 they enqueue the launches and
 * return the bytes they always did.  With 1, record i of frame 1 takes part only if it is MUTUAL: its match m lies in
 * [0, n2) and the column side's best for record m of frame 2 is i -- the column side exactly as cusift_match_mutual /
 * cusift_match_batch_mutual define it, so an exactly tied best keeps the lowest record of frame 1.  Every many-to-one
 * match but one drops out before RANSAC draws.  The pair calls enqueue cusift_match_mutual in place of cusift_match
 * (both record sets' match fields are written; overlapping ranges are refused before anything is enqueued), the planar
 * marking drops a non-mutual record from the candidates and from the refit set under either rule, and the RGB-D
 * selection is cusift_select_mutual's.  The pair-list forms take the column side from cusift_match_batch_mutual's back
 * rows, kept in the context's scratch behind everything that is read back: the records stay unwritten, (a, a) stays legal
 * (every record is then its own mutual match), a pair with an empty frame has no candidate as before, and pair p has the
 * bits of the pair call with the setting on and seed + p.  Still one synchronisation, one read-back and no count read
 * back; one more launch (the column merge) when a frame 1 has more than 64 record slots.  Scratch: the batch matcher's
 * column partials take 12 bytes x n_pairs x ceil(max_pts / 64) x max_pts -- quadratic in max_pts: 12.7 GB for 64 frames
 * (63 consecutive pairs) at max_pts 32768, 0.8 GB at 8192 -- plus 16 bytes x n_pairs x max_pts of back rows. */
int cusift_ctx_set_cross_check(cusift_ctx *ctx, int on);

/* The descriptors the registrations match on, a setting of the context: 32 (the default, the float descriptors) or 8
 * (bytes, on the int8 matrix pipe); anything else: CUSIFT_ERR_INVALID, the setting unchanged.  It affects the calls
 * cusift_ctx_set_cross_check affects and nothing else: cusift_match, cusift_match_mutual, cusift_match_guided, the
 * cusift_match8* calls, cusift_find_homography and cusift_estimate_* do not read it.  With 32 every call enqueues exactly
 * what it always did.  With 8:
 *   - a pair call quantises both record sets into scratch the context owns (two quantiser launches; tables 16-byte, sums
 *     8-byte aligned; grown on demand as the other scratch blocks are) and enqueues cusift_match8 -- with the cross-check
 *     on, cusift_match8_mutual -- in place of cusift_match / cusift_match_mutual;
 *   - a pair-list call quantises the batch once (ONE launch over the frames the list names, honouring d_counters) and
 *     enqueues cusift_match8_batch -- with the cross-check on, cusift_match8_batch_mutual -- which writes the same
 *     cusift_match_row rows.  Everything behind the matcher (marking, selection, RANSAC, refit, read-back) is unchanged.
 * CONTRACT.  With 8 and the cross-check off a registration returns, bit for bit, what this sequence returns with the same
 * seed: cusift_quantize_descriptors on both sets, cusift_match8, and the staged cusift_estimate_* (for RGB-D:
 * cusift_select_matches + cusift_estimate_rigid).  With the cross-check on it is cusift_match8_mutual plus the mutual
 * condition of cusift_ctx_set_cross_check, and d_sift2's match fields are written as cusift_match8_mutual writes them.
 * Pair p of a batch has the bits of the pair call at seed + p.  Still one synchronisation and no count read back, and the
 * number of launches does not depend on the pair list. */
int cusift_ctx_set_match_bits(cusift_ctx *ctx, int bits);

/* Frame-to-frame registration of an RGB-D pair, device-resident from SiftData + depth to [R | t]: cusift_lift_depth
 * of both frames (one width x height image each, rows pitch_elems apart), cusift_match(distance), the 3-D selection
 * above and the RANSAC + refit of cusift_estimate_rigid over the selected pairs, drawn from `seed` -- sampling, tie
 * rule and refit exactly as documented there, reading the points and their number from device memory.  The result
 * maps frame 2 into frame 1: x1 ~ R x2 + t.  The same bits as the staged route (lift, match, select, read back,
 * cusift_estimate_rigid with the same seed).  *num_matches = selected pairs, *num_inliers = the winner's count,
 * h_pairs [num_matches][2] (capacity num_pts1) and h_inliers [num_matches] (capacity num_pts1) may be NULL.  Fewer
 * than 3 selected pairs (2 for rigid_type 0): h_rt = identity, *num_inliers = 0, CUSIFT_OK.  The match fields and
 * coords3D of d_sift1 and coords3D of d_sift2 are written as by the staged calls.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing of the caller's written): NULL h_rt / num_matches / num_inliers /
 * camera, fx or fy 0 or not finite, units_per_metre not > 0, an unknown encoding / distance / rigid_type, num_loops
 * < 1, thresh2 not > 0, a NaN threshold, missing buffers, pitch_elems < width.
 * Blocking: ONE stream synchronisation, at the final read-back; no host decision between the stages. */
int cusift_register_rgbd(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const uint16_t *d_depth1,
                         cusift_point *d_sift2, int num_pts2, const uint16_t *d_depth2, int width, int height,
                         int pitch_elems, const cusift_camera *camera, int distance, float score_thresh,
                         float ambiguity_thresh, int num_loops, float thresh2, int rigid_type /* 0 = 2D, 1 = 3D */,
                         uint64_t seed, float h_rt[12], int *num_matches, int *num_inliers,
                         int *h_pairs /* may be NULL */, char *h_inliers /* may be NULL */);

/* ---- the same over a sequence: a batch of frames and a pair list (sift_sequence.hip) ----------------------------- */
/* The reference registers sequences -- main.cpp: compareMatchingWithMATLAB walks its frames i -> i + 1, test/test.cpp
 * registers SUN3D frames -- one MatchSiftData (extras/matching.cu:232-362) and one EstimateRigidTransformH
 * (extras/rigidTransform.cu:388-520) per pair.  The calls below take the layout cusift_extract_batch produces,
 * d_points[n_images][max_pts] + d_counters[n_images], and a list of frame pairs, and do every pair in the same launches.
 *
 * One row of cusift_match_batch: the fields FindMinCorr / FindMaxCorr compute (extras/matching.cu:140-150,219-229),
 * kept out of the records so that a frame can be the first member of any number of pairs. */
typedef struct {
  float score, ambiguity;
  int match;
  int reserved; /* written as 0 */
} cusift_match_row;

/* cusift_match over a pair list: h_pairs[p] = (frame 1, frame 2), host memory, read before the call returns (keep it
 * valid until the stream has passed the call if it is page-locked).  For pair p and every record i of frame 1,
 * d_rows[p * max_pts + i] = score, ambiguity and match (an index into frame 2) exactly as cusift_match would write them
 * into record i: the same dot products in the same order, the same double-precision 1e-6 in the ambiguity; only between
 * columns whose best scores are exactly equal may `match` name another one of them.  The records per frame are
 * min(d_counters[frame], max_pts), read on the device (d_counters == NULL: max_pts each); rows past frame 1's count are
 * not written, and a pair whose frame 2 has no record writes no row (extras/matching.cu:241-242).  The records are not
 * written at all.  A frame may appear in any number of pairs, on either side; (a, a) is legal.  d_rows: device memory,
 * [n_pairs][max_pts], 16-byte aligned.
 * CUSIFT_ERR_INVALID (nothing enqueued): a pair index outside [0, n_images), n_pairs or n_images outside [0, 65535],
 * max_pts outside [0, 2^20], a NULL h_pairs with n_pairs > 0, an unknown distance, missing buffers.  n_pairs == 0 or
 * max_pts == 0: CUSIFT_OK, nothing enqueued.  Asynchronous on the context's stream. */
int cusift_match_batch(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters /* or NULL */,
                       int n_images, int max_pts, const int *h_pairs /* [n_pairs][2] */, int n_pairs, int distance,
                       cusift_match_row *d_rows);

/* cusift_match_batch with both directions from one pass (cusift_match_mutual over a pair list).  d_rows is exactly what
 * cusift_match_batch writes.  d_rows_back[p * max_pts + j] = score, ambiguity and match (an index into frame 1) of
 * record j of pair p's frame 2 by the column-side model of cusift_match_mutual over the records of frame 1 (lowest row on
 * exactly tied best scores; independent of the split count).  Rows past frame 2's count are not written, and a pair whose
 * frame 1 has no record writes no back row.  The records are not written; (a, a) is legal.  The counts are read on the
 * device and the launch count does not depend on the list.  d_rows_back: device memory, [n_pairs][max_pts], 16-byte
 * aligned, distinct from d_rows.
 * CUSIFT_ERR_INVALID (nothing enqueued): every case of cusift_match_batch, and a NULL d_rows_back. */
int cusift_match_batch_mutual(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters /* or NULL */,
                              int n_images, int max_pts, const int *h_pairs /* [n_pairs][2] */, int n_pairs, int distance,
                              cusift_match_row *d_rows, cusift_match_row *d_rows_back);

/* cusift_match_batch under one model per pair (cusift_match_guided over a pair list): pair p's rows are what
 * cusift_match_batch writes for it with cusift_match_guided's rule added, under the model h_models[9 p .. 9 p + 8] -- all
 * pairs the same kind of `model` and the same radius.  h_models is host memory and is read before the call returns, as
 * h_pairs is; the device copy lives in the context's scratch.  Rows, counts and launches as cusift_match_batch; the
 * records are not written.
 * CUSIFT_ERR_INVALID (nothing enqueued): every case of cusift_match_batch, an unknown model, a NULL h_models, radius not
 * > 0 (NaN included). */
int cusift_match_batch_guided(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters /* or NULL */,
                              int n_images, int max_pts, const int *h_pairs /* [n_pairs][2] */, int n_pairs, int distance,
                              int model, const double *h_models /* [n_pairs][9] */, float radius,
                              cusift_match_row *d_rows);

/* cusift_match_batch under one pose per pair (cusift_match_projected over a pair list): pair p's rows are what
 * cusift_match_batch writes for it with cusift_match_projected's rule added, under the pose h_rts[12 p .. 12 p + 11] --
 * X1 = R X2 + t with frame 1 = the pair's first member, whose coords3D are read -- all pairs under the same camera2 and
 * the same radius.  h_rts and camera2 are host memory and are read before the call returns, as h_pairs is; the device
 * copy lives in the context's scratch.  Rows, counts and launches as cusift_match_batch; the records are not written.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing written): every case of cusift_match_batch, a NULL h_rts or camera2, fx
 * or fy zero or not finite, cx, cy or origin not finite, radius not > 0 (NaN included). */
int cusift_match_batch_projected(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters /* or NULL */,
                                 int n_images, int max_pts, const int *h_pairs /* [n_pairs][2] */, int n_pairs,
                                 int distance, const double *h_rts /* [n_pairs][12] */, const cusift_camera *camera2,
                                 float radius, cusift_match_row *d_rows);

/* ---- 8-bit descriptors: quantised on the device, matched on the int8 matrix pipe ------------------------------------
 * The byte descriptor is what OpenCV, VLFeat and COLMAP store and exchange: 128 unsigned bytes per keypoint, 512 v clipped
 * to 255 ("8-bit descriptors").  A TABLE here is unsigned char [n][128], dense (record i at byte 128 i)
 * and 16-byte aligned, with int sums[n][2] = (sum of q, sum of q * q) over the record's 128 bytes beside it, 8-byte
 * aligned.  Integer scores are exact: every output below is pinned bit for bit by a few lines of integer arithmetic.
 *
 * cusift_quantize_descriptors: d_points[n_images][max_pts] + d_counters[n_images] as cusift_extract_batch leaves them
 * (d_counters == NULL: max_pts records each, as cusift_lift_depth; counts are clamped to max_pts on the device) ->
 * d_q[n_images][max_pts][128] and d_sums[n_images][max_pts][2].  Per element v = data[k], in fp32, pinned to these
 * expressions (the build uses -ffp-contract=off):
 *     t = 512.0f * v                                   (exact)
 *     u = t + 0.5f                                     (one rounding)
 *     q = (v > 0) ? (u < 255.0f ? (int)u : 255) : 0    ((int) truncates)
 * so NaN, zeros and negatives give 0, +infinity and anything at or above 255/512 give 255.  Rows past a frame's count
 * are not written.  One launch, no read-back, asynchronous on the context's stream; the records are not written.
 * CUSIFT_ERR_INVALID (nothing enqueued): n_images outside [0, 65535], max_pts outside [0, 2^24], missing buffers, a d_q
 * that is not 16-byte aligned, a d_sums that is not 8-byte aligned.  n_images == 0 or max_pts == 0: CUSIFT_OK. */
int cusift_quantize_descriptors(cusift_ctx *ctx, const cusift_point *d_points, const unsigned int *d_counters /* or NULL */,
                                int n_images, int max_pts, unsigned char *d_q, int *d_sums);
/* The same two sums for n byte descriptors that came from somewhere else (a COLMAP or OpenCV database): d_sums[i] =
 * (sum q, sum q * q) of d_q[i][0..128).  n <= 0: CUSIFT_OK, nothing enqueued.  Refusals as above. */
int cusift_desc8_sums(cusift_ctx *ctx, const unsigned char *d_q, int n, int *d_sums);
/* cusift_match on two tables: writes score, ambiguity, match, match_xpos, match_ypos of d_sift1[0 .. num_pts1) and nothing
 * else; d_sift2 is read only for coords2D of the match (of record 0 when match is outside [0, num_pts2), as cusift_match).
 * The descriptors of the records themselves are not read: row i is d_q1[i], column j is d_q2[j].
 * SCORES, all integers: S = sum_k q1[k] * q2[k];  for distance 1 the key of column j is D = sum q1^2 + sum q2^2 - 2 S (the
 * two sums from the sums tables) and its score is (float)D * 2^-18; for distance 0 the key is -S and the score is
 * (float)S * 2^-18.  Both integers stay below 2^24 (128 * 255^2 = 8,323,200), so the floats are exact.
 * MODEL: match = the LOWEST column with the smallest key; score = that column's score; second = the score of the second
 * smallest key of the multiset of all columns' keys, so a tie for best gives second == best; with a single column second
 * is cusift_match's initial value, 999 for distance 1 and -1 for distance 0.  ambiguity, cusift_match's two expressions
 * unchanged (the 1e-6 is a double): distance 1: (float)(best / (second + 1e-6)); distance 0: (float)((1 - best) / (1 -
 * second + 1e-6)).
 * The model does not depend on scan order, tile or split count: the same input gives the same bytes under every
 * CUSIFT_POLICY_MATCH_SPLITS (honoured: k > 0 asks for k column splits, at most one per 64 columns), there are no atomics,
 * and every merge breaks ties on the lower column -- with integer keys exact ties are ordinary.
 * QUANTISED DESCRIPTORS ARE NOT UNIT VECTORS (sum (q / 512)^2 is near 1, not 1), so for distance 0 `1 - best` can be
 * slightly negative and the ambiguity with it; the formula is the reference's, verbatim.  Distance 1 is the mode to use.
 * A count <= 0 on either side: CUSIFT_OK, nothing enqueued.  CUSIFT_ERR_INVALID (nothing enqueued): a NULL pointer, a
 * table that is not 16-byte aligned, a sums table that is not 8-byte aligned, a distance other than 0 or 1.  Asynchronous
 * on the context's stream; per-split scratch (16 bytes per split and row) lives in the context. */
int cusift_match8(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const unsigned char *d_q1, const int *d_sums1,
                  const cusift_point *d_sift2, int num_pts2, const unsigned char *d_q2, const int *d_sums2, int distance);
/* cusift_match8 over a pair list, on the tables cusift_quantize_descriptors writes for a batch: the contract of
 * cusift_match_batch (pairs, counts read on the device and clamped to max_pts, the grid sized from max_pts, rows past
 * frame 1's count not written, no row for a pair whose frame 2 is empty, (a, a) legal, the same refusals) with
 * cusift_match8's model: d_rows[p * max_pts + i] = score, ambiguity and match exactly as cusift_match8 writes them for
 * the tables of pair p's two frames.  Also refused: misaligned tables. */
int cusift_match8_batch(cusift_ctx *ctx, const unsigned char *d_q, const int *d_sums,
                        const unsigned int *d_counters /* or NULL */, int n_images, int max_pts,
                        const int *h_pairs /* [n_pairs][2] */, int n_pairs, int distance, cusift_match_row *d_rows);
/* cusift_match8 with both directions from one pass over the integer scores.  Set 1 (d_sift1) receives exactly the bytes
 * cusift_match8 writes.  Set 2 receives the same five fields for each of its records j, over the records of set 1 -- THE
 * COLUMN SIDE, expression by expression:
 *     key(i, j) = the same exact integer as on the row side: D = sum_k (q1[i][k] - q2[j][k])^2 for distance 1, -S for 0;
 *     match     = the LOWEST row i with the smallest key(., j);
 *     score     = (float)D * 2^-18, or (float)S * 2^-18, of that row;
 *     second    = the score of the second smallest key of the multiset {key(i, j) : i}, so a tied best gives second ==
 *                 best; with num_pts1 == 1 it is cusift_match's initial value, 999 for distance 1 and -1 for distance 0;
 *     ambiguity = cusift_match8's two expressions on (score, second), unchanged;
 *     match_xpos, match_ypos = coords2D of d_sift1[match].
 * The keys are symmetric integers, so THE FIELDS OF SET 2 AFTER cusift_match8_mutual(A, B) EQUAL, BYTE FOR BYTE, THE
 * FIELDS OF SET 1 AFTER cusift_match8(B, A), and set 1's equal cusift_match8(A, B)'s.  Every merge orders (key, row)
 * pairs: the same bytes on every run, for every grid and under every CUSIFT_POLICY_MATCH_SPLITS; there are no atomics.
 * A count <= 0 on either side: CUSIFT_OK, nothing enqueued, nothing written.  CUSIFT_ERR_INVALID (nothing enqueued): every
 * case of cusift_match8, and record ranges that overlap (both are written), as cusift_match_mutual.  Scratch in the
 * context: cusift_match8's, plus -- with more than 256 records in set 1 -- column partials of
 * 16 B x ceil(num_pts1 / 256) x num_pts2, folded by one more launch. */
int cusift_match8_mutual(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const unsigned char *d_q1, const int *d_sums1,
                         cusift_point *d_sift2, int num_pts2, const unsigned char *d_q2, const int *d_sums2, int distance);
/* cusift_match8_batch with the column side: d_rows is exactly what cusift_match8_batch writes; d_rows_back[p * max_pts +
 * j] = score, ambiguity and match (an index into frame 1) of record j of pair p's frame 2 by the column side above, over
 * the tables of pair p's two frames.  Rows past frame 2's count are not written, and a pair with an empty frame writes no
 * row on either side.  (a, a) is legal; the launch count does not depend on the list.  d_rows_back: device memory,
 * [n_pairs][max_pts], 16-byte aligned, distinct from d_rows.  CUSIFT_ERR_INVALID (nothing enqueued): every case of
 * cusift_match8_batch, a NULL d_rows_back, d_rows_back == d_rows.  Scratch in the context: cusift_match8_batch's, plus
 * -- with max_pts > 256 -- column partials of 16 B x n_pairs x ceil(max_pts / 256) x max_pts. */
int cusift_match8_batch_mutual(cusift_ctx *ctx, const unsigned char *d_q, const int *d_sums,
                               const unsigned int *d_counters /* or NULL */, int n_images, int max_pts,
                               const int *h_pairs /* [n_pairs][2] */, int n_pairs, int distance, cusift_match_row *d_rows,
                               cusift_match_row *d_rows_back);
/* 8-bit guided matching: cusift_match8 with one more rule -- the geometric predicate of cusift_match_guided (H or F) or of
 * cusift_match_projected (a pose and coords3D), evaluated inside the int8 matcher's update.  The second matching pass of a
 * registration, and a tracker's search against a map, for callers who keep bytes.
 * THE TEST is cusift_match_guided's for `model` = CUSIFT_GUIDE_HOMOGRAPHY / CUSIFT_GUIDE_EPIPOLAR and
 * cusift_match_projected's for the projected call: exactly the expressions pinned there -- fp64 per row, fp32 per pair,
 * the same parenthesisation, the same conventions, -ffp-contract=off -- on x1 = coords2D (X1 = coords3D) of RECORD i of
 * d_sift1 and x2 = coords2D of RECORD j of d_sift2.  The coordinates come from the records, the descriptors from the
 * tables: row i is d_q1[i], column j is d_q2[j], as in cusift_match8.  A NaN anywhere is no pass.
 * THE RESULT, over the set P(i) of the columns that pass against row i, with cusift_match8's exact integer keys (D for
 * distance 1, -S for distance 0) and its scores:
 *     match  = the LOWEST column of the passing set P(i) with the smallest key;   score = that column's score;
 *     second = the score of the second smallest key of the multiset {key(i, j) : j in P(i)}, so a tied best among the
 *              passing columns gives second == best;
 *     EXACTLY ONE passing column: second = cusift_match's initial value, 999 for distance 1 and -1 for distance 0 (a
 *              tiny ambiguity: the only compatible partner, as cusift_match_guided says);
 *     NO COLUMN PASSES: match = -1, score = the initial value, the ambiguity that two initial values give (999 / (999 +
 *              1e-6), or 2 / (2 + 1e-6)) and match_xpos / match_ypos of record 0 -- exactly as cusift_match_guided
 *              documents;
 *     ambiguity, match_xpos, match_ypos otherwise: cusift_match8's expressions on (score, second) and coords2D of
 *              d_sift2[match].
 * A column that fails changes nothing for that row, whatever its key and its index: a failing column with a smaller or
 * an equal key than the winner, below or above it, is as if it were not there.  The same input gives the same bytes under
 * every CUSIFT_POLICY_MATCH_SPLITS -- a row whose passing columns all lie in one split, or in none, included; there are
 * no atomics.  With a radius that every pair passes (1e6 on finite coordinates under a mild model; +infinity, which is
 * legal) the bytes are cusift_match8's.
 * Writes the five fields cusift_match8 writes and nothing else; the records' coords2D and coords3D are read, never
 * written.  A count <= 0 on either side: CUSIFT_OK, nothing enqueued, nothing written.  CUSIFT_ERR_INVALID (nothing
 * enqueued, nothing written): every case of cusift_match8, and every case cusift_match_guided (an unknown model, a NULL
 * h_model, radius not > 0, NaN included) or cusift_match_projected (a NULL h_rt or camera2, a camera that
 * cusift_estimate_pnp refuses, radius not > 0) adds.  A model or a pose that is not finite is no error: it passes
 * nothing, and every row gets the "no column passes" answer.  h_model / h_rt / camera2 are read before the call returns.
 * Asynchronous on the context's stream; scratch as cusift_match8. */
int cusift_match8_guided(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const unsigned char *d_q1, const int *d_sums1,
                         const cusift_point *d_sift2, int num_pts2, const unsigned char *d_q2, const int *d_sums2,
                         int distance, int model, const double h_model[9], float radius);
int cusift_match8_projected(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const unsigned char *d_q1,
                            const int *d_sums1, const cusift_point *d_sift2, int num_pts2, const unsigned char *d_q2,
                            const int *d_sums2, int distance, const double h_rt[12], const struct cusift_camera *camera2,
                            float radius);
/* The same two over a pair list: cusift_match8_batch with cusift_match8_guided's / cusift_match8_projected's rule, pair p
 * under h_models[9 p .. 9 p + 8] or h_rts[12 p .. 12 p + 11] -- one kind of model, one camera and one radius for the list.
 * d_points[n_images][max_pts] are the records the tables were quantised from: the test reads coords2D (coords3D of the
 * pair's first frame) there, the tables carry only bytes; the records are const and are never written.  d_rows[p *
 * max_pts + i] = score, ambiguity and match exactly as the pair call writes them for pair p's records and tables; rows
 * past frame 1's count are not written, a pair whose frame 2 is empty writes no row, (a, a) is legal.  The models are host
 * memory, read before the call returns; the device copy lives in the context's scratch.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing written): every case of cusift_match8_batch and of cusift_match_batch_guided
 * / cusift_match_batch_projected -- the model, pose, camera and radius are checked for an empty list too -- and a NULL
 * d_points with a list and a capacity that are not zero. */
int cusift_match8_batch_guided(cusift_ctx *ctx, const cusift_point *d_points, const unsigned char *d_q, const int *d_sums,
                               const unsigned int *d_counters /* or NULL */, int n_images, int max_pts,
                               const int *h_pairs /* [n_pairs][2] */, int n_pairs, int distance, int model,
                               const double *h_models /* [n_pairs][9] */, float radius, cusift_match_row *d_rows);
int cusift_match8_batch_projected(cusift_ctx *ctx, const cusift_point *d_points, const unsigned char *d_q, const int *d_sums,
                                  const unsigned int *d_counters /* or NULL */, int n_images, int max_pts,
                                  const int *h_pairs /* [n_pairs][2] */, int n_pairs, int distance,
                                  const double *h_rts /* [n_pairs][12] */, const struct cusift_camera *camera2, float radius,
                                  cusift_match_row *d_rows);
/* The pair calls for a caller with records alone (the second matching pass of a guided registration on bytes: a
 * cusift_register_* call while cusift_ctx_set_match_bits is 8, one of these under its model, the cusift_estimate_* call --
 * what the Python chains register_*_guided(match8=True) run):
 * cusift_quantize_descriptors of both record sets into tables in the context's scratch,
 * then cusift_match8_guided / cusift_match8_projected on them -- the same bytes as that staged route on tables of the
 * caller's.  Refusals and empty counts: cusift_match_guided's / cusift_match_projected's.  Three launches (four with
 * split columns), asynchronous. */
int cusift_match8_guided_records(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                                 int num_pts2, int distance, int model, const double h_model[9], float radius);
int cusift_match8_projected_records(cusift_ctx *ctx, cusift_point *d_sift1, int num_pts1, const cusift_point *d_sift2,
                                    int num_pts2, int distance, const double h_rt[12], const struct cusift_camera *camera2,
                                    float radius);

/* cusift_register_rgbd for every pair of a list, device-resident from the extractor's batch + depth images to one
 * [R | t] per pair: ONE cusift_lift_depth over all frames (frame k's depth image at d_depth + k * image_stride_elems),
 * cusift_match_batch, the 3-D selection of cusift_select_matches per pair, and the RANSAC + refit of
 * cusift_estimate_rigid per pair -- sampling, tie rule and refit exactly as documented there, pair p drawing from
 * seed + p (64-bit, wrapping).  Pair p = (a, b) maps frame b into frame a: x_a ~ R x_b + t, h_rt[12 p .. 12 p + 11].
 * Every output of pair p has the bits cusift_register_rgbd(frame a, frame b, ..., seed + p) returns.  h_num_matches[p]
 * = selected matches, h_num_inliers[p] = the winner's count; h_sel_pairs ([n_pairs][max_pts][2], may be NULL) and
 * h_inliers ([n_pairs][max_pts], may be NULL) receive the first h_num_matches[p] entries of pair p's block, the rest of
 * a block is not written.  Fewer than 3 selected matches (2 for rigid_type 0), an empty frame included: identity, 0
 * inliers, CUSIFT_OK.  Of the records only coords3D is written.  A frame may appear in any number of pairs, on either
 * side; (a, a) is legal.  The launch count does not depend on n_pairs, and the host takes no decision between the
 * stages.  Scratch lives in the context and grows on demand.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing of the caller's written): every case of cusift_register_rgbd -- NULL
 * h_rt / h_num_matches / h_num_inliers / camera, fx or fy 0 or not finite, units_per_metre not > 0, an unknown encoding
 * / distance / rigid_type, num_loops < 1, thresh2 not > 0, a NaN threshold, missing buffers, pitch_elems < width --
 * and: image_stride_elems smaller than one image (n_images > 1), a pair index outside [0, n_images), n_pairs or
 * n_images outside [0, 65535], max_pts outside [0, 2^20], a NULL h_pairs with n_pairs > 0.  n_pairs == 0: CUSIFT_OK,
 * nothing enqueued.
 * Blocking: ONE stream synchronisation, at the one read-back. */
int cusift_register_rgbd_batch(cusift_ctx *ctx, cusift_point *d_points, const unsigned int *d_counters /* or NULL */,
                               int n_images, int max_pts, const uint16_t *d_depth, int width, int height,
                               int pitch_elems, size_t image_stride_elems, const cusift_camera *camera,
                               const int *h_pairs /* [n_pairs][2]: (frame 1, frame 2) */, int n_pairs, int distance,
                               float score_thresh, float ambiguity_thresh, int num_loops, float thresh2,
                               int rigid_type /* 0 = 2D, 1 = 3D */, uint64_t seed, float *h_rt /* [n_pairs][12] */,
                               int *h_num_matches, int *h_num_inliers, int *h_sel_pairs /* may be NULL */,
                               char *h_inliers /* may be NULL */);

/* cusift_register_planar for every pair of a list: the extractor's batch and a pair list in, one homography per pair out,
 * in a number of launches that does not depend on n_pairs and with no host decision between the stages.  Pair p = (a, b)
 * maps frame a's coords2D onto frame b: h_homography[9 p .. 9 p + 8] (refined), h_ransac[9 p .. 9 p + 8] (the winner).
 * The records per frame are min(d_counters[frame], max_pts), read on the device (d_counters == NULL: max_pts each); no
 * count reaches the host before the one read-back.  A frame may appear in any number of pairs, on either side; (a, a) is
 * legal.  Pair p draws from seed + p (64-bit, wrapping).
 * STAGES: cusift_match_batch into rows in the context's scratch; a marking kernel that builds each pair's coordinates,
 * candidates and refit set from its rows and from coords2D of frame a's records and of their partners in frame b (the
 * value cusift_match puts into match_xpos / match_ypos); then the compaction, the drawing solver, the scoring and the
 * selection + refit of cusift_estimate_homography with one grid layer per pair.
 * THE RECORDS ARE NEVER WRITTEN.  match_error = sqrtf(err) of every record of frame a goes to h_match_error
 * ([n_pairs][max_pts], may be NULL) and the winner's inlier flags to h_inliers ([n_pairs][max_pts], may be NULL): the
 * first count_a entries of pair p's block, the rest of a block is not written.
 * EQUALITY: every output of pair p has the bits of the staged route -- pair p's row of cusift_match_batch scattered into a
 * copy of frame a's records (score, ambiguity, match, match_xpos / match_ypos = the partner's coords2D), then
 * cusift_estimate_homography(copy, count_a, count_b, rule, lo, hi, ..., seed + p); h_match_error is the match_error that
 * call writes.  Where the rows equal what cusift_match writes (cusift_match_batch documents the one licence to differ:
 * exactly tied best scores) these are the bits of cusift_register_planar(frame a, frame b, ..., seed + p).
 * DEGENERATE PAIRS are decided on the device and disturb no other pair: count_a < 8 -- identity in both matrices, every
 * count 0, h_num_candidates[p] = 0; fewer than 8 candidates -- identity, counts 0, h_num_candidates[p] as counted;
 * count_b == 0 -- no row exists, 0 candidates.  Their flags are 0 and their block of h_match_error is not written (the
 * pair call leaves match_error alone).
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing written): every case of cusift_register_planar -- a NULL h_homography /
 * h_ransac / h_num_candidates / h_num_matches / h_num_fit, num_loops < 1, thresh or refine_thresh not > 0, a NaN lo / hi,
 * an unknown rule or distance, refine_loops < 0, missing buffers -- and: a pair index outside [0, n_images), n_pairs or
 * n_images outside [0, 65535], max_pts outside [0, 2^20], a NULL h_pairs with n_pairs > 0.  n_pairs == 0: CUSIFT_OK,
 * nothing enqueued.  Scratch lives in the context and grows on demand.
 * Blocking: ONE stream synchronisation, at the one read-back. */
int cusift_register_planar_batch(cusift_ctx *ctx, const cusift_point *d_points,
                                 const unsigned int *d_counters /* or NULL */, int n_images, int max_pts,
                                 const int *h_pairs /* [n_pairs][2]: (frame a, frame b) */, int n_pairs, int distance,
                                 int rule, float lo, float hi, int num_loops, float thresh, int refine_loops,
                                 float refine_thresh, uint64_t seed, float *h_homography /* [n_pairs][9] */,
                                 float *h_ransac /* [n_pairs][9] */, int *h_num_candidates, int *h_num_matches,
                                 int *h_num_fit, int *h_best_loop /* may be NULL */,
                                 char *h_inliers /* [n_pairs][max_pts], may be NULL */,
                                 float *h_match_error /* [n_pairs][max_pts], may be NULL */);

/* ---- the pair-list forms of the fundamental matrix, the calibrated pose and the absolute pose ---------------------- */
/* cusift_register_epipolar, cusift_register_pose and cusift_register_pnp for every pair of a list, with the contract of
 * cusift_register_planar_batch: the extractor's batch and a pair list in, one model per pair out, in a number of launches
 * that does not depend on n_pairs, with no host decision between the stages and no count read back.  The records per
 * frame are min(d_counters[frame], max_pts), read on the device (d_counters == NULL: max_pts each).  A frame may appear in
 * any number of pairs, on either side; (a, a) is legal.  What the three calls share:
 * SEED: pair p draws from seed + p (64-bit, wrapping).
 * STAGES: cusift_match_batch into rows in the context's scratch; a marking kernel that builds each pair's coordinates and
 * candidates from its rows, from frame a's records and from coords2D of their partners in frame b (the value cusift_match
 * puts into match_xpos / match_ypos); then the compaction, the drawing solver, the scoring and the selection + refit of
 * the pair call with one grid layer per pair.
 * THE RECORDS ARE NEVER WRITTEN.  match_error of every record of frame a goes to h_match_error ([n_pairs][max_pts], may
 * be NULL) and the winner's inlier flags to h_inliers ([n_pairs][max_pts], may be NULL): the first count_a entries of
 * pair p's block, the rest of a block is not written.
 * EQUALITY: every output of pair p has the bits of the staged route -- pair p's row of cusift_match_batch scattered into a
 * copy of frame a's records (score, ambiguity, match, match_xpos / match_ypos = the partner's coords2D), then
 * cusift_estimate_fundamental, cusift_estimate_pose on that F (thresh = refine_thresh), or cusift_estimate_pnp on the
 * copy, with count_a, count_b and seed + p; h_match_error is the match_error that call writes and h_points3d the coords3D
 * that cusift_estimate_pose writes.  Where the rows equal what cusift_match writes (cusift_match_batch documents the one
 * licence to differ: exactly tied best scores) these are the bits of cusift_register_epipolar, cusift_register_pose or
 * cusift_register_pnp(frame a, frame b, ..., seed + p).
 * DEGENERATE PAIRS are decided on the device, disturb no other pair and answer what the pair call answers: nine zeros in
 * both matrices (F), [I | 0], zero votes and zeros in h_points3d (pose), [I | 0] in both poses (PnP).  Every count is 0,
 * the flags are 0 and the pair's block of h_match_error is not written (the pair call leaves match_error alone).
 * h_num_candidates[p] = 0 when frame a has fewer records than the model's minimum -- 8 for F and the pose, 6 for PnP --
 * and the counted number otherwise (0 when frame b is empty: no row exists).  For PnP a winner that counts no point is
 * nothing to fit either, as in cusift_estimate_pnp: [I | 0], counts 0, h_num_candidates[p] as counted.
 * CROSS-CHECK: cusift_ctx_set_cross_check is honoured as in cusift_register_planar_batch -- the column side comes from
 * cusift_match_batch_mutual's back rows in the context's scratch, a record that is not mutual is no candidate, and pair p
 * has the bits of the pair call with the setting on and seed + p.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing written): every case of the pair call -- a NULL required output (the
 * two models and the three counts; for the pose also h_rt, h_num_front and camera1; for PnP camera2), fx or fy 0 or not
 * finite, cx / cy / origin not finite, num_loops outside [1, 2^24], thresh or refine_thresh not > 0, a NaN lo / hi, an
 * unknown rule or distance, refine_loops < 0, missing buffers -- and: a pair index outside [0, n_images), n_pairs or
 * n_images outside [0, 65535], max_pts outside [0, 2^20], a NULL h_pairs with n_pairs > 0.  n_pairs == 0: CUSIFT_OK,
 * nothing enqueued, nothing written.  max_pts == 0: every pair is degenerate, answered from the arguments alone.  Scratch
 * lives in the context and grows on demand.
 * Blocking: ONE stream synchronisation, at the one read-back.
 *
 * cusift_register_epipolar_batch: pair p = (a, b) gives x_b^T F x_a = 0, h_fundamental[9 p .. 9 p + 8] (refined) and
 * h_ransac[9 p .. 9 p + 8] (the winner), as cusift_estimate_fundamental defines them. */
int cusift_register_epipolar_batch(cusift_ctx *ctx, const cusift_point *d_points,
                                   const unsigned int *d_counters /* or NULL */, int n_images, int max_pts,
                                   const int *h_pairs /* [n_pairs][2]: (frame a, frame b) */, int n_pairs, int distance,
                                   int rule, float lo, float hi, int num_loops, float thresh, int refine_loops,
                                   float refine_thresh, uint64_t seed, double *h_fundamental /* [n_pairs][9] */,
                                   double *h_ransac /* [n_pairs][9] */, int *h_num_candidates, int *h_num_matches,
                                   int *h_num_fit, int *h_best_loop /* may be NULL */,
                                   char *h_inliers /* [n_pairs][max_pts], may be NULL */,
                                   float *h_match_error /* [n_pairs][max_pts], may be NULL */);

/* cusift_register_epipolar_batch followed, in the same call and before the one read-back, by the pose stage of
 * cusift_register_pose for every pair: one pair of cameras serves every pair of the list (camera2 == NULL: camera1 for both
 * views).  h_rt[12 p .. 12 p + 11] = [R | t] of pair p with |t| = 1, h_num_front[p], h_votes ([n_pairs][4], may be NULL)
 * and h_sigma ([n_pairs][3], may be NULL) as cusift_estimate_pose defines them.  The records are const and a frame may be
 * frame a of many pairs, so the triangulated points do not go into coords3D: h_points3d ([n_pairs][max_pts][3], may be
 * NULL) receives the first count_a rows of pair p's block, the values cusift_estimate_pose writes into coords3D. */
int cusift_register_pose_batch(cusift_ctx *ctx, const cusift_point *d_points,
                               const unsigned int *d_counters /* or NULL */, int n_images, int max_pts,
                               const int *h_pairs /* [n_pairs][2]: (frame a, frame b) */, int n_pairs, int distance,
                               int rule, float lo, float hi, int num_loops, float thresh, int refine_loops,
                               float refine_thresh, uint64_t seed, const cusift_camera *camera1,
                               const cusift_camera *camera2 /* may be NULL */, double *h_fundamental /* [n_pairs][9] */,
                               double *h_ransac /* [n_pairs][9] */, int *h_num_candidates, int *h_num_matches,
                               int *h_num_fit, int *h_best_loop /* may be NULL */,
                               char *h_inliers /* [n_pairs][max_pts], may be NULL */,
                               float *h_match_error /* [n_pairs][max_pts], may be NULL */,
                               double *h_rt /* [n_pairs][12] */, int *h_num_front, int *h_votes /* may be NULL */,
                               double *h_sigma /* may be NULL */,
                               float *h_points3d /* [n_pairs][max_pts][3], may be NULL */);

/* cusift_register_pnp for every pair of a list: coords3D of frame a's records -- from cusift_lift_depth over the batch, or
 * the caller's -- against the pixels of their matches in frame b, whose camera is camera2 for every pair.  coords3D is
 * read and never written.  h_rt[12 p .. 12 p + 11] (refined) and h_ransac[12 p .. 12 p + 11] (the winner) map frame b
 * into frame a, X_a = R X_b + t, in the unit coords3D is in: metric after a depth lift.  Frames of 6 and 7 records are
 * fitted, as in the pair call. */
int cusift_register_pnp_batch(cusift_ctx *ctx, const cusift_point *d_points,
                              const unsigned int *d_counters /* or NULL */, int n_images, int max_pts,
                              const int *h_pairs /* [n_pairs][2]: (frame a, frame b) */, int n_pairs, int distance,
                              int rule, float lo, float hi, const cusift_camera *camera2, int num_loops, float thresh,
                              int refine_loops, float refine_thresh, uint64_t seed, double *h_rt /* [n_pairs][12] */,
                              double *h_ransac /* [n_pairs][12] */, int *h_num_candidates, int *h_num_matches,
                              int *h_num_fit, int *h_best_loop /* may be NULL */,
                              char *h_inliers /* [n_pairs][max_pts], may be NULL */,
                              float *h_match_error /* [n_pairs][max_pts], may be NULL */);

/* ---- descriptors at caller-supplied keypoints -------------------------------------------- */
/* Orientation + descriptor of keypoints the CALLER supplies -- a tracker's predictions, reprojected map points, a dense
 * grid, another detector's output, an earlier extraction's records -- in place, in the caller's order (OpenCV's
 * compute() / useProvidedKeypoints, VLFeat's 'frames').  New: the reference describes only what it detects.
 * Asynchronous on the context's stream: no host read-back, no allocation once the arena is sized.
 * d_points: n_images * p->max_pts records; image i has min(d_counters[i], max_pts) of them, max_pts with d_counters ==
 * NULL; nothing beyond that count is touched.  coords2D and scale are in input-image pixels, as extraction writes them.
 * Of `p` only num_octaves, subsampling, max_pts, tex_frac_bits, root_sift and upsample are read; keep_strongest,
 * cross-check and match-bits do not affect the call.
 *   pyramid   octave images o = 0 .. num_octaves - 1 in the context's arena, the extraction's bit for bit: sub[0] =
 *             p->subsampling (0.5f * p->subsampling with upsample = 1, octave 0 then being the cusift_scale_up
 *             enlargement), sub[o] = sub[o - 1] * 2.0f, image o + 1 = cusift_scale_down(variance 0.5) of image o.
 *   skipped   a record with a coordinate or the scale not finite, or !(scale > 0): no image is read, data becomes 128
 *             zeros, subsampling 0, orientation stays.  Everything finite is legal -- positions outside the image, any
 *             scale: the samplers clamp, as for the stage calls.
 *   octave    recorded: CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE is not set and the record's subsampling has exactly the bits
 *             of some sub[o] -- that o (the first such).  Otherwise (subsampling 0, NaN, anything else) from the scale,
 *             in fp32: the largest o with   scale >= 0.93303299f * sub[o]   (one product, one comparison), 0 if there
 *             is none.  0.93303299f = 2^-0.1 is the lowest scale / subsampling the detector's refinement assigns, so an
 *             octave's range [0.93303299f sub[o], 0.93303299f sub[o + 1]) is the one the detector emits.
 *   units     px = x / sub[o], py = y / sub[o], kscale = scale / sub[o], three fp32 divisions (exact for a power of two).
 *   written   orientation (degrees) -- unless CUSIFT_DESCRIBE_KEEP_ORIENTATION, which uses the record's value as it is
 *             (0 = upright SIFT); data[128] (RootSIFT with p->root_sift); subsampling = sub[o].  Every other byte of the
 *             record, coords2D and scale included, keeps the caller's bits.
 * The same device functions as the extraction on the same images: records of cusift_extract_batch come back byte for
 * byte.  CUSIFT_ERR_INVALID, nothing enqueued: the geometry cusift_extract_batch refuses, unknown flag bits, NULL
 * images or points with something to do.  n_images == 0 or max_pts == 0: CUSIFT_OK, nothing done. */
enum { CUSIFT_DESCRIBE_KEEP_ORIENTATION = 1, CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE = 2 };
int cusift_describe_batch(cusift_ctx *ctx, const float *d_imgs, int n_images, int w, int h, int pitch,
                          size_t image_stride, const cusift_params *p, cusift_point *d_points,
                          const unsigned int *d_counters /* or NULL */, unsigned int flags);

/* ---- second-peak orientations ----------------------------------------------------------- */
/* A second record for every keypoint whose orientation histogram has a second peak above `ratio` of the first, as
 * Lowe's, OpenCV's, VLFeat's and SiftGPU's extraction emit one.  The reference computes both peaks and leaves the
 * duplication compiled out (ComputeOrientations_D, cuSIFT_D.cu:380 `&& false`); this is that rule, at most ONE duplicate
 * per keypoint.  A stage on any records: an extraction's (cusift_ctx_set_second_orientation, below, runs it
 * behind every extraction) or a caller's after cusift_describe_batch.  Asynchronous on the context's stream: three
 * launches behind the pyramid's whatever the records hold, no host read-back, no allocation once the arena is sized.
 * d_points: n_images * p->max_pts records; image i has n = min(d_counters[i], max_pts) of them.  Pyramid, `skipped`
 * validity, octave and units are cusift_describe_batch's, CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE (the only flag) included;
 * of `p` the same fields are read.
 *   parent    record j < n gets a duplicate iff it is valid (coordinates and scale finite, scale > 0) and, with hist[32]
 *             the smoothed histogram of the orientation stage -- on the record's octave image in octave units, the same
 *             texture model, sums in the oracle's order: the same bits -- and pk[b] = hist[b] where hist[b] > hist[b - 1]
 *             && hist[b] >= hist[b + 1] (indices mod 32), else 0:
 *               maxval1 = max(0, max_b pk[b]),   i1 = the first b with pk[b] == maxval1 > 0, -1 if there is none;
 *               maxval2 = max(0, max_{b != i1} pk[b]),   i2 = the first b != i1 with pk[b] == maxval2 > 0, -1 if none
 *             (what the reference's one pass over the 32 peaks, cuSIFT_D.cu:359-375, leaves in these four), it holds
 *               i2 >= 0   &&   maxval2 > ratio * maxval1          in fp32: one product, one strict comparison,
 *             and the orientation below is a number (a histogram with infinite entries may give a NaN: no duplicate).
 *             The record's own orientation field is neither read nor checked.
 *   second    orientation2 = 11.25f * (pk2 < 0 ? pk2 + 32 : pk2),   pk2 = i2 + 0.5f * (v1 - v2) / (2.0f * maxval2 - v1 - v2),
 *             v1 = hist[(i2 + 1) & 31], v2 = hist[(i2 + 31) & 31]: the first peak's interpolation around i2.
 *   placed    with m the number of parents of image i: duplicate k (k = 0, 1, ... in ascending parent index) goes to
 *             slot n + k as long as n + k < max_pts; d_counters[i] = min(n + m, max_pts) (a raw counter above max_pts
 *             comes back as max_pts).  Records [0, n) keep every byte; nothing at or beyond the new count is touched.
 *             No append race: the same input gives the same bytes on every run.
 *   holds     the parent's record byte for byte, except: orientation = orientation2; data[128] = the descriptor at
 *             orientation2 from the extraction's own descriptor device function (RootSIFT with p->root_sift);
 *             subsampling = sub[o] of the octave the rule above chose -- the parent's own bits whenever the parent was
 *             described on this pyramid.
 * CUSIFT_ERR_INVALID, nothing enqueued: what cusift_describe_batch refuses, a ratio outside (0, 1] or not a number,
 * d_counters == NULL, any other flag bit.  n_images == 0 or max_pts == 0: CUSIFT_OK, nothing done. */
int cusift_second_orientations_batch(cusift_ctx *ctx, const float *d_imgs, int n_images, int w, int h, int pitch,
                                     size_t image_stride, const cusift_params *p, cusift_point *d_points,
                                     unsigned int *d_counters /* in-out, not NULL */, float ratio, unsigned int flags);

/* The stage above behind every extraction of a context (new here; the reference computes the peak and leaves the duplication compiled out,
 * cuSIFT_D.cu:380): a keypoint whose orientation histogram has a second peak above `ratio` of the first gets a second
 * record at that orientation.  Sticky per context; ratio = 0 (the default) turns it off and extraction is bit for bit
 * and launch for launch what it was; 0.8f is the reference's constant.  With 0 < ratio <= 1 every cusift_extract /
 * _extract_host / _extract_batch on this context, and every cusift_graph recorded while it is set, runs the stage of
 * cusift_second_orientations_batch (above: the contract, expression by expression) right behind the
 * description, on the pyramid that launch has just read: three more launches on the context's stream, the same number
 * whatever the images hold, no host read-back.  Image i then holds its n records, every byte as with ratio = 0, and
 * behind them the duplicates in ascending parent index, cut where max_pts ends; d_counters[i] = min(n + duplicates,
 * max_pts).  With cusift_ctx_set_keep_strongest(k) the selection runs first, only kept records duplicate, and an image
 * holds up to min(2 k, max_pts) records.  The stage needs the one description launch over all octaves: the call is
 * refused with CUSIFT_ERR_INVALID, nothing enqueued, with fused_detect = 0, CUSIFT_POLICY_GENERIC_KERNELS or more than
 * 256 images per call.  A ratio that is negative, above 1 or not a number is refused here.  cusift_tiled_* refuses a
 * context with ratio > 0; cusift_pipe_* creates its own contexts and does not duplicate. */
int cusift_ctx_set_second_orientation(cusift_ctx *ctx, float ratio);

/* ---- feature tracks of a sequence: match-graph components and their triangulation (sift_tracks.hip) --------------- */
/* From the rows of a pair-list matcher to TRACKS, the observations (frame, record) of one scene point across the
 * sequence: what OpenMVG's TracksBuilder, COLMAP's correspondence graph and every bundle adjuster take as input.  New:
 * the reference returns matches per pair.  Everything stays on the device.
 * NODES: v = f * max_pts + i is live when i < count_f = min(d_counters[f], max_pts) (d_counters == NULL: max_pts each);
 * N = n_images * max_pts <= 2^31 - 1.
 * EDGES: for pair p = (a, b) of h_pairs and a live record i of frame a, with row = d_rows[p * max_pts + i] and m =
 * row.match, the edge (a, i) -- (b, m) exists iff ALL of
 *     a != b;   0 <= m < count_b;
 *     the row passes `rule`, the CANDIDATES predicates of cusift_estimate_homography:  0: score > lo && ambiguity < hi;
 *       1: score < lo^2 && ambiguity < hi^2 (the squares in fp32).  A NaN fails; rule 0 with lo = -inf and hi = +inf
 *       switches the test off;
 *     d_keep == NULL or d_keep[p * max_pts + i] != 0   (where the h_inliers of a cusift_register_*_batch call go back in);
 *     d_rows_back == NULL or d_rows_back[p * max_pts + m].match == i   (the cross-check of cusift_select_mutual).
 * Rows past count_a are never read, and a pair with count_a == 0 or count_b == 0 contributes nothing whatever bytes its
 * rows hold (the matchers leave them unwritten).  A frame may be in any number of pairs, on either side; repeated pairs,
 * and both (a, b) and (b, a), are legal.  Rows of cusift_match8_batch* are the same struct.
 * TRACKS: a connected component of the live nodes under the edges is a track iff it has at least min_views (>= 2) nodes
 * AND no two of its nodes lie in one frame.  A component with two records of one frame is dropped whole (OpenMVG's rule:
 * one wrong match must not glue two scene points together).  Tracks are numbered 0 .. T-1 in ascending order of their
 * smallest node.
 * OUTPUTS, device memory:
 *     d_track[v]      track of node v or -1; all N entries are written, dead slots included
 *     d_offsets[0..T] and d_obs[0 .. d_offsets[T]): the nodes of track t in ascending node order -- one per frame, frames
 *                     ascending -- at d_obs[d_offsets[t] .. d_offsets[t + 1]).  The caller provides N / 2 + 1 entries of
 *                     d_offsets and N of d_obs; entries past the ones named are not written
 *     d_stats[8]      [0] T; [1] observations = d_offsets[T]; [2] accepted (p, i) rows, duplicates counted each time;
 *                     [3] components dropped for a shared frame; [4] components of >= 2 nodes dropped only for
 *                     min_views; [5..7] 0
 * Asynchronous on the context's stream: no synchronisation, no read-back, and a number of launches that depends on
 * neither the data nor n_pairs (a lock-free union-find, ordered scans; sift_tracks.hip).  Scratch lives in the context
 * and grows on demand.  h_pairs is read before the call returns.  The same input gives the same bytes in every output.
 * CUSIFT_ERR_INVALID (nothing enqueued, nothing written): what cusift_match_batch refuses of n_images, max_pts, h_pairs
 * and n_pairs; N > 2^31 - 1; a NULL d_rows with n_pairs > 0; a NULL output; an unknown rule; a NaN lo or hi; min_views <
 * 2; d_rows_back == d_rows.  n_pairs == 0 or max_pts == 0: CUSIFT_OK, every d_track entry -1, d_offsets[0] = 0, d_stats
 * zeros. */
int cusift_build_tracks(cusift_ctx *ctx, const unsigned int *d_counters /* or NULL */, int n_images, int max_pts,
                        const int *h_pairs /* [n_pairs][2] */, int n_pairs,
                        const cusift_match_row *d_rows /* [n_pairs][max_pts] */,
                        const cusift_match_row *d_rows_back /* [n_pairs][max_pts] or NULL */,
                        const unsigned char *d_keep /* [n_pairs][max_pts] or NULL */,
                        int rule, float lo, float hi, int min_views,
                        int *d_track /* [n_images][max_pts] */, int *d_offsets, int *d_obs,
                        unsigned int *d_stats /* [8] */);

/* The 3-D point of every track from ALL its views: the midpoint triangulation, the point nearest to all pixel rays, from a
 * 3 x 3 positive definite system.  h_poses[f] is the row-major [R | t] of frame f, camera to world, X_world = R X_f + t:
 * the top three rows of chain_poses' matrices -- with metric poses the points share one scale, which the per-pair points
 * of cusift_register_pose* (|t| = 1 per pair) do not.  One cusift_camera serves all frames; only fx, fy, cx, cy and
 * origin are used, px = cx - origin, py = cy - origin, the floats widened first.  The track count is read on the device
 * from d_stats[0] and clamped to max_tracks; the grid is sized from max_tracks.  ALL FP64, every expression evaluated in
 * the order written (the build uses -ffp-contract=off), the members of a track in d_obs order, the sums from 0:
 *     x, y = coords2D of the record, widened;   d = ((x - px) / fx, (y - py) / fy, 1)
 *     w[i] = (R[i][0]*d0 + R[i][1]*d1) + R[i][2];          n = (w0*w0 + w1*w1) + w2*w2
 *     M[i][j] = (i == j ? 1 : 0) - (w[i]*w[j]) / n
 *     A[i][j] += M[i][j];      g[i] += (M[i][0]*t0 + M[i][1]*t1) + M[i][2]*t2
 *     q00 = A00;  l00 = sqrt(q00);  l10 = A10 / l00;  l20 = A20 / l00
 *     q11 = A11 - l10*l10;  l11 = sqrt(q11);  l21 = (A21 - l20*l10) / l11
 *     q22 = A22 - (l20*l20 + l21*l21);  l22 = sqrt(q22)
 *     y0 = g0 / l00;  y1 = (g1 - l10*y0) / l11;  y2 = (g2 - (l20*y0 + l21*y1)) / l22
 *     X2 = y2 / l22;  X1 = (y1 - l21*X2) / l11;  X0 = (y0 - (l10*X1 + l20*X2)) / l00
 *     per member:  e = X - t;  c[j] = (R[0][j]*e0 + R[1][j]*e1) + R[2][j]*e2;  in front iff c2 > 0
 *                  u = fx*(c0/c2) + px;  v = fy*(c1/c2) + py;  err2 = (u - x)*(u - x) + (v - y)*(v - y)
 *                  worst = err2 > worst ? err2 : worst          (from 0; a NaN never enters)
 * DEGENERATE: any of q00, q11, q22 not > min_pivot, or X not finite -- four zeros and d_front = 0.  Two identical rays
 * give q22 = 1.1e-16, positive, so 0 lets them through; 1e-12 is about a thousand times the rounding noise of a ten-view
 * sum (10 * 2^-53).  A caller who wants a parallax limit passes more: for two views, 1 - cos(angle between the rays).
 * Every other track: d_points3d[t] = (X0, X1, X2, sqrt(worst)) -- the point in world coordinates and its largest
 * reprojection error in pixels -- and d_front[t] = the number of members in front of their camera.  Rows at or past the
 * track count are not written.  d_points is read, never written.  Asynchronous, no synchronisation; h_poses is read
 * before the call returns, as h_models is.
 * CUSIFT_ERR_INVALID (nothing enqueued): a NULL pointer; a pose entry that is not finite; fx or fy zero or not finite;
 * cx, cy or origin not finite; min_pivot negative or NaN; max_tracks < 0; n_images outside [0, 65535], max_pts outside
 * [0, 2^20], N > 2^31 - 1. */
int cusift_triangulate_tracks(cusift_ctx *ctx, const cusift_point *d_points, int n_images, int max_pts,
                              const int *d_offsets, const int *d_obs, const unsigned int *d_stats, int max_tracks,
                              const double *h_poses /* [n_images][12] */, const cusift_camera *camera,
                              double min_pivot, double *d_points3d /* [max_tracks][4] */, int *d_front /* [max_tracks] */);

/* ---- bundle adjustment: the poses and the track points refined together (sift_bundle.hip) ------------------------- */
/* Minimises  sum over the USED observations of  rho(|pi(R_f^T (X_t - t_f)) - pixel|^2)  over the poses of the frames that
 * move and the points of the used tracks, by Schur-complement Levenberg-Marquardt, on the device.  New: the reference
 * stops at one model per pair.  The conventions are cusift_triangulate_tracks', unchanged: h_poses[f] = row-major
 * [R | t], camera to world; one camera for all frames, px = cx - origin, py = cy - origin, the floats widened; the track
 * count T = min(d_stats[0], max_tracks) is read on the device; d_points is read, never written.  rho is the identity
 * (huber == 0) or Huber's function at `huber` pixels, applied as IRLS weights taken at the current accepted iterate.
 * ALL FP64, every expression in the order written (-ffp-contract=off), "from 0" sums start at +0.0.
 * ONE OBSERVATION of track t in frame f, pixel (x, y) = coords2D widened, pose P = [R | t], point X:
 *     e = X - t;  c[j] = (R[0][j]*e0 + R[1][j]*e1) + R[2][j]*e2;  q0 = c0/c2;  q1 = c1/c2
 *     r0 = (fx*q0 + px) - x;  r1 = (fy*q1 + py) - y;  err2 = r0*r0 + r1*r1
 *     rho = err2  if huber == 0 or err2 <= huber*huber,  else (2*huber)*sqrt(err2) - huber*huber
 *     w   = 1     under the same condition,              else huber / sqrt(err2)
 * USED, decided once, at entry, under h_poses and the input d_points3d.  A track is unused if its input row is four
 * zeros (triangulation's degenerate mark), if a member is not a node of the batch, or if a member's x or y is not
 * finite.  Otherwise an observation is used iff c2 > 0 && err2 < inf && (max_error == 0 || sqrt(err2) <= max_error),
 * and the track is used iff at least two of its observations are; an unused track has no used observation.  Unused
 * tracks keep their input row bit for bit.
 * HELD: frame f is held iff h_fixed[f] != 0 (h_fixed == NULL: frame 0 only) or it has no used observation.  Its camera
 * Jacobian is taken as zero, its diagonal block of the reduced system is the identity, its output pose is its input pose
 * bit for bit.  With frame 0 alone held the scale is left to the damping; fix a second frame to pin it.
 * PARAMETRISATION: R <- R Exp(w) with the Rodrigues expression of the PnP refit (E = I + A [w]x + B [w]x^2, A = sin(th)
 * / th, B = (1 - cos(th)) / th^2, 1 and 1/2 below th^2 = 1e-20; R'[i][j] = (R[i][0]*E[0][j] + R[i][1]*E[1][j]) +
 * R[i][2]*E[2][j]), t <- t + dt, X <- X + dX; the camera unknowns are ordered (w, dt).  JACOBIANS of (r0, r1):
 *     a0 = fx/c2;  a1 = fy/c2;  b0 = 0 - a0*q0;  b1 = 0 - a1*q1
 *     JX[0][k] = a0*R[k][0] + b0*R[k][2];   JX[1][k] = a1*R[k][1] + b1*R[k][2]                       (k = 0..2)
 *     Jc[0][0..2] = (0 - b0*c1,  b0*c0 - a0*c2,  a0*c1);   Jc[1][0..2] = (a1*c2 - b1*c1,  b1*c0,  0 - a1*c0)
 *     Jc[r][3 + k] = 0 - JX[r][k]
 *     W[a][k] = w*(Jc[0][a]*JX[0][k] + Jc[1][a]*JX[1][k])                      (6 x 3, never stored: recomputed)
 * ONE ITERATION at the current poses, points and lambda:
 *   per used track, over its used members in d_obs order, from 0:
 *     V[i][j] += w*(JX[0][i]*JX[0][j] + JX[1][i]*JX[1][j])   (i >= j);     gt[i] += w*(JX[0][i]*r0 + JX[1][i]*r1)
 *     v_ii = V_ii + lambda*V_ii;  v10, v20, v21 = V's;  c00 = v11*v22 - v21*v21;  c10 = v21*v20 - v10*v22
 *     c20 = v10*v21 - v11*v20;  det = (v00*c00 + v10*c10) + v20*c20;  c11 = v00*v22 - v20*v20
 *     c21 = v10*v20 - v00*v21;  c22 = v00*v11 - v10*v10;   Vi[i][j] = Vi[j][i] = c_ij / det
 *     the track's pivots FAIL unless v00 > 0 && c22 > 0 && 0 < det < inf
 *   per used observation:  Y[a][k] = (W[a][0]*Vi[0][k] + W[a][1]*Vi[1][k]) + W[a][2]*Vi[2][k]
 *   per free frame f, over its records (FRAME ORDER, below), from 0:
 *     U[a][b] += w*(Jc[0][a]*Jc[0][b] + Jc[1][a]*Jc[1][b]);    gf[a] += w*(Jc[0][a]*r0 + Jc[1][a]*r1)
 *     ef[a] += (Y[a][0]*gt0 + Y[a][1]*gt1) + Y[a][2]*gt2
 *   per pair of free frames f <= g, over the records of frame f whose track has a used observation in g, FRAME ORDER:
 *     E[a][b] += (Y_f[a][0]*W_g[b][0] + Y_f[a][1]*W_g[b][1]) + Y_f[a][2]*W_g[b][2]
 *   the reduced system, dense, of size M = 6 n_images:   S[6f+a][6f+b] = (a == b ? U[a][a] + lambda*U[a][a] : U[a][b])
 *     - E_ff[a][b];   S[6g+b][6f+a] = 0 - E_fg[a][b]  (f < g);   rhs[6f+a] = ef[a] - gf[a];   a held frame: identity
 *     block, zero rows and columns, rhs 0.  Only the lower triangle of S is used.
 *   Cholesky, column j = 0 .. M-1:  acc_i = S[i][j], then acc_i -= L[i][k]*L[j][k] for k = 0 .. j-1 ascending (i >= j);
 *     L[j][j] = sqrt(acc_j);  L[i][j] = acc_i / L[j][j].  The pivot FAILS unless 0 < acc_j < inf.
 *     L y = rhs:  for j ascending  y_j = b_j / L[j][j],  then b_i -= L[i][j]*y_j for i > j;
 *     L^T d = y:  for j descending  d_j = y_j / L[j][j],  then y_i -= L[j][i]*d_j for i < j.
 *   trial poses of the free frames from d[6f .. 6f+5] as above.  Trial points, per used track, members in d_obs order:
 *     z[k] = ((((W[0][k]*d0 + W[1][k]*d1) + W[2][k]*d2) + W[3][k]*d3) + W[4][k]*d4) + W[5][k]*d5   (d of the member's frame)
 *     s[k] = gt[k], then s[k] += z[k];   X'[i] = X[i] + (0 - ((Vi[i][0]*s0 + Vi[i][1]*s1) + Vi[i][2]*s2))
 *   the cost of a track = sum of rho over its used members in d_obs order from 0; +inf if its pivots failed, if a used
 *     observation lands at c2 <= 0 (or NaN), or if the sum is not < inf.  The COST = the sum over the used tracks in
 *     FRAME ORDER by track number; the trial cost is +inf too if a pivot of S failed.
 * FRAME ORDER: 256 partial sums, partial k takes index k, k + 256, k + 512, ... ascending, from 0 (the index is the
 * record of the frame, or the track number; what is not used adds nothing); then partial[k] += partial[k + h] for
 * h = 128, 64, .. 1, and partial[0] is the sum.  No floating-point atomics anywhere: the same input gives the same bytes
 * in every output on every run.
 * THE DECISION, on the device: the trial is accepted iff trial cost < cost.  Accepted: the trial becomes the iterate,
 * lambda = max(lambda / 10, lambda_min), and the solver stops if (cost - trial) / cost <= min_decrease.  Rejected:
 * lambda = 10 lambda, and the solver stops if lambda > lambda_max.  Without a used track it is stopped at entry.  After
 * a stop the remaining enqueued iterations do nothing.
 * OUTPUTS, device memory:
 *     d_points3d[t]  (X, Y, Z, sqrt of the largest err2 over the track's used observations, from 0) of a used track under
 *                    the final poses; other rows, and rows at or past T, are not written
 *     d_poses        all n_images poses, [R | t] row-major
 *     d_history[k]   (cost before, trial cost, lambda used, flag): 1 accepted, 0 rejected; an iteration that did not run:
 *                    (cost, cost, lambda, 2)
 *     d_summary[8]   entry cost, final cost, accepted steps, iterations run, used tracks, used observations, free frames,
 *                    final lambda
 * Asynchronous on the context's stream: no synchronisation, no read-back, 5 launches before the first iteration
 * (copies included), 6 per iteration and 1 behind the last, whatever the data holds.  Scratch lives in the context and
 * grows on demand: a word per node, some 200 bytes per track, and S (8 M^2 bytes, 18.9 MB at 256 frames).  h_poses and
 * h_fixed are read before the call returns.
 * CUSIFT_ERR_INVALID (nothing enqueued): everything cusift_triangulate_tracks refuses; a NULL params or output;
 * n_images > 256 (the reduced system is dense; beyond it takes an iterative solver); iterations outside [1, 100];
 * lambda, lambda_min or lambda_max not positive and finite; huber, max_error or min_decrease negative or not finite.
 * max_tracks == 0 (or a batch without nodes): CUSIFT_OK, d_poses = h_poses, d_summary zeros, d_history rows
 * (0, 0, lambda, 2). */
typedef struct cusift_bundle_params {
  int    iterations;    /* Levenberg-Marquardt iterations ENQUEUED, 1 .. 100 */
  double lambda;        /* initial damping, > 0                      (default 1e-3) */
  double lambda_min;    /* floor after an accepted step              (default 1e-9) */
  double lambda_max;    /* above it the solver stops                 (default 1e6)  */
  double huber;         /* pixels; 0 = plain squared error */
  double max_error;     /* pixels; entry gate per observation; 0 = off */
  double min_decrease;  /* relative; stop after an accepted step that gains less (default 1e-12) */
} cusift_bundle_params;
void cusift_bundle_default_params(cusift_bundle_params *p); /* the defaults above, iterations 10 */

int cusift_bundle_adjust(cusift_ctx *ctx, const cusift_point *d_points, int n_images, int max_pts,
                         const int *d_offsets, const int *d_obs, const unsigned int *d_stats, int max_tracks,
                         const double *h_poses /* [n_images][12] */,
                         const unsigned char *h_fixed /* [n_images] or NULL: frame 0 only */,
                         const cusift_camera *camera, const cusift_bundle_params *params,
                         double *d_points3d /* [max_tracks][4], IN and OUT */,
                         double *d_poses /* [n_images][12], OUT */,
                         double *d_history /* [iterations][4], OUT */, double *d_summary /* [8], OUT */);

#ifdef __cplusplus
}
#endif
#endif /* CUSIFT_AMD_EXTRAS_H */
