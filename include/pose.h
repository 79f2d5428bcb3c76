// pose.h -- calibrated two-view pose on the device: from matched SiftData and the cameras' intrinsics to [R | t] and a
// triangulated point in coords3D of every record that fits, where the RGB-D path (rgbd.h) gets both from depth images.
// The reference has no counterpart; the calls sit on cusift_estimate_pose / cusift_register_pose (cusift_amd_extras.h,
// where the arithmetic is written out): the essential matrix E = K2^T F K1, its four (R, t) candidates, the cheirality
// vote over the candidates that fit F and the triangulation all run on the device in fp64, with one synchronisation.
//
// Rt is 12 doubles, row-major [R | t] with X1 = R X2 + t -- RegisterRGBD's direction -- and |t| = 1: the baseline is the
// unit of length, also of coords3D.  [I | 0] and *numFront = 0 when F is degenerate or nothing lies in front of both
// cameras.  camera belongs to `data` / `data1` (coords2D), camera2 to the matches' image (NULL: the same camera); of a
// cusift_camera only fx, fy, cx, cy and origin are used.
#ifndef CUSIFT_AMD_POSE_H
#define CUSIFT_AMD_POSE_H

#include <cstdint>

#include "cuSIFT.h"
#include "cusift_amd_extras.h"
#include "epipolar.h"
#include "sequence.h"

// The pose from a fundamental matrix F (9 doubles as EstimateFundamental returns them) over the device records of
// `data`, which carry match fields.  The fit set is the candidates of `rule` (as EstimateFundamental's) within `thresh`
// px of F; *numFront of them lie in front of both cameras under the chosen pose, and coords3D of EVERY device record is
// written: the triangulated point for those, zeros for the rest (data.Synchronize() brings it to the host).  votes (may
// be NULL): the four candidates' counts; sigma (may be NULL): the singular values of E.  Returns the elapsed milliseconds.
inline double EstimatePose(SiftData &data, const double *F, const cusift_camera *camera, double *Rt, int *numFront,
                           float minScore = 0.0f, float maxAmbiguity = 0.8f, float thresh = 1.0f, int rule = 0,
                           const cusift_camera *camera2 = nullptr, int numPts2 = -1, int *votes = nullptr,
                           double *sigma = nullptr) {
  TimerGPU timer;
  safeCall(cusift_estimate_pose(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(data.d_data), data.numPts, numPts2,
                                rule, minScore, maxAmbiguity, F, thresh, camera, camera2, Rt, numFront, votes, sigma));
  return timer.read();
}

// RegisterEpipolar, then EstimatePose at refineThresh with the refined F where the device left it, in one call with one
// synchronisation (cusift_register_pose).  F (may be NULL) receives the refined fundamental matrix.  Writes the match
// fields, match_error and coords3D of data1's device records; SetCrossCheck(true) (matching.h) is honoured as
// RegisterEpipolar honours it.
inline double RegisterPose(SiftData &data1, SiftData &data2, const cusift_camera *camera, double *Rt, int *numMatches,
                           int *numFit, int *numFront, int numLoops = 10000, float minScore = 0.0f,
                           float maxAmbiguity = 0.8f, float thresh = 1.0f, int refineLoops = 5,
                           float refineThresh = 1.0f, uint64_t seed = 0, int distance = 0, int rule = 0,
                           const cusift_camera *camera2 = nullptr, double *F = nullptr, int *votes = nullptr,
                           double *sigma = nullptr) {
  TimerGPU timer;
  double refined[9], winner[9];
  int numCandidates = 0;
  safeCall(cusift_register_pose(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(data1.d_data), data1.numPts,
                                reinterpret_cast<const cusift_point *>(data2.d_data), data2.numPts, distance, rule,
                                minScore, maxAmbiguity, numLoops, thresh, refineLoops, refineThresh, seed, camera, camera2,
                                F ? F : refined, winner, &numCandidates, numMatches, numFit, nullptr, nullptr, nullptr,
                                nullptr, nullptr, Rt, numFront, votes, sigma));
  return timer.read();
}

// RegisterPose for a whole sequence in one call (cusift_register_pose_batch): pair k = (a, b) of `pairs` gives
// Rts[12 k .. 12 k + 11] = [R | t] with X_a = R X_b + t and |t| = 1 -- PER PAIR: the scale of every pair is its own, so
// these poses do not compose into a trajectory (RegisterPnPSequence of pnp.h, which is metric, does).  `camera` serves
// frame a and camera2 frame b of every pair (NULL: the same camera).  An empty `pairs` means (i, i + 1) for every
// consecutive frame; pair k draws from seed + k and has the bits RegisterPose gives for it with that seed.  The frames
// are NOT written: points3D[k] holds 3 floats per record of frame a, what RegisterPose writes into coords3D.
// fundamentals (optional): the refined F of every pair.  Returns the elapsed milliseconds.
inline double RegisterPoseSequence(std::vector<SiftData *> &frames, std::vector<std::pair<int, int> > pairs,
                                   const cusift_camera *camera, std::vector<double> &Rts,
                                   std::vector<int> *numMatches = NULL, std::vector<int> *numFit = NULL,
                                   std::vector<int> *numFront = NULL, int numLoops = 10000, float minScore = 0.0f,
                                   float maxAmbiguity = 0.8f, float thresh = 1.0f, int refineLoops = 5,
                                   float refineThresh = 1.0f, uint64_t seed = 0, int distance = 0, int rule = 0,
                                   const cusift_camera *camera2 = nullptr, std::vector<double> *fundamentals = NULL,
                                   std::vector<std::vector<float> > *points3D = NULL,
                                   std::vector<std::vector<char> > *inliers = NULL) {
  TimerGPU timer;
  cusift_dropin::SequencePack pack(frames, pairs);
  cusift_dropin::SequenceOutputs<double> out(pack, 9, inliers != NULL, false);  // F's outputs; the pose's own on top
  std::vector<int> front(pack.slots());
  std::vector<double> rt(12 * pack.slots());
  std::vector<float> h_xyz(points3D ? 3 * pack.flat() : 0);
  safeCall(cusift_register_pose_batch(cusift_dropin::ctx(), pack.d_points(), pack.d_counters(), pack.n, pack.max_pts,
                                      pack.h_pairs.data(), pack.n_pairs, distance, rule, minScore, maxAmbiguity, numLoops,
                                      thresh, refineLoops, refineThresh, seed, camera, camera2, out.model.data(),
                                      out.winner.data(), out.candidates.data(), out.matches.data(), out.fit.data(), NULL,
                                      out.flags(), NULL, rt.data(), front.data(), NULL, NULL,
                                      points3D ? h_xyz.data() : NULL));
  out.finish(fundamentals, NULL, numMatches, numFit, out.candidates, 8, NULL, inliers);
  Rts.assign(rt.begin(), rt.begin() + 12 * (size_t)pack.n_pairs);
  if (numFront) numFront->assign(front.begin(), front.begin() + pack.n_pairs);
  pack.rows(h_xyz, 3, NULL, points3D);
  return timer.read();
}

#endif  // CUSIFT_AMD_POSE_H
