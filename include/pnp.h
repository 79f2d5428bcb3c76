// pnp.h -- absolute pose on the device from 3-D/2-D matches (PnP): the records of one frame carry coords3D -- from a depth
// image (rgbd.h) or from RegisterPose (pose.h) -- and their matches carry pixels of an ordinary image; the answer is that
// image's pose in the unit the points are in, metres or the first baseline.  This is the step that registers a third
// view after RegisterPose, or a colour-only frame against an RGB-D one.  The reference has no counterpart; the calls sit
// on cusift_estimate_pnp / cusift_register_pnp (cusift_amd_extras.h, where the arithmetic is written out): six-point DLT
// hypotheses, reprojection inliers, the first hypothesis with the most inliers and Gauss-Newton rounds, all on the
// device in fp64, with one synchronisation.
//
// Rt is 12 doubles, row-major [R | t] with X1 = R X2 + t -- RegisterRGBD's direction -- and t in the unit of coords3D.
// [I | 0] and zero counts when fewer than six records qualify.  camera2 belongs to the matches' image; of a cusift_camera
// only fx, fy, cx, cy and origin are used.  A coplanar point set gets a rotation but no promise about the pose:
// planar scenes belong to RegisterPlanar (homography.h).
#ifndef CUSIFT_AMD_PNP_H
#define CUSIFT_AMD_PNP_H

#include <cstdint>

#include "cuSIFT.h"
#include "cusift_amd_extras.h"
#include "epipolar.h"
#include "matching.h"
#include "sequence.h"

// The pose over the device records of `data`, which carry match fields and coords3D.  The candidates are those of `rule`
// (as EstimateFundamental's) with a finite coords3D whose z is not 0; *numMatches of them lie within `thresh` px of the
// winning hypothesis, *numFit within refineThresh px of the refined pose.  match_error of EVERY device record becomes its
// reprojection error in pixels.  ransac (may be NULL): the winner's [R | t].  Returns the elapsed milliseconds.
inline double EstimatePnP(SiftData &data, const cusift_camera *camera2, double *Rt, int *numMatches, int *numFit,
                          int numLoops = 10000, float minScore = 0.0f, float maxAmbiguity = 0.8f, float thresh = 2.0f,
                          int refineLoops = 5, float refineThresh = 2.0f, uint64_t seed = 0, int rule = 0,
                          int numPts2 = -1, double *ransac = nullptr, int *numCandidates = nullptr) {
  TimerGPU timer;
  double winner[12];
  int candidates = 0;
  safeCall(cusift_estimate_pnp(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(data.d_data), data.numPts, numPts2,
                               rule, minScore, maxAmbiguity, camera2, numLoops, thresh, refineLoops, refineThresh, seed, Rt,
                               ransac ? ransac : winner, numCandidates ? numCandidates : &candidates, numMatches, numFit,
                               nullptr, nullptr, nullptr, nullptr, nullptr));
  return timer.read();
}

// MatchSiftData(data1, data2), then EstimatePnP over data1, in one call with one synchronisation (cusift_register_pnp).
// Writes the match fields and match_error of data1's device records and leaves coords3D alone; SetCrossCheck(true)
// (matching.h) is honoured as RegisterEpipolar honours it.
inline double RegisterPnP(SiftData &data1, SiftData &data2, const cusift_camera *camera2, double *Rt, int *numMatches,
                          int *numFit, int numLoops = 10000, float minScore = 0.0f, float maxAmbiguity = 0.8f,
                          float thresh = 2.0f, int refineLoops = 5, float refineThresh = 2.0f, uint64_t seed = 0,
                          int distance = 0, int rule = 0, double *ransac = nullptr, int *numCandidates = nullptr) {
  TimerGPU timer;
  double winner[12];
  int candidates = 0;
  safeCall(cusift_register_pnp(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(data1.d_data), data1.numPts,
                               reinterpret_cast<const cusift_point *>(data2.d_data), data2.numPts, distance, rule,
                               minScore, maxAmbiguity, camera2, numLoops, thresh, refineLoops, refineThresh, seed, Rt,
                               ransac ? ransac : winner, numCandidates ? numCandidates : &candidates, numMatches, numFit,
                               nullptr, nullptr, nullptr, nullptr, nullptr));
  return timer.read();
}

// MatchSiftData under a pose that is already known (not in the reference): cusift_match_projected() instead of
// cusift_match() -- the second matching pass behind RegisterPnP, or a tracker's search under a predicted pose.  A record
// of data2 can be the match of a record of data1 only within `radius` pixels of where Rt (12 doubles, [R | t] with X1 = R
// X2 + t, as RegisterPnP returns it) and camera2 put that record's coords3D.  A record without depth (coords3D z == 0),
// behind camera 2 or that nothing passes has match == -1 and is not returned.  Everything else is MatchSiftData's, as in
// MatchSiftDataGuided (matching.h).
inline std::vector<SiftMatch *> MatchSiftDataProjected(SiftData &data1, SiftData &data2, const double Rt[12],
                                                       const cusift_camera *camera2, float radius,
                                                       MatchSiftDistance distance = MatchSiftDistanceL2,
                                                       float scoreThreshold = 999.0, float ambiguityThreshold = 1.0,
                                                       MatchType type = MatchType2D) {
  std::vector<SiftMatch *> matches;
  if (!data1.numPts || !data2.numPts) return matches;
  if (data1.d_data == nullptr || data2.d_data == nullptr) return matches;
  cusift_ctx *ctx = cusift_dropin::ctx();
  safeCall(cusift_match_projected(ctx, reinterpret_cast<cusift_point *>(data1.d_data), data1.numPts,
                                  reinterpret_cast<const cusift_point *>(data2.d_data), data2.numPts,
                                  distance == MatchSiftDistanceL2 ? 1 : 0, Rt, camera2, radius));
  return cusift_dropin::read_back_matches(ctx, data1, data2, scoreThreshold, ambiguityThreshold, type);
}

// MatchSiftDataProjected on the byte descriptors (cusift_match8_projected): MatchSiftData8 (matching.h) where a record of
// data2 counts for a record of data1 only within `radius` pixels of where Rt and camera2 put that record's coords3D -- the
// same test, evaluated on the records' coordinates inside the int8 matcher.  The same filter, the same return type.
inline std::vector<SiftMatch *> MatchSiftData8Projected(SiftData &data1, SiftDescriptors8 &desc1, SiftData &data2,
                                                        SiftDescriptors8 &desc2, const double Rt[12],
                                                        const cusift_camera *camera2, float radius,
                                                        MatchSiftDistance distance = MatchSiftDistanceL2,
                                                        float scoreThreshold = 999.0, float ambiguityThreshold = 1.0,
                                                        MatchType type = MatchType2D) {
  if (!data1.numPts || !data2.numPts) return {};
  if (data1.d_data == nullptr || data2.d_data == nullptr) return {};
  if (desc1.numPts != data1.numPts || desc2.numPts != data2.numPts) return {};  // not the descriptors of these sets
  cusift_ctx *ctx = cusift_dropin::ctx();
  safeCall(cusift_match8_projected(ctx, reinterpret_cast<cusift_point *>(data1.d_data), data1.numPts, desc1.d_data,
                                   desc1.d_sums, reinterpret_cast<const cusift_point *>(data2.d_data), data2.numPts,
                                   desc2.d_data, desc2.d_sums, distance == MatchSiftDistanceL2 ? 1 : 0, Rt, camera2,
                                   radius));
  return cusift_dropin::read_back_matches(ctx, data1, data2, scoreThreshold, ambiguityThreshold, type);
}

// RegisterPnP for a whole sequence in one call (cusift_register_pnp_batch): pair k = (a, b) of `pairs` gives
// Rts[12 k .. 12 k + 11] = [R | t] with X_a = R X_b + t in the unit of frame a's coords3D -- metric after a depth lift, so
// the poses of consecutive pairs compose into a trajectory.  camera2 is the camera of frame b of every pair.  coords3D of
// the frames' device records is read and not written, and neither is anything else of them.  An empty `pairs` means
// (i, i + 1) for every consecutive frame; pair k draws from seed + k and has the bits RegisterPnP gives for it with that
// seed.  matchErrors[k][i]: what RegisterPnP leaves in match_error of record i of frame a (empty for a pair without a
// fit); inliers[k][i]: the winner's flag.  Returns the elapsed milliseconds.
inline double RegisterPnPSequence(std::vector<SiftData *> &frames, std::vector<std::pair<int, int> > pairs,
                                  const cusift_camera *camera2, std::vector<double> &Rts,
                                  std::vector<int> *numMatches = NULL, std::vector<int> *numFit = NULL,
                                  int numLoops = 10000, float minScore = 0.0f, float maxAmbiguity = 0.8f,
                                  float thresh = 2.0f, int refineLoops = 5, float refineThresh = 2.0f, uint64_t seed = 0,
                                  int distance = 0, int rule = 0, std::vector<double> *ransac = NULL,
                                  std::vector<std::vector<float> > *matchErrors = NULL,
                                  std::vector<std::vector<char> > *inliers = NULL,
                                  std::vector<int> *numCandidates = NULL) {
  TimerGPU timer;
  cusift_dropin::SequencePack pack(frames, pairs);
  cusift_dropin::SequenceOutputs<double> out(pack, 12, inliers != NULL, matchErrors != NULL);
  safeCall(cusift_register_pnp_batch(cusift_dropin::ctx(), pack.d_points(), pack.d_counters(), pack.n, pack.max_pts,
                                     pack.h_pairs.data(), pack.n_pairs, distance, rule, minScore, maxAmbiguity, camera2,
                                     numLoops, thresh, refineLoops, refineThresh, seed, out.model.data(), out.winner.data(),
                                     out.candidates.data(), out.matches.data(), out.fit.data(), NULL, out.flags(),
                                     out.errors()));
  // a fit counts at least its own six samples
  out.finish(&Rts, ransac, numMatches, numFit, out.matches, 1, matchErrors, inliers);
  if (numCandidates) numCandidates->assign(out.candidates.begin(), out.candidates.begin() + pack.n_pairs);
  return timer.read();
}

#endif  // CUSIFT_AMD_PNP_H
