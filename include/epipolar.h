// epipolar.h -- two views of a general 3-D scene: the fundamental matrix from matched SiftData, on the device.  The
// reference has no counterpart; the calls mirror EstimateHomography / RegisterPlanar of homography.h over
// cusift_estimate_fundamental / cusift_register_epipolar (cusift_amd_extras.h, where the arithmetic is written out):
// candidates, eight samples per hypothesis drawn from a seed, the normalised 8-point solve, Sampson inlier counts over
// the candidates, selection and the refit all run on the device in fp64, with one synchronisation; the same seed gives
// the same bytes.
//
// F is 9 doubles, row-major, Frobenius norm 1, with x2^T F x1 = 0 for x1 = (coords2D, 1) of `data` / `data1` and x2 =
// (match_xpos, match_ypos, 1); nine zeros when there are fewer than 8 candidates.  thresh and refineThresh are Sampson
// distances in pixels (1 px each by default, where the planar calls use 5 and 3 px of reprojection error); numLoops is
// used as given.
#ifndef CUSIFT_AMD_EPIPOLAR_H
#define CUSIFT_AMD_EPIPOLAR_H

#include <cstdint>
#include <utility>
#include <vector>

#include "cuSIFT.h"
#include "cusift_amd_extras.h"
#include "sequence.h"

// RANSAC + refit on the device records of `data` (which carry match fields).  *numMatches: inliers of the winning
// hypothesis among the candidates; *numFit: candidates within refineThresh of the refined F.  match_error (the Sampson
// distance under the refined F) is written into the DEVICE records (data.Synchronize() brings it to the host).  rule 0:
// score > minScore && ambiguity < maxAmbiguity; rule 1: score < minScore^2 && ambiguity < maxAmbiguity^2 (for
// MatchSiftDistanceL2).  ransac (may be NULL): the winning hypothesis before the refit.  Returns the elapsed milliseconds.
inline double EstimateFundamental(SiftData &data, double *F, int *numMatches, int *numFit, int numLoops = 10000,
                                  float minScore = 0.0f, float maxAmbiguity = 0.8f, float thresh = 1.0f,
                                  int refineLoops = 5, float refineThresh = 1.0f, uint64_t seed = 0, int rule = 0,
                                  double *ransac = nullptr, int numPts2 = -1) {
  TimerGPU timer;
  double winner[9];
  int numCandidates = 0;
  safeCall(cusift_estimate_fundamental(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(data.d_data), data.numPts,
                                       numPts2, rule, minScore, maxAmbiguity, numLoops, thresh, refineLoops,
                                       refineThresh, seed, F, ransac ? ransac : winner, &numCandidates, numMatches,
                                       numFit, nullptr, nullptr, nullptr, nullptr, nullptr));
  return timer.read();
}

// MatchSiftData's device part, then EstimateFundamental over data1, in one call with one synchronisation
// (cusift_register_epipolar).  distance: 0 = MatchSiftDistanceDotProduct, 1 = MatchSiftDistanceL2 (use rule 1 with it).
// Writes the match fields and match_error of data1's device records; after SetCrossCheck(true) (matching.h) only mutual
// matches are candidates and data2's match fields are written too.
inline double RegisterEpipolar(SiftData &data1, SiftData &data2, double *F, int *numMatches, int *numFit,
                               int numLoops = 10000, float minScore = 0.0f, float maxAmbiguity = 0.8f,
                               float thresh = 1.0f, int refineLoops = 5, float refineThresh = 1.0f, uint64_t seed = 0,
                               int distance = 0, int rule = 0, double *ransac = nullptr) {
  TimerGPU timer;
  double winner[9];
  int numCandidates = 0;
  safeCall(cusift_register_epipolar(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(data1.d_data), data1.numPts,
                                    reinterpret_cast<const cusift_point *>(data2.d_data), data2.numPts, distance, rule,
                                    minScore, maxAmbiguity, numLoops, thresh, refineLoops, refineThresh, seed, F,
                                    ransac ? ransac : winner, &numCandidates, numMatches, numFit, nullptr, nullptr,
                                    nullptr, nullptr, nullptr));
  return timer.read();
}

// RegisterEpipolar for a whole sequence in one call (cusift_register_epipolar_batch): pair k = (a, b) of `pairs` gives
// x_b^T F x_a = 0, fundamentals[9 k .. 9 k + 8]; an empty `pairs` means (i, i + 1) for every consecutive frame.  Every
// pair is matched, marked, drawn, scored and refitted in the same launches, with one synchronisation.  Pair k draws from
// seed + k, so every pair has the bits RegisterEpipolar gives for it with that seed.  A frame may be in any number of
// pairs, on either side.  The frames themselves are NOT written: matchErrors[k][i] is what RegisterEpipolar leaves in
// match_error of record i of frame a (empty for a pair without a fit), inliers[k][i] the winner's flag.  ransac
// (optional): the winning hypotheses before the refit.  Returns the elapsed milliseconds.
inline double RegisterEpipolarSequence(std::vector<SiftData *> &frames, std::vector<std::pair<int, int> > pairs,
                                       std::vector<double> &fundamentals, std::vector<int> *numMatches = NULL,
                                       std::vector<int> *numFit = NULL, int numLoops = 10000, float minScore = 0.0f,
                                       float maxAmbiguity = 0.8f, float thresh = 1.0f, int refineLoops = 5,
                                       float refineThresh = 1.0f, uint64_t seed = 0, int distance = 0, int rule = 0,
                                       std::vector<double> *ransac = NULL,
                                       std::vector<std::vector<float> > *matchErrors = NULL,
                                       std::vector<std::vector<char> > *inliers = NULL) {
  TimerGPU timer;
  cusift_dropin::SequencePack pack(frames, pairs);
  cusift_dropin::SequenceOutputs<double> out(pack, 9, inliers != NULL, matchErrors != NULL);
  safeCall(cusift_register_epipolar_batch(cusift_dropin::ctx(), pack.d_points(), pack.d_counters(), pack.n, pack.max_pts,
                                          pack.h_pairs.data(), pack.n_pairs, distance, rule, minScore, maxAmbiguity,
                                          numLoops, thresh, refineLoops, refineThresh, seed, out.model.data(),
                                          out.winner.data(), out.candidates.data(), out.matches.data(), out.fit.data(),
                                          NULL, out.flags(), out.errors()));
  out.finish(&fundamentals, ransac, numMatches, numFit, out.candidates, 8, matchErrors, inliers);
  return timer.read();
}

#endif  // CUSIFT_AMD_EPIPOLAR_H
