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

namespace cusift_dropin {
// What the sequence calls of epipolar.h, pose.h and pnp.h share: the frames' device records packed into one
// [n][maxPts] block with device-to-device copies (maxPts = the largest numPts), their counts next to it, and the pair
// list -- an empty one means (i, i + 1) for every consecutive frame.
struct SequencePack {
  void *points = nullptr, *counters = nullptr;
  int n = 0, max_pts = 1, n_pairs = 0;
  std::vector<unsigned int> counts;
  std::vector<int> h_pairs;
  SequencePack(std::vector<SiftData *> &frames, std::vector<std::pair<int, int> > &pairs) {
    cusift_ctx *c = ctx();
    n = (int)frames.size();
    if (pairs.empty())
      for (int i = 0; i + 1 < n; i++) pairs.push_back(std::make_pair(i, i + 1));
    n_pairs = (int)pairs.size();
    counts.assign((size_t)(n > 0 ? n : 1), 0u);
    for (int i = 0; i < n; i++) {
      counts[i] = frames[i]->d_data != nullptr && frames[i]->numPts > 0 ? (unsigned int)frames[i]->numPts : 0u;
      if ((int)counts[i] > max_pts) max_pts = (int)counts[i];
    }
    safeCall(cusift_malloc(&points, sizeof(SiftPoint) * (size_t)(n > 0 ? n : 1) * (size_t)max_pts));
    safeCall(cusift_malloc(&counters, sizeof(unsigned int) * counts.size()));
    safeCall(cusift_memcpy_h2d(c, counters, counts.data(), sizeof(unsigned int) * counts.size()));
    for (int i = 0; i < n; i++)
      if (counts[i] > 0)
        safeCall(cusift_memcpy_d2d(c, static_cast<SiftPoint *>(points) + (size_t)i * max_pts, frames[i]->d_data,
                                   sizeof(SiftPoint) * (size_t)counts[i]));
    h_pairs.assign(2 * slots(), 0);
    for (int k = 0; k < n_pairs; k++) h_pairs[2 * (size_t)k] = pairs[k].first, h_pairs[2 * (size_t)k + 1] = pairs[k].second;
  }
  ~SequencePack() {
    cusift_free(points);
    cusift_free(counters);
  }
  SequencePack(const SequencePack &) = delete;
  SequencePack &operator=(const SequencePack &) = delete;
  size_t slots() const { return (size_t)(n_pairs > 0 ? n_pairs : 1); }
  const cusift_point *d_points() const { return static_cast<const cusift_point *>(points); }
  const unsigned int *d_counters() const { return static_cast<const unsigned int *>(counters); }
  // the first count_a entries of every pair's block of `flat` ([n_pairs][max_pts][width]); keep[k] == 0: an empty row
  template <class T>
  void rows(const std::vector<T> &flat, int width, const std::vector<char> *keep, std::vector<std::vector<T> > *out) const {
    if (!out) return;
    out->assign((size_t)n_pairs, std::vector<T>());
    for (int k = 0; k < n_pairs; k++) {
      if (keep && !(*keep)[k]) continue;
      const size_t first = (size_t)k * max_pts * width, count = (size_t)counts[h_pairs[2 * (size_t)k]] * width;
      (*out)[k].assign(flat.begin() + first, flat.begin() + first + count);
    }
  }
};
}  // namespace cusift_dropin

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
  const size_t slots = pack.slots(), flat = (size_t)pack.n_pairs * pack.max_pts;
  std::vector<int> candidates(slots), matches(slots), fit(slots);
  std::vector<double> fund(9 * slots), win(9 * slots);
  std::vector<char> h_flags(inliers ? flat : 0);
  std::vector<float> h_err(matchErrors ? flat : 0);
  safeCall(cusift_register_epipolar_batch(cusift_dropin::ctx(), pack.d_points(), pack.d_counters(), pack.n, pack.max_pts,
                                          pack.h_pairs.data(), pack.n_pairs, distance, rule, minScore, maxAmbiguity,
                                          numLoops, thresh, refineLoops, refineThresh, seed, fund.data(), win.data(),
                                          candidates.data(), matches.data(), fit.data(), NULL,
                                          inliers ? h_flags.data() : NULL, matchErrors ? h_err.data() : NULL));
  fundamentals.assign(fund.begin(), fund.begin() + 9 * (size_t)pack.n_pairs);
  if (ransac) ransac->assign(win.begin(), win.begin() + 9 * (size_t)pack.n_pairs);
  if (numMatches) numMatches->assign(matches.begin(), matches.begin() + pack.n_pairs);
  if (numFit) numFit->assign(fit.begin(), fit.begin() + pack.n_pairs);
  std::vector<char> fitted(slots);
  for (int k = 0; k < pack.n_pairs; k++) fitted[k] = candidates[k] >= 8;
  pack.rows(h_flags, 1, NULL, inliers);
  pack.rows(h_err, 1, &fitted, matchErrors);
  return timer.read();
}

#endif  // CUSIFT_AMD_EPIPOLAR_H
