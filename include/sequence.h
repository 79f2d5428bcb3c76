// sequence.h -- what the sequence calls of homography.h, epipolar.h, pose.h, pnp.h and rgbd.h share: one device
// allocation, the frames packed for a pair-list call of cusift_amd_extras.h, and the outputs of the marked pair-list
// forms (H, F, pose, PnP) with their way back into the callers' vectors.  Plain C++ over the C ABI: no HIP headers.
#ifndef CUSIFT_AMD_SEQUENCE_H
#define CUSIFT_AMD_SEQUENCE_H

#include <cstddef>
#include <utility>
#include <vector>

#include "cuSIFT.h"

namespace cusift_dropin {
// a device allocation of at least one byte; freed when it goes out of scope
struct device_block {
  void *ptr = nullptr;
  explicit device_block(size_t bytes) { safeCall(cusift_malloc(&ptr, bytes > 0 ? bytes : 1)); }
  ~device_block() { cusift_free(ptr); }
  device_block(const device_block &) = delete;
  device_block &operator=(const device_block &) = delete;
};

// The frames' device records packed into one [n][maxPts] block with device-to-device copies (maxPts = the largest
// numPts, at least 1), their counts next to it -- a frame without device records or with numPts <= 0 counts 0 and is not
// copied -- and the pair list: an empty one means (i, i + 1) for every consecutive frame.  The frames are not written.
struct SequencePack {
  int n, n_pairs = 0, max_pts = 1;
  std::vector<unsigned int> counts;
  std::vector<int> h_pairs;
  device_block points, counters;
  SequencePack(std::vector<SiftData *> &frames, std::vector<std::pair<int, int> > &pairs)
      : n((int)frames.size()), counts(frame_counts(frames, &max_pts)),
        points(sizeof(SiftPoint) * counts.size() * (size_t)max_pts), counters(sizeof(unsigned int) * counts.size()) {
    cusift_ctx *c = ctx();
    if (pairs.empty())
      for (int i = 0; i + 1 < n; i++) pairs.push_back(std::make_pair(i, i + 1));
    n_pairs = (int)pairs.size();
    safeCall(cusift_memcpy_h2d(c, counters.ptr, counts.data(), sizeof(unsigned int) * counts.size()));
    for (int i = 0; i < n; i++)
      if (counts[i] > 0)
        safeCall(cusift_memcpy_d2d(c, static_cast<SiftPoint *>(points.ptr) + (size_t)i * max_pts, frames[i]->d_data,
                                   sizeof(SiftPoint) * (size_t)counts[i]));
    h_pairs.assign(2 * slots(), 0);
    for (int k = 0; k < n_pairs; k++) h_pairs[2 * (size_t)k] = pairs[k].first, h_pairs[2 * (size_t)k + 1] = pairs[k].second;
  }
  // max(n, 1) entries; *max_pts grows to the largest of them
  static std::vector<unsigned int> frame_counts(const std::vector<SiftData *> &frames, int *max_pts) {
    std::vector<unsigned int> counts(frames.empty() ? 1 : frames.size(), 0u);
    for (size_t i = 0; i < frames.size(); i++) {
      counts[i] = frames[i]->d_data != nullptr && frames[i]->numPts > 0 ? (unsigned int)frames[i]->numPts : 0u;
      if ((int)counts[i] > *max_pts) *max_pts = (int)counts[i];
    }
    return counts;
  }
  size_t slots() const { return (size_t)(n_pairs > 0 ? n_pairs : 1); }  // host arrays per pair have at least one entry
  size_t flat() const { return (size_t)n_pairs * max_pts; }             // entries of a [n_pairs][max_pts] output
  cusift_point *d_points() const { return static_cast<cusift_point *>(points.ptr); }
  const unsigned int *d_counters() const { return static_cast<const unsigned int *>(counters.ptr); }
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

// What cusift_register_{planar,epipolar,pose,pnp}_batch write on the host for a pack, and finish(): the first n_pairs
// entries of each into the caller's vectors (a NULL one is left out).  T: float for H, double for F and [R | t];
// values: 9 or 12 per model.  flags() / errors() are NULL unless asked for (and with no pair, when nothing is written).
template <class T>
struct SequenceOutputs {
  const SequencePack &pack;
  const int values;
  std::vector<int> candidates, matches, fit;
  std::vector<T> model, winner;
  std::vector<char> h_flags;
  std::vector<float> h_err;
  SequenceOutputs(const SequencePack &p, int values_, bool want_flags, bool want_errors)
      : pack(p), values(values_), candidates(p.slots()), matches(p.slots()), fit(p.slots()),
        model(values_ * p.slots()), winner(values_ * p.slots()), h_flags(want_flags ? p.flat() : 0),
        h_err(want_errors ? p.flat() : 0) {}
  char *flags() { return h_flags.empty() ? NULL : h_flags.data(); }
  float *errors() { return h_err.empty() ? NULL : h_err.data(); }
  // matchErrors[k] stays empty unless pair k was fitted: support[k] >= least
  void finish(std::vector<T> *models, std::vector<T> *ransac, std::vector<int> *numMatches, std::vector<int> *numFit,
              const std::vector<int> &support, int least, std::vector<std::vector<float> > *matchErrors,
              std::vector<std::vector<char> > *inliers) const {
    const size_t P = (size_t)pack.n_pairs;
    if (models) models->assign(model.begin(), model.begin() + values * P);
    if (ransac) ransac->assign(winner.begin(), winner.begin() + values * P);
    if (numMatches) numMatches->assign(matches.begin(), matches.begin() + P);
    if (numFit) numFit->assign(fit.begin(), fit.begin() + P);
    std::vector<char> fitted(P);
    for (size_t k = 0; k < P; k++) fitted[k] = support[k] >= least;
    pack.rows(h_flags, 1, NULL, inliers);
    pack.rows(h_err, 1, &fitted, matchErrors);
  }
};
}  // namespace cusift_dropin

#endif  // CUSIFT_AMD_SEQUENCE_H
