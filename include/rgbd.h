// rgbd.h -- the step the reference's RGB-D chain never had: SiftPoint::coords3D from a depth image, and the whole
// frame-to-frame registration (lift, match, select, RANSAC, refit) as one device-resident call.
// With LiftSiftData the reference's commented-out RANSACTestImage (test/test.cpp:136-184) is a live program:
//     LiftSiftData(d1, depth1, w, h, cam);  LiftSiftData(d2, depth2, w, h, cam);
//     matches = MatchSiftData(d1, d2, MatchSiftDistanceL2, 1000, 0.6, MatchType3D);       // matching.h, unchanged
//     EstimateRigidTransform(matches, Rt, &numInliers, 1024, 0.05, RigidTransformType3D);  // rigidTransform.h, unchanged
// RegisterRGBD does the same without the two host filters and the re-upload in between (cusift_register_rgbd,
// cusift_amd_extras.h: one stream synchronisation, at the read-back).  The lift convention is documented at
// cusift_lift_depth.  RegisterRGBDSequence does a whole sequence -- a pair list over n frames -- in one such call
// (cusift_register_rgbd_batch).  Plain C++ over the C ABI: no HIP headers.
#ifndef CUSIFT_AMD_RGBD_H
#define CUSIFT_AMD_RGBD_H

#include <cstddef>
#include <cstdint>
#include <ctime>
#include <utility>
#include <vector>

#include "cuSIFT.h"
#include "cusift_amd_extras.h"
#include "matching.h"
#include "rigidTransform.h"
#include "sequence.h"

namespace cusift_dropin {
// a 16-bit depth image on the device, dense rows; freed when it goes out of scope
struct device_depth : device_block {
  device_depth(const unsigned short *h_depth, int w, int h) : device_block(sizeof(unsigned short) * (size_t)w * (size_t)h) {
    safeCall(cusift_memcpy_h2d(ctx(), ptr, h_depth, sizeof(unsigned short) * (size_t)w * (size_t)h));
  }
  const uint16_t *get() const { return static_cast<const uint16_t *>(ptr); }
};
}  // namespace cusift_dropin

// Uploads the depth image (w x h 16-bit samples, dense rows), writes coords3D of the device records and refreshes
// coords3D of the host records when the SiftData has both.  Nothing else of a record changes.
inline void LiftSiftData(SiftData &data, const unsigned short *h_depth, int w, int h, const cusift_camera &camera) {
  if (data.numPts <= 0 || data.d_data == nullptr || h_depth == nullptr) return;
  cusift_ctx *ctx = cusift_dropin::ctx();
  cusift_dropin::device_depth depth(h_depth, w, h);
  safeCall(cusift_lift_depth(ctx, reinterpret_cast<cusift_point *>(data.d_data), nullptr, 1, data.numPts, depth.get(), w,
                             h, w, (size_t)w * (size_t)h, &camera));
  if (data.h_data != nullptr)
    safeCall(cusift_memcpy2d_d2h(ctx, data.h_data[0].coords3D, sizeof(SiftPoint), data.d_data[0].coords3D,
                                 sizeof(SiftPoint), 3 * sizeof(float), (size_t)data.numPts));
  else
    safeCall(cusift_ctx_synchronize(ctx));  // the depth image is freed on return
}

// Registration of frame 2 onto frame 1 (x1 ~ R x2 + t, Rt = [R | t] row-major): both SiftData need device records.
// thresh is a distance (metres), like EstimateRigidTransform's.  pairs (optional) receives (index in data1, index in
// data2) of every selected match, inliers (optional) one flag per selected match.  seed 0: time(0), like the
// reference's RANSAC.  The device records of both frames get their coords3D, those of data1 their match fields; host
// records are not refreshed (Synchronize them if they are needed).
inline void RegisterRGBD(SiftData &data1, SiftData &data2, const unsigned short *h_depth1,
                         const unsigned short *h_depth2, int w, int h, const cusift_camera &camera, float Rt[12],
                         int *numInliers, int *numMatches = NULL, int numLoops = 1024, float thresh = 0.05f,
                         RigidTransformType type = RigidTransformType3D,
                         MatchSiftDistance distance = MatchSiftDistanceL2, float scoreThreshold = 999.0f,
                         float ambiguityThreshold = 1.0f, uint64_t seed = 0,
                         std::vector<std::pair<int, int> > *pairs = NULL, std::vector<char> *inliers = NULL) {
  cusift_ctx *ctx = cusift_dropin::ctx();
  cusift_dropin::device_depth depth1(h_depth1, w, h), depth2(h_depth2, w, h);
  const int n1 = data1.d_data != nullptr ? data1.numPts : 0, n2 = data2.d_data != nullptr ? data2.numPts : 0;
  std::vector<int> h_pairs(pairs ? 2 * (size_t)(n1 > 0 ? n1 : 1) : 0);
  std::vector<char> h_flags(inliers ? (size_t)(n1 > 0 ? n1 : 1) : 0);
  int matches = 0, found = 0;
  safeCall(cusift_register_rgbd(ctx, reinterpret_cast<cusift_point *>(data1.d_data), n1, depth1.get(),
                                reinterpret_cast<cusift_point *>(data2.d_data), n2, depth2.get(), w, h, w, &camera,
                                distance == MatchSiftDistanceL2 ? 1 : 0, scoreThreshold, ambiguityThreshold, numLoops,
                                thresh * thresh, type == RigidTransformType3D ? 1 : 0,
                                seed ? seed : (uint64_t)std::time(0), Rt, &matches, &found,
                                pairs ? h_pairs.data() : NULL, inliers ? h_flags.data() : NULL));
  if (numInliers) *numInliers = found;
  if (numMatches) *numMatches = matches;
  if (pairs) {
    pairs->clear();
    for (int k = 0; k < matches; k++) pairs->push_back(std::make_pair(h_pairs[2 * (size_t)k], h_pairs[2 * (size_t)k + 1]));
  }
  if (inliers) inliers->assign(h_flags.begin(), h_flags.begin() + matches);
}

// Registration of a whole sequence in one call (cusift_register_rgbd_batch): pair k = (a, b) of `pairs` maps frame b
// into frame a, Rt[12 k .. 12 k + 11] = [R | t] row-major with x_a ~ R x_b + t; an empty `pairs` means (i, i + 1) for
// every consecutive frame, the walk of main.cpp: compareMatchingWithMATLAB.  The frames' device records are packed
// into one [n][maxPts] block with device-to-device copies (maxPts = the largest numPts), the depth images (w x h
// 16-bit samples each, dense rows) are uploaded into one block, and every pair is matched, filtered and estimated in
// the same launches, with one synchronisation.  Pair k draws from seed + k (seed 0: time(0)), so with the same seed
// pair 0 has the bits RegisterRGBD gives for it.  A frame may be in any number of pairs.  The frames themselves are not
// written: coords3D and the match results live in the packed block and in the outputs.  selected / inliers (optional)
// receive, per pair, what RegisterRGBD's pairs / inliers receive.
inline void RegisterRGBDSequence(std::vector<SiftData *> &frames, const std::vector<const unsigned short *> &h_depths,
                                 int w, int h, const cusift_camera &camera, std::vector<std::pair<int, int> > pairs,
                                 std::vector<float> &Rt, std::vector<int> *numInliers = NULL,
                                 std::vector<int> *numMatches = NULL, int numLoops = 1024, float thresh = 0.05f,
                                 RigidTransformType type = RigidTransformType3D,
                                 MatchSiftDistance distance = MatchSiftDistanceL2, float scoreThreshold = 999.0f,
                                 float ambiguityThreshold = 1.0f, uint64_t seed = 0,
                                 std::vector<std::vector<std::pair<int, int> > > *selected = NULL,
                                 std::vector<std::vector<char> > *inliers = NULL) {
  cusift_ctx *ctx = cusift_dropin::ctx();
  cusift_dropin::SequencePack pack(frames, pairs);  // a copy: the lift and the matcher write it, not the frames
  const int n_pairs = pack.n_pairs, max_pts = pack.max_pts;
  const size_t image = (size_t)w * (size_t)h;
  cusift_dropin::device_block depth(sizeof(unsigned short) * image * (size_t)pack.n);
  for (int i = 0; i < pack.n; i++)
    safeCall(cusift_memcpy_h2d(ctx, static_cast<unsigned short *>(depth.ptr) + (size_t)i * image, h_depths[i],
                               sizeof(unsigned short) * image));
  std::vector<int> matches(pack.slots()), found(pack.slots());
  std::vector<int> h_sel(selected ? 2 * pack.flat() : 0);
  std::vector<char> h_flags(inliers ? pack.flat() : 0);
  std::vector<float> rt(12 * pack.slots());
  safeCall(cusift_register_rgbd_batch(ctx, pack.d_points(), pack.d_counters(), pack.n, max_pts,
                                      static_cast<const uint16_t *>(depth.ptr), w, h, w, image, &camera,
                                      pack.h_pairs.data(), n_pairs, distance == MatchSiftDistanceL2 ? 1 : 0,
                                      scoreThreshold, ambiguityThreshold, numLoops, thresh * thresh,
                                      type == RigidTransformType3D ? 1 : 0, seed ? seed : (uint64_t)std::time(0),
                                      rt.data(), matches.data(), found.data(), selected ? h_sel.data() : NULL,
                                      inliers ? h_flags.data() : NULL));
  Rt.assign(rt.begin(), rt.begin() + 12 * (size_t)n_pairs);
  if (numInliers) numInliers->assign(found.begin(), found.begin() + n_pairs);
  if (numMatches) numMatches->assign(matches.begin(), matches.begin() + n_pairs);
  if (selected) {
    selected->assign((size_t)n_pairs, std::vector<std::pair<int, int> >());
    for (int k = 0; k < n_pairs; k++)
      for (int m = 0; m < matches[k]; m++) {
        const int *row = h_sel.data() + 2 * ((size_t)k * max_pts + (size_t)m);
        (*selected)[k].push_back(std::make_pair(row[0], row[1]));
      }
  }
  if (inliers) {
    inliers->assign((size_t)n_pairs, std::vector<char>());
    for (int k = 0; k < n_pairs; k++)
      (*inliers)[k].assign(h_flags.begin() + (size_t)k * max_pts, h_flags.begin() + (size_t)k * max_pts + matches[k]);
  }
}

#endif  // CUSIFT_AMD_RGBD_H
