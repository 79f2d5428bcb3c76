// matching.h -- drop-in for the reference's extras/matching.h (MatchSiftData) on top of the C ABI.
// Same enums, SiftMatch record and call signature (extras/matching.h:10-39); the N x M search runs in
// cusift_match() (one MFMA kernel, no score matrix in memory), the threshold filter runs here like in the
// reference (extras/matching.cu:318-349).
#ifndef CUSIFT_AMD_MATCHING_H
#define CUSIFT_AMD_MATCHING_H

#include <vector>

#include "cuSIFT.h"
#include "cusift_amd_extras.h"

typedef enum { MatchSiftDistanceDotProduct, MatchSiftDistanceL2 } MatchSiftDistance;
typedef enum { MatchType2D, MatchType3D } MatchType;

typedef struct {
  SiftPoint *pt1;
  SiftPoint *pt2;
  float score;      // distance metric (dot product or L2 = 2 - 2 x.y)
  float ambiguity;  // ratio of best and second best
  float error;
} SiftMatch;

namespace cusift_dropin {
// What every MatchSiftData variant does behind its matcher: the five match fields of data1's records back to the host
// (extras/matching.cu:311-315; without a host copy: a synchronisation and no matches), then MatchSiftData's
// threshold filter.
inline std::vector<SiftMatch *> read_back_matches(cusift_ctx *ctx, SiftData &data1, SiftData &data2, float scoreThreshold,
                                                  float ambiguityThreshold, MatchType type) {
  std::vector<SiftMatch *> matches;
  if (data1.h_data == nullptr) {
    safeCall(cusift_ctx_synchronize(ctx));
    return matches;
  }
  safeCall(cusift_memcpy2d_d2h(ctx, &data1.h_data[0].score, sizeof(SiftPoint), &data1.d_data[0].score, sizeof(SiftPoint),
                               5 * sizeof(float), (size_t)data1.numPts));
  const float thresh2 = scoreThreshold * scoreThreshold;
  const float athresh2 = ambiguityThreshold * ambiguityThreshold;
  for (int i = 0; i < data1.numPts; i++) {
    SiftPoint &p = data1.h_data[i];
    if (!(p.score < thresh2 && p.ambiguity < athresh2)) continue;
    if (p.match < 0 || p.match >= data2.numPts || data2.h_data == nullptr) continue;
    if (type == MatchType2D || (p.coords3D[2] != 0 && data2.h_data[p.match].coords3D[2] != 0)) {
      SiftMatch *m = new SiftMatch();
      m->pt1 = &p;
      m->pt2 = &data2.h_data[p.match];
      m->score = p.score;
      m->ambiguity = p.ambiguity;
      m->error = 0.0f;
      matches.push_back(m);
    }
  }
  return matches;
}
}  // namespace cusift_dropin

// Exhaustive search between all SIFT keypoints of two images (the caller owns the returned SiftMatch objects,
// as in the reference).  Both SiftData need host AND device buffers, as in the reference.
inline std::vector<SiftMatch *> MatchSiftData(SiftData &data1, SiftData &data2,
                                              MatchSiftDistance distance = MatchSiftDistanceL2,
                                              float scoreThreshold = 999.0, float ambiguityThreshold = 1.0,
                                              MatchType type = MatchType2D) {
  std::vector<SiftMatch *> matches;
  if (!data1.numPts || !data2.numPts) return matches;
  if (data1.d_data == nullptr || data2.d_data == nullptr) return matches;
  cusift_ctx *ctx = cusift_dropin::ctx();
  safeCall(cusift_match(ctx, reinterpret_cast<cusift_point *>(data1.d_data), data1.numPts,
                        reinterpret_cast<const cusift_point *>(data2.d_data), data2.numPts,
                        distance == MatchSiftDistanceL2 ? 1 : 0));
  return cusift_dropin::read_back_matches(ctx, data1, data2, scoreThreshold, ambiguityThreshold, type);
}

// MatchSiftData under a model that is already known (not in the reference): cusift_match_guided() instead of
// cusift_match() -- a record of data2 whose coords2D fail the test against a record of data1 cannot be its match.  model:
// CUSIFT_GUIDE_HOMOGRAPHY (M = H, x2 ~ H x1, within `radius` pixels of H x1) or CUSIFT_GUIDE_EPIPOLAR (M = F, x2^T F x1 =
// 0, within `radius` pixels of the line F x1); M is row-major.  A record that nothing passes has match == -1 and is not
// returned.  Everything else is MatchSiftData's.
inline std::vector<SiftMatch *> MatchSiftDataGuided(SiftData &data1, SiftData &data2, int model, const double M[9],
                                                    float radius, MatchSiftDistance distance = MatchSiftDistanceL2,
                                                    float scoreThreshold = 999.0, float ambiguityThreshold = 1.0,
                                                    MatchType type = MatchType2D) {
  std::vector<SiftMatch *> matches;
  if (!data1.numPts || !data2.numPts) return matches;
  if (data1.d_data == nullptr || data2.d_data == nullptr) return matches;
  cusift_ctx *ctx = cusift_dropin::ctx();
  safeCall(cusift_match_guided(ctx, reinterpret_cast<cusift_point *>(data1.d_data), data1.numPts,
                               reinterpret_cast<const cusift_point *>(data2.d_data), data2.numPts,
                               distance == MatchSiftDistanceL2 ? 1 : 0, model, M, radius));
  return cusift_dropin::read_back_matches(ctx, data1, data2, scoreThreshold, ambiguityThreshold, type);
}

// MatchSiftData with the cross-check (not in the reference): one cusift_match_mutual() fills the match fields of BOTH
// sets -- data1's as MatchSiftData does, data2's with its best and second best in data1 (the lowest record on exactly
// tied best scores) -- and a pair (i, j) is returned only if it passes MatchSiftData's filter and record j's match is i.
// Both SiftData need host AND device buffers; both host copies are synchronised.  The two sets must be distinct.
inline std::vector<SiftMatch *> MatchSiftDataMutual(SiftData &data1, SiftData &data2,
                                                    MatchSiftDistance distance = MatchSiftDistanceL2,
                                                    float scoreThreshold = 999.0, float ambiguityThreshold = 1.0,
                                                    MatchType type = MatchType2D) {
  std::vector<SiftMatch *> matches;
  if (!data1.numPts || !data2.numPts) return matches;
  if (data1.d_data == nullptr || data2.d_data == nullptr) return matches;
  cusift_ctx *ctx = cusift_dropin::ctx();
  safeCall(cusift_match_mutual(ctx, reinterpret_cast<cusift_point *>(data1.d_data), data1.numPts,
                               reinterpret_cast<cusift_point *>(data2.d_data), data2.numPts,
                               distance == MatchSiftDistanceL2 ? 1 : 0));
  if (data1.h_data == nullptr || data2.h_data == nullptr) {
    safeCall(cusift_ctx_synchronize(ctx));
    return matches;
  }
  safeCall(cusift_memcpy2d_d2h(ctx, &data1.h_data[0].score, sizeof(SiftPoint), &data1.d_data[0].score, sizeof(SiftPoint),
                               5 * sizeof(float), (size_t)data1.numPts));
  safeCall(cusift_memcpy2d_d2h(ctx, &data2.h_data[0].score, sizeof(SiftPoint), &data2.d_data[0].score, sizeof(SiftPoint),
                               5 * sizeof(float), (size_t)data2.numPts));
  const float thresh2 = scoreThreshold * scoreThreshold;
  const float athresh2 = ambiguityThreshold * ambiguityThreshold;
  for (int i = 0; i < data1.numPts; i++) {
    SiftPoint &p = data1.h_data[i];
    if (!(p.score < thresh2 && p.ambiguity < athresh2)) continue;
    if (p.match < 0 || p.match >= data2.numPts) continue;
    SiftPoint &q = data2.h_data[p.match];
    if (type == MatchType3D && !(p.coords3D[2] != 0 && q.coords3D[2] != 0)) continue;
    if (q.match != i) continue;  // the cross-check
    SiftMatch *m = new SiftMatch();
    m->pt1 = &p;
    m->pt2 = &q;
    m->score = p.score;
    m->ambiguity = p.ambiguity;
    m->error = 0.0f;
    matches.push_back(m);
  }
  return matches;
}

// ---- 8-bit descriptors (not in the reference; cusift_quantize_descriptors, cusift_match8) ------------------------------
// The byte descriptors of a SiftData: record i's 128 bytes at h_data / d_data + 128 i -- 512 v clipped to 255, the
// convention of OpenCV, VLFeat and COLMAP -- and d_sums[2 i], d_sums[2 i + 1] = sum q, sum q^2 on the device.  Copying is
// disabled, as for SiftData.
struct SiftDescriptors8 {
  int numPts = 0;                   // descriptors held
  int maxPts = 0;                   // descriptors allocated
  unsigned char *h_data = nullptr;  // [maxPts][128], or nullptr: no host copy wanted
  unsigned char *d_data = nullptr;  // [maxPts][128], 16-byte aligned
  int *d_sums = nullptr;            // [maxPts][2]
  SiftDescriptors8() = default;
  SiftDescriptors8(const SiftDescriptors8 &) = delete;
  SiftDescriptors8 &operator=(const SiftDescriptors8 &) = delete;
  ~SiftDescriptors8() { release(); }
  void release() {
    if (d_data) cusift_free(d_data);
    if (d_sums) cusift_free(d_sums);
    cusift_dropin::host_free(h_data);
    h_data = d_data = nullptr;
    d_sums = nullptr;
    numPts = maxPts = 0;
  }
};

inline void InitSiftDescriptors8(SiftDescriptors8 &desc, int num = 1024, bool host = false) {
  desc.release();
  if (num <= 0) return;
  void *p = nullptr;
  safeCall(cusift_malloc(&p, (size_t)128 * (size_t)num));
  desc.d_data = static_cast<unsigned char *>(p);
  safeCall(cusift_malloc(&p, sizeof(int) * 2 * (size_t)num));
  desc.d_sums = static_cast<int *>(p);
  if (host) desc.h_data = static_cast<unsigned char *>(cusift_dropin::host_alloc((size_t)128 * (size_t)num));
  desc.maxPts = num;
}
inline void FreeSiftDescriptors8(SiftDescriptors8 &desc) { desc.release(); }

// Quantises the descriptors of data's device records into desc (grown when it holds fewer than data.numPts, keeping
// whether it has a host copy) and copies the bytes to desc.h_data when that is not null (blocking then; otherwise
// asynchronous on the calling thread's context).
inline void QuantizeSiftData(SiftData &data, SiftDescriptors8 &desc) {
  if (desc.maxPts < data.numPts) InitSiftDescriptors8(desc, data.numPts, desc.h_data != nullptr);
  desc.numPts = data.numPts;
  if (!data.numPts || data.d_data == nullptr) return;
  cusift_ctx *ctx = cusift_dropin::ctx();
  safeCall(cusift_quantize_descriptors(ctx, reinterpret_cast<const cusift_point *>(data.d_data), nullptr, 1, data.numPts,
                                       desc.d_data, desc.d_sums));
  if (desc.h_data != nullptr) safeCall(cusift_memcpy_d2h(ctx, desc.h_data, desc.d_data, (size_t)128 * (size_t)data.numPts));
}

// MatchSiftData on the byte descriptors (cusift_match8: int8 matrix pipe, exact integer scores scaled by 2^-18 to
// MatchSiftData's range): the same filter, the same return type.  desc1 / desc2 hold the descriptors of data1 / data2
// (QuantizeSiftData, or bytes from elsewhere with cusift_desc8_sums); the float descriptors of the records are not read.
inline std::vector<SiftMatch *> MatchSiftData8(SiftData &data1, SiftDescriptors8 &desc1, SiftData &data2,
                                               SiftDescriptors8 &desc2, MatchSiftDistance distance = MatchSiftDistanceL2,
                                               float scoreThreshold = 999.0, float ambiguityThreshold = 1.0,
                                               MatchType type = MatchType2D) {
  std::vector<SiftMatch *> matches;
  if (!data1.numPts || !data2.numPts) return matches;
  if (data1.d_data == nullptr || data2.d_data == nullptr) return matches;
  if (desc1.numPts != data1.numPts || desc2.numPts != data2.numPts) return matches;  // not the descriptors of these sets
  cusift_ctx *ctx = cusift_dropin::ctx();
  safeCall(cusift_match8(ctx, reinterpret_cast<cusift_point *>(data1.d_data), data1.numPts, desc1.d_data, desc1.d_sums,
                         reinterpret_cast<const cusift_point *>(data2.d_data), data2.numPts, desc2.d_data, desc2.d_sums,
                         distance == MatchSiftDistanceL2 ? 1 : 0));
  return cusift_dropin::read_back_matches(ctx, data1, data2, scoreThreshold, ambiguityThreshold, type);
}

// MatchSiftDataGuided on the byte descriptors (cusift_match8_guided): MatchSiftData8 where a record of data2 whose coords2D
// fail the test of `model` under M against a record of data1 cannot be its match -- the same test, evaluated on the
// records' coordinates inside the int8 matcher.  A record that nothing passes has match == -1 and is not returned.  The
// same filter, the same return type.
inline std::vector<SiftMatch *> MatchSiftData8Guided(SiftData &data1, SiftDescriptors8 &desc1, SiftData &data2,
                                                     SiftDescriptors8 &desc2, int model, const double M[9], float radius,
                                                     MatchSiftDistance distance = MatchSiftDistanceL2,
                                                     float scoreThreshold = 999.0, float ambiguityThreshold = 1.0,
                                                     MatchType type = MatchType2D) {
  if (!data1.numPts || !data2.numPts) return {};
  if (data1.d_data == nullptr || data2.d_data == nullptr) return {};
  if (desc1.numPts != data1.numPts || desc2.numPts != data2.numPts) return {};  // not the descriptors of these sets
  cusift_ctx *ctx = cusift_dropin::ctx();
  safeCall(cusift_match8_guided(ctx, reinterpret_cast<cusift_point *>(data1.d_data), data1.numPts, desc1.d_data,
                                desc1.d_sums, reinterpret_cast<const cusift_point *>(data2.d_data), data2.numPts,
                                desc2.d_data, desc2.d_sums, distance == MatchSiftDistanceL2 ? 1 : 0, model, M, radius));
  return cusift_dropin::read_back_matches(ctx, data1, data2, scoreThreshold, ambiguityThreshold, type);
}

// MatchSiftData8 with the cross-check (cusift_match8_mutual: both directions from one pass over the integer scores): the
// match fields of BOTH sets are written -- data2's are what MatchSiftData8(data2, desc2, data1, desc1) would write into it,
// byte for byte -- and a pair (i, j) is returned only if it passes MatchSiftData's filter and record j's match is i.
// MatchSiftDataMutual's filter and return type; both SiftData need host AND device buffers; the sets must be distinct.
inline std::vector<SiftMatch *> MatchSiftData8Mutual(SiftData &data1, SiftDescriptors8 &desc1, SiftData &data2,
                                                     SiftDescriptors8 &desc2,
                                                     MatchSiftDistance distance = MatchSiftDistanceL2,
                                                     float scoreThreshold = 999.0, float ambiguityThreshold = 1.0,
                                                     MatchType type = MatchType2D) {
  std::vector<SiftMatch *> matches;
  if (!data1.numPts || !data2.numPts) return matches;
  if (data1.d_data == nullptr || data2.d_data == nullptr) return matches;
  if (desc1.numPts != data1.numPts || desc2.numPts != data2.numPts) return matches;  // not the descriptors of these sets
  cusift_ctx *ctx = cusift_dropin::ctx();
  safeCall(cusift_match8_mutual(ctx, reinterpret_cast<cusift_point *>(data1.d_data), data1.numPts, desc1.d_data,
                                desc1.d_sums, reinterpret_cast<cusift_point *>(data2.d_data), data2.numPts, desc2.d_data,
                                desc2.d_sums, distance == MatchSiftDistanceL2 ? 1 : 0));
  if (data1.h_data == nullptr || data2.h_data == nullptr) {
    safeCall(cusift_ctx_synchronize(ctx));
    return matches;
  }
  safeCall(cusift_memcpy2d_d2h(ctx, &data1.h_data[0].score, sizeof(SiftPoint), &data1.d_data[0].score, sizeof(SiftPoint),
                               5 * sizeof(float), (size_t)data1.numPts));
  safeCall(cusift_memcpy2d_d2h(ctx, &data2.h_data[0].score, sizeof(SiftPoint), &data2.d_data[0].score, sizeof(SiftPoint),
                               5 * sizeof(float), (size_t)data2.numPts));
  const float thresh2 = scoreThreshold * scoreThreshold;
  const float athresh2 = ambiguityThreshold * ambiguityThreshold;
  for (int i = 0; i < data1.numPts; i++) {
    SiftPoint &p = data1.h_data[i];
    if (!(p.score < thresh2 && p.ambiguity < athresh2)) continue;
    if (p.match < 0 || p.match >= data2.numPts) continue;
    SiftPoint &q = data2.h_data[p.match];
    if (type == MatchType3D && !(p.coords3D[2] != 0 && q.coords3D[2] != 0)) continue;
    if (q.match != i) continue;  // the cross-check
    SiftMatch *m = new SiftMatch();
    m->pt1 = &p;
    m->pt2 = &q;
    m->score = p.score;
    m->ambiguity = p.ambiguity;
    m->error = 0.0f;
    matches.push_back(m);
  }
  return matches;
}

// The cross-check inside the registrations (not in the reference; cusift_ctx_set_cross_check): while on, RegisterPlanar,
// RegisterRGBD and their ...Sequence forms (homography.h, rgbd.h) feed their RANSAC mutual matches only -- record i of
// the first set must be the best of its own match, the lowest record on exactly tied best scores.  Acts on the calling
// thread's implicit context, the one those calls use.  RegisterPlanar then writes the match fields of data2's device
// records too.  MatchSiftData, MatchSiftDataMutual, FindHomography and EstimateRigidTransform do not change.
inline void SetCrossCheck(bool on) { safeCall(cusift_ctx_set_cross_check(cusift_dropin::ctx(), on ? 1 : 0)); }

// The descriptors the registrations match on (not in the reference; cusift_ctx_set_match_bits): 32, the default, or 8 --
// RegisterPlanar, RegisterRGBD and the other calls SetCrossCheck affects then quantise their records into scratch of the
// calling thread's implicit context and match the bytes on the int8 matrix pipe, bit for bit what QuantizeSiftData +
// MatchSiftData8 + the staged estimate give.  Anything else throws; nothing else reads the setting.
inline void SetMatchBits(int bits) { safeCall(cusift_ctx_set_match_bits(cusift_dropin::ctx(), bits)); }

#endif  // CUSIFT_AMD_MATCHING_H
