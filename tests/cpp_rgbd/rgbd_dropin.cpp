// The reference's RANSACTestImage (test/test.cpp:136-184, commented out there because nothing filled coords3D) as a
// live program on the reference's own pair: the VLFeat keypoints of frames 1 and 2, their depth images, INTRINSICS and
// MATLAB's Rt1_2.  Twice: staged through LiftSiftData + the unchanged MatchSiftData / EstimateRigidTransform headers,
// and fused through RegisterRGBD.  The reference version would only print; this one asserts.
//
//   rgbd_dropin sift1.bin sift2.bin depth1.u16 depth2.u16 intrinsics.txt Rt1_2.bin
// depth*.u16: 640 x 480 raw little-endian 16-bit samples as stored in the reference's PNGs (the Python test writes them
// from tests/golden/rgbd_depth.npz).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "debug.h"
#include "rgbd.h"

static int failures = 0;
#define EXPECT(cond, ...)                           \
  do {                                              \
    if (!(cond)) {                                  \
      std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                     \
      std::printf("\n");                            \
      ++failures;                                   \
    }                                               \
  } while (0)

static const int W = 640, H = 480;

static bool read_file(const char *path, void *dst, size_t bytes) {
  FILE *fp = std::fopen(path, "rb");
  if (!fp) return false;
  const bool ok = std::fread(dst, 1, bytes, fp) == bytes;
  std::fclose(fp);
  return ok;
}

static void print_rt(const char *what, const float *Rt) {
  std::printf("%s\n", what);
  for (int i = 0; i < 3; i++) std::printf("  % .6f % .6f % .6f % .6f\n", Rt[4 * i], Rt[4 * i + 1], Rt[4 * i + 2], Rt[4 * i + 3]);
}

// |R x2 + t - x1| under MATLAB's Rt1_2, in double
static double residual(const double *Rt, const float *x1, const float *x2) {
  double e = 0;
  for (int i = 0; i < 3; i++) {
    const double p = Rt[4 * i] * x2[0] + Rt[4 * i + 1] * x2[1] + Rt[4 * i + 2] * x2[2] + Rt[4 * i + 3] - x1[i];
    e += p * p;
  }
  return std::sqrt(e);
}

// The fixture's inliers are the matches below 0.05 m under Rt1_2: 325 of the 330 lie below 0.03 m and must be inliers,
// three lie at 0.195 m or more and must not be; the two in between (0.0477, 0.0501 m) may fall either way.
static void check_inliers(const char *who, const std::vector<double> &res, const std::vector<char> &inl, int numInliers) {
  int sure = 0, far = 0, flagged = 0;
  for (size_t i = 0; i < res.size(); i++) {
    flagged += inl[i] ? 1 : 0;
    if (res[i] < 0.03) {
      sure++;
      EXPECT(inl[i] == 1, "%s: match %zu (%.4f m under Rt1_2) is not an inlier", who, i, res[i]);
    } else if (res[i] >= 0.195) {
      far++;
      EXPECT(inl[i] == 0, "%s: match %zu (%.4f m under Rt1_2) is an inlier", who, i, res[i]);
    }
  }
  EXPECT(sure == 325 && far == 3, "%s: %d matches below 0.03 m, %d at 0.195 m or more", who, sure, far);
  EXPECT(flagged == numInliers, "%s: %d flags, %d inliers reported", who, flagged, numInliers);
  EXPECT(numInliers >= 325 && numInliers <= 327, "%s: %d inliers", who, numInliers);
}

static void check_rt(const char *who, const float *Rt, const double *want) {
  // a RANSAC result against MATLAB's own RANSAC: the loose bound of the reference-style program (the Python test
  // compares with a float64 refit over the very same inliers)
  for (int i = 0; i < 12; i++) EXPECT(std::fabs(Rt[i] - want[i]) <= 0.01, "%s: Rt[%d] = %f, fixture %f", who, i, Rt[i], want[i]);
}

int main(int argc, char **argv) {
  if (argc < 7) {
    std::printf("usage: %s sift1 sift2 depth1.u16 depth2.u16 intrinsics.txt Rt1_2.bin\n", argv[0]);
    return 2;
  }
  InitCuda(0);
  std::vector<unsigned short> depth1((size_t)W * H), depth2((size_t)W * H);
  double K[9], want[12];
  FILE *fp = std::fopen(argv[5], "r");
  bool ok = fp != NULL;
  for (int i = 0; ok && i < 9; i++) ok = std::fscanf(fp, "%lf", &K[i]) == 1;
  if (fp) std::fclose(fp);
  ok = ok && read_file(argv[3], depth1.data(), 2 * depth1.size()) && read_file(argv[4], depth2.data(), 2 * depth2.size()) &&
       read_file(argv[6], want, sizeof(want));
  if (!ok) {
    std::printf("FAILED: cannot read the inputs\n");
    return 1;
  }
  cusift_camera cam;
  cam.fx = (float)K[0], cam.fy = (float)K[4], cam.cx = (float)K[2], cam.cy = (float)K[5];
  cam.origin = 1.0f, cam.units_per_metre = 1000.0f, cam.encoding = 1;

  // ---- staged: the reference's RANSACTestImage shape ----
  {
    SiftData d1, d2;
    EXPECT(ReadVLFeatSiftData(d1, argv[1]) > 0 && ReadVLFeatSiftData(d2, argv[2]) > 0, "cannot read the VLFeat dumps");
    LiftSiftData(d1, depth1.data(), W, H, cam);
    LiftSiftData(d2, depth2.data(), W, H, cam);
    int holes = 0;
    for (int i = 0; i < d1.numPts; i++) holes += d1.h_data[i].coords3D[2] == 0.0f ? 1 : 0;
    EXPECT(holes == 29, "%d records of frame 1 without depth", holes);
    std::vector<SiftMatch *> matches = MatchSiftData(d1, d2, MatchSiftDistanceL2, 1000.0f, 0.6f, MatchType3D);
    std::vector<SiftMatch *> matches2d = MatchSiftData(d1, d2, MatchSiftDistanceL2, 1000.0f, 0.6f, MatchType2D);
    EXPECT(matches2d.size() == 340, "%zu 2-D matches", matches2d.size());
    EXPECT(matches.size() == 330, "%zu 3-D matches", matches.size());
    float Rt[12];
    int numInliers = -1;
    std::vector<char> inl(matches.size(), 2);
    EstimateRigidTransform(matches, Rt, &numInliers, 1024, 0.05f, RigidTransformType3D, NULL, inl.data());
    std::printf("staged: matches %zu, inliers %d\n", matches.size(), numInliers);
    print_rt("  Rt (device)", Rt);
    std::vector<double> res;
    for (size_t i = 0; i < matches.size(); i++) res.push_back(residual(want, matches[i]->pt1->coords3D, matches[i]->pt2->coords3D));
    check_inliers("staged", res, inl, numInliers);
    check_rt("staged", Rt, want);
    for (size_t i = 0; i < matches.size(); i++) delete matches[i];
    for (size_t i = 0; i < matches2d.size(); i++) delete matches2d[i];
  }
  // ---- fused ----
  {
    SiftData d1, d2;
    ReadVLFeatSiftData(d1, argv[1]);
    ReadVLFeatSiftData(d2, argv[2]);
    float Rt[12];
    int numInliers = -1, numMatches = -1;
    std::vector<std::pair<int, int> > pairs;
    std::vector<char> inl;
    RegisterRGBD(d1, d2, depth1.data(), depth2.data(), W, H, cam, Rt, &numInliers, &numMatches, 1024, 0.05f,
                 RigidTransformType3D, MatchSiftDistanceL2, 1000.0f, 0.6f, 7, &pairs, &inl);
    std::printf("fused: matches %d, inliers %d\n", numMatches, numInliers);
    print_rt("  Rt (device)", Rt);
    EXPECT(numMatches == 330 && pairs.size() == 330 && inl.size() == 330, "%d matches, %zu pairs", numMatches, pairs.size());
    d1.Synchronize();  // coords3D of the device records -> host
    d2.Synchronize();
    std::vector<double> res;
    for (size_t k = 0; k < pairs.size(); k++) {
      EXPECT(k == 0 || pairs[k].first > pairs[k - 1].first, "pairs not ascending at %zu", k);
      EXPECT(pairs[k].first >= 0 && pairs[k].first < d1.numPts && pairs[k].second >= 0 && pairs[k].second < d2.numPts, "pair %zu out of range", k);
      res.push_back(residual(want, d1.h_data[pairs[k].first].coords3D, d2.h_data[pairs[k].second].coords3D));
    }
    if (res.size() == inl.size()) check_inliers("fused", res, inl, numInliers);
    check_rt("fused", Rt, want);
    float Rt2[12];
    int again = -1;
    RegisterRGBD(d1, d2, depth1.data(), depth2.data(), W, H, cam, Rt2, &again, NULL, 1024, 0.05f, RigidTransformType3D,
                 MatchSiftDistanceL2, 1000.0f, 0.6f, 7);
    EXPECT(again == numInliers && std::memcmp(Rt, Rt2, sizeof(Rt)) == 0, "the same seed gave another answer");
  }
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
