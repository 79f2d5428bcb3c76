// The reference's RANSACWithIndices and RANSACWithRandom (test/test.cpp:62-134) against include/rigidTransform.h on
// its own fixture (tests/golden/rigid_ransac.bin = test/data/RigidTransform_RANSAC.bin: 120 matched 3-D pairs, 10
// sample triples, MATLAB's Rt).  The reference versions only print; these assert.
//
//   rigid_dropin tests/golden/rigid_ransac.bin
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "debug.h"
#include "rigidTransform.h"

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

static void free_matches(std::vector<SiftMatch *> &matches) {
  for (size_t i = 0; i < matches.size(); i++) {
    delete matches[i]->pt1;
    delete matches[i]->pt2;
    delete matches[i];
  }
}

static void print_rt(const char *what, const float *Rt) {
  std::printf("%s\n", what);
  for (int i = 0; i < 3; i++) std::printf("  % .6f % .6f % .6f % .6f\n", Rt[4 * i], Rt[4 * i + 1], Rt[4 * i + 2], Rt[4 * i + 3]);
}

static void ransac_with_indices(const char *path) {
  std::vector<int> indices;
  float Rt[12];
  std::vector<SiftMatch *> matches = ReadMATLABRANSAC(path, indices, Rt);
  EXPECT(matches.size() == 120 && indices.size() == 30, "fixture: %zu matches, %zu indices", matches.size(), indices.size());
  if (matches.empty()) return;
  const int numLoops = (int)indices.size() / 3;
  for (size_t i = 0; i < indices.size(); i++) EXPECT(indices[i] >= 0 && indices[i] < 120, "index %d not 0-based", indices[i]);

  float Rt_test[12];
  int numInliers[1] = {-1};
  const float thresh2 = 0.05f * 0.05f;
  std::vector<float> h_coord(6 * matches.size());
  for (size_t i = 0; i < matches.size(); i++) {
    memcpy(&h_coord[6 * i], matches[i]->pt1->coords3D, sizeof(float) * 3);
    memcpy(&h_coord[6 * i + 3], matches[i]->pt2->coords3D, sizeof(float) * 3);
  }
  std::vector<char> h_inliers(matches.size(), 2);
  const std::vector<int> before(indices);
  EstimateRigidTransformH(h_coord.data(), Rt_test, numInliers, numLoops, (int)matches.size(), thresh2, RigidTransformType3D,
                          &indices[0], h_inliers.data());
  std::printf("RANSACWithIndices: inliers / total: %d / %zu\n", numInliers[0], matches.size());
  print_rt("  Rt (device)", Rt_test);
  print_rt("  Rt (MATLAB)", Rt);
  EXPECT(numInliers[0] == 114, "inliers %d, expected 114", numInliers[0]);
  EXPECT(indices == before, "h_indices was written");
  int flagged = 0;
  double yc[3] = {0, 0, 0};
  for (size_t i = 0; i < matches.size(); i++) {
    EXPECT(h_inliers[i] == 0 || h_inliers[i] == 1, "flag %d of point %zu", (int)h_inliers[i], i);
    if (h_inliers[i] == 1) {
      flagged++;
      for (int k = 0; k < 3; k++) yc[k] += h_coord[6 * i + 3 + k];
    }
  }
  EXPECT(flagged == 114, "%d flags set", flagged);
  // The refit's B has the float64 eigenvalues 0.043, 23.0, 62.9, 79.9: relative gap g = (23.0 - 0.043) / 79.9 = 0.287,
  // rotation bound beta = 32 * 2^-24 / g; t = xc - R yc inherits beta * |yc| (+ 1e-6 for its own rounding).
  const double beta = 32.0 * std::ldexp(1.0, -24) / ((23.0 - 0.043) / 79.9);
  const double ynorm = std::sqrt(yc[0] * yc[0] + yc[1] * yc[1] + yc[2] * yc[2]) / (flagged > 0 ? flagged : 1);
  double dr = 0, dt = 0;
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) dr += ((double)Rt_test[4 * i + j] - Rt[4 * i + j]) * ((double)Rt_test[4 * i + j] - Rt[4 * i + j]);
    dt += ((double)Rt_test[4 * i + 3] - Rt[4 * i + 3]) * ((double)Rt_test[4 * i + 3] - Rt[4 * i + 3]);
  }
  dr = std::sqrt(dr / 2.0);
  dt = std::sqrt(dt);
  std::printf("  |dR|_F / sqrt2 = %.3g (bound %.3g), |dt| = %.3g (bound %.3g)\n", dr, beta, dt, beta * ynorm + 1e-6);
  EXPECT(dr <= beta, "R differs from the fixture by %.3g > %.3g", dr, beta);
  EXPECT(dt <= beta * ynorm + 1e-6, "t differs from the fixture by %.3g > %.3g", dt, beta * ynorm + 1e-6);
  free_matches(matches);
}

static void ransac_with_random(const char *path) {
  std::vector<int> indices;
  float Rt[12];
  std::vector<SiftMatch *> matches = ReadMATLABRANSAC(path, indices, Rt);
  if (matches.empty()) {
    EXPECT(false, "cannot read %s", path);
    return;
  }
  const int numLoops = 4096;
  float Rt_test[12];
  int numInliers[1] = {-1};
  EstimateRigidTransform(matches, Rt_test, numInliers, numLoops, 0.05f, RigidTransformType3D);
  std::printf("RANSACWithRandom: inliers / total: %d / %zu\n", numInliers[0], matches.size());
  print_rt("  Rt (device)", Rt_test);
  // the best of the ten given triples already reaches 114
  EXPECT(numInliers[0] >= 114 && numInliers[0] <= 120, "inliers %d", numInliers[0]);
  for (int i = 0; i < 12; i++)
    EXPECT(std::fabs(Rt_test[i] - Rt[i]) <= 0.01f, "Rt[%d] = %f, fixture %f", i, Rt_test[i], Rt[i]);
  free_matches(matches);
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: %s rigid_ransac.bin\n", argv[0]);
    return 2;
  }
  InitCuda(0);
  ransac_with_indices(argv[1]);
  ransac_with_random(argv[1]);
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
