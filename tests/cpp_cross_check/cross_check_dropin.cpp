// SetCrossCheck (include/matching.h) from plain C++ (g++), no HIP headers: RegisterPlanar on a planted pair with and
// without the cross-check.
//
// Frame 2 has kTrue + kSpare records with distinct descriptors.  Records 0 .. kTrue - 1 of frame 1 carry the descriptor
// of their partner in frame 2 and follow a planted homography; records kTrue .. kTrue + kExtra - 1 are exact copies of the
// descriptors of kExtra true records at random positions: many-to-one matches whose score ties the true record's bit for
// bit, so the column side keeps the true, lower record.  Checked: the candidates are kTrue + kExtra without the
// cross-check and kTrue with it, no copy is an inlier with it, both runs recover the homography, the match fields of
// frame 2 are written only while it is on, and turning it off again gives the first run's bits.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cuSIFT.h"
#include "homography.h"
#include "matching.h"

static int failures = 0;
#define EXPECT(cond, ...)                                \
  do {                                                   \
    if (!(cond)) {                                       \
      std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                          \
      std::printf("\n");                                 \
      ++failures;                                        \
    }                                                    \
  } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uniform01() {  // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) / 9007199254740992.0;
}

static const int kTrue = 600, kExtra = 150, kSpare = 40, kN1 = kTrue + kExtra, kN2 = kTrue + kSpare;
static const double kH[9] = {0.92, -0.11, 37.0, 0.08, 1.05, -21.0, 2.1e-5, -3.4e-5, 1.0};

static double corner_distance(const float *a) {
  const double corners[4][2] = {{0, 0}, {1280, 0}, {0, 960}, {1280, 960}};
  double worst = 0.0;
  for (const auto &c : corners) {
    const double d0 = (double)a[6] * c[0] + (double)a[7] * c[1] + 1.0, d1 = kH[6] * c[0] + kH[7] * c[1] + 1.0;
    const double ex = ((double)a[0] * c[0] + (double)a[1] * c[1] + (double)a[2]) / d0 - (kH[0] * c[0] + kH[1] * c[1] + kH[2]) / d1;
    const double ey = ((double)a[3] * c[0] + (double)a[4] * c[1] + (double)a[5]) / d0 - (kH[3] * c[0] + kH[4] * c[1] + kH[5]) / d1;
    worst = std::fmax(worst, std::sqrt(ex * ex + ey * ey));
  }
  return worst;
}

struct Result {
  float H[9], R[9];
  int candidates, matches, fit;
  std::vector<char> inliers;
  std::vector<SiftPoint> frame1, frame2;  // the device records afterwards
};

static Result run(const std::vector<SiftPoint> &f1, const std::vector<SiftPoint> &f2) {
  SiftData d1, d2;
  auto upload = [](SiftData &d, const std::vector<SiftPoint> &src) {
    InitSiftData(d, (int)src.size(), true, true);
    std::memcpy(d.h_data, src.data(), sizeof(SiftPoint) * src.size());
    d.numPts = (int)src.size();
    safeCall(cusift_memcpy_h2d(cusift_dropin::ctx(), d.d_data, d.h_data, sizeof(SiftPoint) * src.size()));
  };
  upload(d1, f1);
  upload(d2, f2);
  Result r;
  r.candidates = r.matches = r.fit = -1;
  r.inliers.assign((size_t)kN1, 9);
  // the C call, which RegisterPlanar wraps, for the candidate count and the flags
  safeCall(cusift_register_planar(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(d1.d_data), kN1,
                                  reinterpret_cast<const cusift_point *>(d2.d_data), kN2, 0, 0, 0.85f, 0.95f, 1008, 5.0f, 5,
                                  3.0f, 11, r.H, r.R, &r.candidates, &r.matches, &r.fit, nullptr, r.inliers.data(), nullptr,
                                  nullptr, nullptr));
  float H2[9], R2[9];
  int m2 = -1, fit2 = -1;
  {
    SiftData e1, e2;
    upload(e1, f1);
    upload(e2, f2);
    RegisterPlanar(e1, e2, H2, &m2, &fit2, 1000, 0.85f, 0.95f, 5.0f, 5, 3.0f, 11, 0, 0, R2);  // 1000 loops round up to 1008
  }
  EXPECT(std::memcmp(H2, r.H, sizeof(H2)) == 0 && std::memcmp(R2, r.R, sizeof(R2)) == 0 && m2 == r.matches && fit2 == r.fit,
         "RegisterPlanar differs from cusift_register_planar on the same context");
  d1.Synchronize();
  d2.Synchronize();
  r.frame1.assign(d1.h_data, d1.h_data + kN1);
  r.frame2.assign(d2.h_data, d2.h_data + kN2);
  return r;
}

int main() {
  InitCuda(0);
  {
    std::vector<SiftPoint> f1((size_t)kN1), f2((size_t)kN2);
    std::memset(f1.data(), 0, sizeof(SiftPoint) * f1.size());
    std::memset(f2.data(), 0, sizeof(SiftPoint) * f2.size());
    for (int j = 0; j < kN2; j++) {
      SiftPoint &q = f2[j];
      double norm = 0.0;
      for (int d = 0; d < 128; d++) {
        q.data[d] = (float)uniform01();
        norm += (double)q.data[d] * q.data[d];
      }
      for (int d = 0; d < 128; d++) q.data[d] = (float)(q.data[d] / std::sqrt(norm));
      q.coords2D[0] = (float)(1280.0 * uniform01()), q.coords2D[1] = (float)(960.0 * uniform01());
      q.match = -7;  // a mark: untouched unless the cross-check writes it
    }
    for (int i = 0; i < kTrue; i++) {
      const int j = (i * 7 + 3) % kN2;  // the partner's slot in frame 2 (7 and 640 are coprime)
      SiftPoint &p = f1[i], &q = f2[j];
      std::memcpy(p.data, q.data, sizeof(p.data));
      const double x = 1280.0 * uniform01(), y = 960.0 * uniform01();
      p.coords2D[0] = (float)x, p.coords2D[1] = (float)y;
      const double den = kH[6] * x + kH[7] * y + 1.0;
      q.coords2D[0] = (float)((kH[0] * x + kH[1] * y + kH[2]) / den + 0.6 * (uniform01() - 0.5));
      q.coords2D[1] = (float)((kH[3] * x + kH[4] * y + kH[5]) / den + 0.6 * (uniform01() - 0.5));
    }
    for (int k = 0; k < kExtra; k++) {  // copies of every fourth true record, at positions of their own
      SiftPoint &p = f1[kTrue + k];
      std::memcpy(p.data, f1[4 * k].data, sizeof(p.data));
      p.coords2D[0] = (float)(1280.0 * uniform01()), p.coords2D[1] = (float)(960.0 * uniform01());
    }

    const Result off = run(f1, f2);
    SetCrossCheck(true);
    const Result on = run(f1, f2);
    SetCrossCheck(false);
    const Result again = run(f1, f2);

    std::printf("cross-check off: %d candidates, %d inliers, %d fit, corners %.3f px from the planted homography\n",
                off.candidates, off.matches, off.fit, corner_distance(off.H));
    std::printf("cross-check on:  %d candidates, %d inliers, %d fit, corners %.3f px\n", on.candidates, on.matches, on.fit,
                corner_distance(on.H));
    EXPECT(off.candidates == kTrue + kExtra, "%d candidates without the cross-check, expected %d", off.candidates, kN1);
    EXPECT(on.candidates == kTrue, "%d candidates with the cross-check, expected %d", on.candidates, kTrue);
    EXPECT(corner_distance(off.H) < 0.5 && corner_distance(on.H) < 0.5, "the homography is not recovered");
    EXPECT(on.matches >= (int)(0.97 * kTrue) && on.matches <= kTrue, "%d inliers with the cross-check", on.matches);
    int flagged = 0, named = 0, written_off = 0, written_on = 0;
    for (int k = 0; k < kExtra; k++) flagged += on.inliers[kTrue + k] != 0;
    EXPECT(flagged == 0, "%d copies are inliers with the cross-check on", flagged);
    for (int i = 0; i < kTrue; i++) named += on.frame2[(i * 7 + 3) % kN2].match == i && on.frame1[i].match == (i * 7 + 3) % kN2;
    EXPECT(named == kTrue, "%d of %d true records are mutual", named, kTrue);
    for (int j = 0; j < kN2; j++) written_off += off.frame2[j].match != -7, written_on += on.frame2[j].match != -7;
    EXPECT(written_off == 0 && written_on == kN2, "frame 2's match fields: %d written when off, %d when on", written_off,
           written_on);
    EXPECT(std::memcmp(again.H, off.H, sizeof(off.H)) == 0 && std::memcmp(again.R, off.R, sizeof(off.R)) == 0 &&
               again.candidates == off.candidates && again.matches == off.matches && again.fit == off.fit &&
               again.inliers == off.inliers &&
               std::memcmp(again.frame1.data(), off.frame1.data(), sizeof(SiftPoint) * kN1) == 0 &&
               std::memcmp(again.frame2.data(), off.frame2.data(), sizeof(SiftPoint) * kN2) == 0,
           "turning the cross-check off again does not give the first run's bits");
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
