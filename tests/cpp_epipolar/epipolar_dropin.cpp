// EstimateFundamental and RegisterEpipolar of include/epipolar.h on two views of a planted, non-planar scene.
//
// 3-D points in front of two 1280 x 960 cameras (f = 1000; the second turned 0.15 rad about y and moved 0.8 along x),
// 0.3 px of noise, gross outliers; every record of frame 1 has its partner's descriptor, so the matcher pairs them with a
// dot product of 1.  Checked:
//   * F has Frobenius norm 1 and determinant 0 within 1e-12, and lies close to the planted geometry: at least 99 % of the
//     planted inliers have match_error < 1 px (printed beside it: how many the planted F itself keeps within 1 px);
//   * the two thresholds differ (0.75 px for the hypotheses, 1 px for the refit), so that neither can stand in for the
//     other: numMatches against a double restatement of the pinned inlier test with the device's own winner at 0.75 px,
//     numFit with the device's own F at 1 px, both exactly; match_error within 1e-5 relative;
//   * RegisterEpipolar = cusift_match + EstimateFundamental, byte for byte; the same seed twice gives the same bytes;
//   * fewer than 8 records: nine zeros, zero counts.
// Plain C++ (g++), no HIP headers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cuSIFT.h"
#include "epipolar.h"

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
static double gauss() {  // Box-Muller
  const double u = 1.0 - uniform01(), v = uniform01();
  return std::sqrt(-2.0 * std::log(u)) * std::cos(6.283185307179586 * v);
}

// the pinned inlier test of cusift_amd_extras.h: e * e and den
static void sampson(const double *F, double x1, double y1, double x2, double y2, double *e2, double *den) {
  const double l0 = (F[0] * x1 + F[1] * y1) + F[2];
  const double l1 = (F[3] * x1 + F[4] * y1) + F[5];
  const double l2 = (F[6] * x1 + F[7] * y1) + F[8];
  const double m0 = (F[0] * x2 + F[3] * y2) + F[6];
  const double m1 = (F[1] * x2 + F[4] * y2) + F[7];
  const double e = (x2 * l0 + y2 * l1) + l2;
  *den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1;
  *e2 = e * e;
}

int main() {
  InitCuda(0);
  {
    const int nIn = 600, nOut = 400, n = nIn + nOut;
    const float lo = 0.85f, hi = 0.95f;
    const float thresh = 0.75f, refineThresh = 1.0f;  // apart: the winner's count is taken at one, numFit at the other
    const double t2 = (double)thresh * thresh, rt2 = (double)refineThresh * refineThresh;
    const double f = 1000.0, cx = 640.0, cy = 480.0, ang = 0.15, base = 0.8;
    const double ca = std::cos(ang), sa = std::sin(ang);
    // X2 = R X1 + t with R a turn about y and t = -R C, C = (base, 0, 0); F = K^-T [t]x R K^-1
    const double R[9] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca};
    const double t[3] = {-ca * base, 0.0, sa * base};
    const double tx[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
    const double Ki[9] = {1 / f, 0, -cx / f, 0, 1 / f, -cy / f, 0, 0, 1};
    double E[9], EK[9], Ftrue[9];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        E[3 * i + j] = 0;
        for (int k = 0; k < 3; k++) E[3 * i + j] += tx[3 * i + k] * R[3 * k + j];
      }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        EK[3 * i + j] = 0;
        for (int k = 0; k < 3; k++) EK[3 * i + j] += E[3 * i + k] * Ki[3 * k + j];
      }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        Ftrue[3 * i + j] = 0;
        for (int k = 0; k < 3; k++) Ftrue[3 * i + j] += Ki[3 * k + i] * EK[3 * k + j];
      }
    std::vector<SiftPoint> f1((size_t)n), f2((size_t)n);
    std::memset(f1.data(), 0, sizeof(SiftPoint) * n);
    std::memset(f2.data(), 0, sizeof(SiftPoint) * n);
    std::vector<char> planted((size_t)n);
    for (int i = 0; i < n; i++) {
      const int j = (i * 7 + 3) % n;  // the partner's slot in frame 2 (7 and 1000 are coprime)
      SiftPoint &p = f1[i], &q = f2[j];
      planted[i] = (i % 5) != 1 && (i % 5) != 3;  // 60 % inliers, interleaved
      if (planted[i]) {
        for (;;) {  // a point both cameras see
          const double X = -3.0 + 6.0 * uniform01(), Y = -2.0 + 4.0 * uniform01(), Z = 3.0 + 9.0 * uniform01();
          const double X2 = R[0] * X + R[2] * Z + t[0], Y2 = Y, Z2 = R[6] * X + R[8] * Z + t[2];
          const double u1 = f * X / Z + cx, v1 = f * Y / Z + cy, u2 = f * X2 / Z2 + cx, v2 = f * Y2 / Z2 + cy;
          if (u1 < 0 || u1 >= 1280 || v1 < 0 || v1 >= 960 || u2 < 0 || u2 >= 1280 || v2 < 0 || v2 >= 960) continue;
          p.coords2D[0] = (float)(u1 + 0.3 * gauss()), p.coords2D[1] = (float)(v1 + 0.3 * gauss());
          q.coords2D[0] = (float)(u2 + 0.3 * gauss()), q.coords2D[1] = (float)(v2 + 0.3 * gauss());
          break;
        }
      } else {
        p.coords2D[0] = (float)(1280.0 * uniform01()), p.coords2D[1] = (float)(960.0 * uniform01());
        q.coords2D[0] = (float)(1280.0 * uniform01()), q.coords2D[1] = (float)(960.0 * uniform01());
      }
      double norm = 0.0;
      for (int d = 0; d < 128; d++) {
        p.data[d] = (float)uniform01();
        norm += (double)p.data[d] * p.data[d];
      }
      for (int d = 0; d < 128; d++) q.data[d] = p.data[d] = (float)(p.data[d] / std::sqrt(norm));
    }
    auto upload = [&](SiftData &d, const std::vector<SiftPoint> &src) {
      InitSiftData(d, n, true, true);
      std::memcpy(d.h_data, src.data(), sizeof(SiftPoint) * n);
      d.numPts = n;
      safeCall(cusift_memcpy_h2d(cusift_dropin::ctx(), d.d_data, d.h_data, sizeof(SiftPoint) * n));
    };

    // ---- two steps: the matcher, then EstimateFundamental ----
    SiftData a1, a2;
    upload(a1, f1);
    upload(a2, f2);
    safeCall(cusift_match(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(a1.d_data), n,
                          reinterpret_cast<const cusift_point *>(a2.d_data), n, 0));
    double Fdev[9], Rdev[9];
    int numMatches = -1, numFit = -1;
    EstimateFundamental(a1, Fdev, &numMatches, &numFit, 1000, lo, hi, thresh, 5, refineThresh, 11, 0, Rdev, n);
    a1.Synchronize();
    std::printf("EstimateFundamental: %d inliers within %.2f px of the winner, %d within %.2f px of the refit (%d planted of %d)\n",
                numMatches, thresh, numFit, refineThresh, nIn, n);
    int paired = 0;
    for (int i = 0; i < n; i++) paired += a1.h_data[i].match == (i * 7 + 3) % n;
    EXPECT(paired == n, "%d of %d records found their partner", paired, n);
    double norm = 0.0;
    for (int i = 0; i < 9; i++) norm += Fdev[i] * Fdev[i];
    const double det = Fdev[0] * (Fdev[4] * Fdev[8] - Fdev[5] * Fdev[7]) - Fdev[1] * (Fdev[3] * Fdev[8] - Fdev[5] * Fdev[6]) +
                       Fdev[2] * (Fdev[3] * Fdev[7] - Fdev[4] * Fdev[6]);
    EXPECT(std::fabs(std::sqrt(norm) - 1.0) <= 1e-12 && std::fabs(det) <= 1e-12, "norm %.17g, det %.3g", std::sqrt(norm), det);
    // numFit and match_error from the device's own F, in double
    int fit = 0, fitTight = 0, won = 0, good = 0, goodTrue = 0;
    double worst = 0.0;
    for (int i = 0; i < n; i++) {
      const SiftPoint &pt = a1.h_data[i];
      double e2, den;
      sampson(Fdev, pt.coords2D[0], pt.coords2D[1], pt.match_xpos, pt.match_ypos, &e2, &den);
      fit += e2 < rt2 * den;  // every record is a candidate here (the matcher's scores are 1)
      fitTight += e2 < t2 * den;
      const double err = std::sqrt(e2 / den);
      worst = std::fmax(worst, std::fabs(err - pt.match_error) / std::fmax(err, 1e-30));
      good += planted[i] && pt.match_error < 1.0f;
      sampson(Ftrue, pt.coords2D[0], pt.coords2D[1], pt.match_xpos, pt.match_ypos, &e2, &den);
      goodTrue += planted[i] && e2 < den;
      sampson(Rdev, pt.coords2D[0], pt.coords2D[1], pt.match_xpos, pt.match_ypos, &e2, &den);
      won += e2 < t2 * den;
    }
    std::printf("planted inliers within 1 px: %d under the device's F, %d under the planted F, of %d; match_error off by "
                "%.3g relative\n", good, goodTrue, nIn, worst);
    EXPECT(fit == numFit, "numFit %d, the restatement counts %d", numFit, fit);
    EXPECT(won == numMatches, "numMatches %d, the restatement counts %d under the winner", numMatches, won);
    EXPECT(worst <= 1e-5, "match_error off by %.3g relative", worst);
    EXPECT(good >= (int)std::ceil(0.99 * nIn), "%d of %d planted inliers within 1 px", good, nIn);
    // the winner comes from eight noisy points: it holds its own samples, and the refit over its inliers gains on it
    // -- at the winner's own threshold, and all the more at the wider one
    EXPECT(numMatches >= 8 && numMatches <= n && fitTight >= numMatches && numFit >= numMatches,
           "%d inliers, %d fit at the same threshold, %d fit", numMatches, fitTight, numFit);
    std::vector<float> devErr((size_t)n);
    for (int i = 0; i < n; i++) devErr[i] = a1.h_data[i].match_error;

    // ---- one step ----
    double F1[9], R1[9], F2[9], R2[9];
    int m1 = -1, fit1 = -1, m2 = -1, fit2 = -1;
    {
      SiftData b1, b2;
      upload(b1, f1);
      upload(b2, f2);
      RegisterEpipolar(b1, b2, F1, &m1, &fit1, 1000, lo, hi, thresh, 5, refineThresh, 11, 0, 0, R1);
      b1.Synchronize();
      int same = 0;
      for (int i = 0; i < n; i++) same += std::memcmp(&b1.h_data[i].match_error, &devErr[i], sizeof(float)) == 0;
      EXPECT(same == n, "match_error of %d records differs from the two-step route", n - same);
    }
    {
      SiftData b1, b2;
      upload(b1, f1);
      upload(b2, f2);
      RegisterEpipolar(b1, b2, F2, &m2, &fit2, 1000, lo, hi, thresh, 5, refineThresh, 11, 0, 0, R2);
    }
    std::printf("RegisterEpipolar: %d inliers, %d fit\n", m1, fit1);
    EXPECT(std::memcmp(F1, Fdev, sizeof(F1)) == 0 && std::memcmp(R1, Rdev, sizeof(R1)) == 0 && m1 == numMatches && fit1 == numFit,
           "RegisterEpipolar differs from cusift_match + EstimateFundamental");
    EXPECT(std::memcmp(F1, F2, sizeof(F1)) == 0 && std::memcmp(R1, R2, sizeof(R1)) == 0 && m1 == m2 && fit1 == fit2,
           "the same seed gave another answer");

    // fewer than 8 records: nine zeros, zero counts
    SiftData tiny;
    InitSiftData(tiny, 4, true, true);
    tiny.numPts = 4;
    double f3[9];
    int m3 = -1, fit3 = -1;
    for (double &v : f3) v = 7.0;
    EstimateFundamental(tiny, f3, &m3, &fit3);
    bool zeros = true;
    for (double v : f3) zeros = zeros && v == 0.0;
    EXPECT(m3 == 0 && fit3 == 0 && zeros, "tiny set");
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
