// The reference's demo chain (main.cpp:331-335: MatchSiftData, FindHomography, ImproveHomography) on the device:
// EstimateHomography and RegisterPlanar of include/homography.h against the unchanged host ImproveHomography.
//
// Two frames with a planted homography and gross outliers; every record of frame 1 has its partner's descriptor, so the
// matcher pairs them with a dot product of 1.  Checked:
//   * EstimateHomography's refined H against the host ImproveHomography started from the same winner (h_ransac) on a
//     synchronised copy: the mapped corners agree within max(64 d_order, r32), where d_order is what reversing the
//     summation order does to a float64 restatement of the refit and r32 what one fp32 ulp on each coefficient can do;
//   * match_error of every device record against a float64 evaluation with the device's own H, within 8 * 2^-24 * S
//     (S = the largest coordinate magnitude);
//   * RegisterPlanar = cusift_match + EstimateHomography, bit for bit; the same seed twice gives the same bits.
// Plain C++ (g++), no HIP headers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cuSIFT.h"
#include "homography.h"

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

static const double kCorners[4][2] = {{0, 0}, {1280, 0}, {0, 960}, {1280, 960}};

template <class T, class U>
static double corner_distance(const T *a, const U *b) {
  double worst = 0.0;
  for (const auto &c : kCorners) {
    const double d0 = (double)a[6] * c[0] + (double)a[7] * c[1] + 1.0, d1 = (double)b[6] * c[0] + (double)b[7] * c[1] + 1.0;
    const double ex = ((double)a[0] * c[0] + (double)a[1] * c[1] + (double)a[2]) / d0 -
                      ((double)b[0] * c[0] + (double)b[1] * c[1] + (double)b[2]) / d1;
    const double ey = ((double)a[3] * c[0] + (double)a[4] * c[1] + (double)a[5]) / d0 -
                      ((double)b[3] * c[0] + (double)b[4] * c[1] + (double)b[5]) / d1;
    worst = std::fmax(worst, std::sqrt(ex * ex + ey * ey));
  }
  return worst;
}

// ImproveHomography's rounds (include/homography.h:109-130) with A kept in double, summed forwards or backwards
static void improve_double(const SiftPoint *pts, int n, const float *start, int loops, float lo, float hi, float thresh,
                           bool reverse, double A[8]) {
  const float limit = thresh * thresh;
  for (int i = 0; i < 8; i++) A[i] = start[i] / start[8];
  for (int loop = 0; loop < loops; loop++) {
    double M[8][8] = {{0}}, X[8] = {0};
    for (int k = 0; k < n; k++) {
      const SiftPoint &pt = pts[reverse ? n - 1 - k : k];
      if (pt.score < lo || pt.ambiguity > hi) continue;
      const float px = pt.coords2D[0], py = pt.coords2D[1];
      const float den = (float)(A[6] * px + A[7] * py + 1.0f);
      const float dx = (float)((A[0] * px + A[1] * py + A[2]) / den - pt.match_xpos);
      const float dy = (float)((A[3] * px + A[4] * py + A[5]) / den - pt.match_ypos);
      const float err = dx * dx + dy * dy;
      const float wei = limit / (err + limit);
      const double Yx[8] = {px, py, 1.0, 0.0, 0.0, 0.0, -(double)(px * pt.match_xpos), -(double)(py * pt.match_xpos)};
      const double Yy[8] = {0.0, 0.0, 0.0, px, py, 1.0, -(double)(px * pt.match_ypos), -(double)(py * pt.match_ypos)};
      for (int c = 0; c < 8; c++) {
        for (int r = 0; r < 8; r++) M[r][c] += Yx[c] * Yx[r] * wei + Yy[c] * Yy[r] * wei;
        X[c] += Yx[c] * pt.match_xpos * wei + Yy[c] * pt.match_ypos * wei;
      }
    }
    cusift_dropin::cholesky_solve8(M, X, A);
  }
}

int main() {
  InitCuda(0);
  {
    const double H[9] = {0.92, -0.11, 37.0, 0.08, 1.05, -21.0, 2.1e-5, -3.4e-5, 1.0};
    const int nIn = 600, nOut = 400, n = nIn + nOut;
    const float lo = 0.85f, hi = 0.95f;
    std::vector<SiftPoint> f1((size_t)n), f2((size_t)n);
    std::memset(f1.data(), 0, sizeof(SiftPoint) * n);
    std::memset(f2.data(), 0, sizeof(SiftPoint) * n);
    float S = 0.0f;
    for (int i = 0; i < n; i++) {
      const int j = (i * 7 + 3) % n;  // the partner's slot in frame 2 (7 and 1000 are coprime)
      SiftPoint &p = f1[i], &q = f2[j];
      const double x = 1280.0 * uniform01(), y = 960.0 * uniform01();
      p.coords2D[0] = (float)x, p.coords2D[1] = (float)y;
      const bool inlier = (i % 5) != 1 && (i % 5) != 3;  // 60 % inliers, interleaved
      if (inlier) {
        const double den = H[6] * x + H[7] * y + 1.0;
        q.coords2D[0] = (float)((H[0] * x + H[1] * y + H[2]) / den + 0.6 * (uniform01() - 0.5));
        q.coords2D[1] = (float)((H[3] * x + H[4] * y + H[5]) / den + 0.6 * (uniform01() - 0.5));
      } else {
        q.coords2D[0] = (float)(1280.0 * uniform01()), q.coords2D[1] = (float)(960.0 * uniform01());
      }
      double norm = 0.0;
      for (int d = 0; d < 128; d++) {
        p.data[d] = (float)uniform01();
        norm += (double)p.data[d] * p.data[d];
      }
      for (int d = 0; d < 128; d++) q.data[d] = p.data[d] = (float)(p.data[d] / std::sqrt(norm));
      S = std::fmax(S, std::fmax(std::fmax(std::fabs(p.coords2D[0]), std::fabs(p.coords2D[1])),
                                 std::fmax(std::fabs(q.coords2D[0]), std::fabs(q.coords2D[1]))));
    }
    auto upload = [&](SiftData &d, const std::vector<SiftPoint> &src) {
      InitSiftData(d, n, true, true);
      std::memcpy(d.h_data, src.data(), sizeof(SiftPoint) * n);
      d.numPts = n;
      safeCall(cusift_memcpy_h2d(cusift_dropin::ctx(), d.d_data, d.h_data, sizeof(SiftPoint) * n));
    };

    // ---- two steps: the matcher, then EstimateHomography ----
    SiftData a1, a2;
    upload(a1, f1);
    upload(a2, f2);
    safeCall(cusift_match(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(a1.d_data), n,
                          reinterpret_cast<const cusift_point *>(a2.d_data), n, 0));
    float Hdev[9], Rdev[9];
    int numMatches = -1, numFit = -1;
    EstimateHomography(a1, Hdev, &numMatches, &numFit, 1000, lo, hi, 5.0f, 5, 3.0f, 11, 0, Rdev, n);
    a1.Synchronize();
    std::printf("EstimateHomography: %d inliers, %d within 3 px of the refit (%d planted of %d)\n", numMatches, numFit, nIn, n);
    EXPECT(numMatches >= (int)(0.9 * nIn) && numMatches <= nIn + 40, "%d inliers", numMatches);
    EXPECT(numFit >= (int)(0.97 * nIn) && numFit <= nIn + 25, "%d fit", numFit);
    EXPECT(Hdev[8] == 1.0f && Rdev[8] == 1.0f, "h[8] != 1");
    int paired = 0;
    for (int i = 0; i < n; i++) paired += a1.h_data[i].match == (i * 7 + 3) % n;
    EXPECT(paired == n, "%d of %d records found their partner", paired, n);
    std::vector<float> devErr((size_t)n);
    for (int i = 0; i < n; i++) devErr[i] = a1.h_data[i].match_error;

    // the unchanged host refit from the same winner, on the synchronised copy
    float Hhost[9];
    std::memcpy(Hhost, Rdev, sizeof(Hhost));
    const int hostFit = ImproveHomography(a1, Hhost, 5, lo, hi, 3.0f);
    double Af[8], Ab[8];
    improve_double(a1.h_data, n, Rdev, 5, lo, hi, 3.0f, false, Af);
    improve_double(a1.h_data, n, Rdev, 5, lo, hi, 3.0f, true, Ab);
    for (int i = 0; i < 8; i++) EXPECT((float)Af[i] == Hhost[i], "the restatement is not ImproveHomography at %d", i);
    const double dOrder = corner_distance(Af, Ab);
    double r32 = 0.0;
    for (int i = 0; i < 8; i++) {
      float up[9];
      std::memcpy(up, Hhost, sizeof(up));
      up[i] = std::nextafterf(up[i], INFINITY);
      r32 += corner_distance(up, Hhost);
    }
    const double bound = std::fmax(64.0 * dOrder, r32), got = corner_distance(Hdev, Hhost);
    std::printf("corners: device against host refit %.3g px (bound %.3g: d_order %.3g, r32 %.3g); against the planted "
                "homography %.3f px; host numFit %d\n", got, bound, dOrder, r32, corner_distance(Hdev, H), hostFit);
    EXPECT(got <= bound, "corners %.3g px apart, bound %.3g", got, bound);
    EXPECT(corner_distance(Hdev, H) < 0.5, "refined homography %.3f px from the planted one", corner_distance(Hdev, H));
    EXPECT(std::abs(numFit - hostFit) <= n / 100, "numFit %d, host %d", numFit, hostFit);

    // match_error of every record against float64 with the device's own H
    const double tol = 8.0 * std::ldexp(1.0, -24) * S;
    double worstErr = 0.0;
    for (int i = 0; i < n; i++) {
      const SiftPoint &pt = a1.h_data[i];
      const double den = (double)Hdev[6] * pt.coords2D[0] + (double)Hdev[7] * pt.coords2D[1] + 1.0;
      const double dx = ((double)Hdev[0] * pt.coords2D[0] + (double)Hdev[1] * pt.coords2D[1] + Hdev[2]) / den - pt.match_xpos;
      const double dy = ((double)Hdev[3] * pt.coords2D[0] + (double)Hdev[4] * pt.coords2D[1] + Hdev[5]) / den - pt.match_ypos;
      worstErr = std::fmax(worstErr, std::fabs(std::sqrt(dx * dx + dy * dy) - devErr[i]));
    }
    std::printf("match_error: worst deviation from float64 %.3g px (bound %.3g)\n", worstErr, tol);
    EXPECT(worstErr <= tol, "match_error off by %.3g, bound %.3g", worstErr, tol);

    // ---- one step ----
    float H1[9], R1[9], H2[9], R2[9];
    int m1 = -1, fit1 = -1, m2 = -1, fit2 = -1;
    {
      SiftData b1, b2;
      upload(b1, f1);
      upload(b2, f2);
      RegisterPlanar(b1, b2, H1, &m1, &fit1, 1000, lo, hi, 5.0f, 5, 3.0f, 11, 0, 0, R1);
      b1.Synchronize();
      int same = 0;
      for (int i = 0; i < n; i++) same += std::memcmp(&b1.h_data[i].match_error, &devErr[i], sizeof(float)) == 0;
      EXPECT(same == n, "match_error of %d records differs from the two-step route", n - same);
    }
    {
      SiftData b1, b2;
      upload(b1, f1);
      upload(b2, f2);
      RegisterPlanar(b1, b2, H2, &m2, &fit2, 1000, lo, hi, 5.0f, 5, 3.0f, 11, 0, 0, R2);
    }
    std::printf("RegisterPlanar: %d inliers, %d fit\n", m1, fit1);
    EXPECT(std::memcmp(H1, Hdev, sizeof(H1)) == 0 && std::memcmp(R1, Rdev, sizeof(R1)) == 0 && m1 == numMatches && fit1 == numFit,
           "RegisterPlanar differs from cusift_match + EstimateHomography");
    EXPECT(std::memcmp(H1, H2, sizeof(H1)) == 0 && std::memcmp(R1, R2, sizeof(R1)) == 0 && m1 == m2 && fit1 == fit2,
           "the same seed gave another answer");

    // fewer than 8 records: identity, zero counts (extras/homography.cu:205)
    SiftData tiny;
    InitSiftData(tiny, 4, true, true);
    tiny.numPts = 4;
    float h3[9];
    int m3 = -1, fit3 = -1;
    EstimateHomography(tiny, h3, &m3, &fit3);
    EXPECT(m3 == 0 && fit3 == 0 && h3[0] == 1.0f && h3[4] == 1.0f && h3[8] == 1.0f && h3[1] == 0.0f, "tiny set");
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
