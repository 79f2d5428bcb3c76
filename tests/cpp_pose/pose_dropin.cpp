// RegisterPose and EstimatePose of include/pose.h on two views of a planted, non-planar scene.
//
// The scene of tests/cpp_epipolar: 3-D points in front of two 1280 x 960 cameras (f = 1000; the second turned 0.15 rad
// about y and moved 0.8 along x), 0.3 px of noise, 40 % gross outliers; every record of frame 1 has its partner's
// descriptor, so the matcher pairs them with a dot product of 1.  Checked:
//   * RegisterPose: R within 0.25 degrees of the planted rotation, t within 1.5 degrees of the planted direction, |t| = 1,
//     R orthonormal with determinant +1; at least 99 % of the planted records carry a point, and at least 90 % of those
//     lie within 5 % of the planted 3-D point once scaled by the planted baseline; a record with no point is all zeros;
//   * EstimatePose with the F that RegisterPose returned gives the same Rt, counts and coords3D, byte for byte;
//   * cusift_estimate_pose refuses a NULL camera and writes nothing; F of nine zeros is the degenerate answer.
// Plain C++ (g++), no HIP headers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cuSIFT.h"
#include "pose.h"

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

int main() {
  InitCuda(0);
  {
    const int nIn = 600, nOut = 400, n = nIn + nOut;
    const float lo = 0.85f, hi = 0.95f;
    const double f = 1000.0, cx = 640.0, cy = 480.0, ang = 0.15, base = 0.8;
    const double ca = std::cos(ang), sa = std::sin(ang);
    // X2 = R X1 + t with R a turn about y and t = -R C, C = (base, 0, 0); so X1 = R^T X2 + C
    const double R[9] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca};
    const double t[3] = {-ca * base, 0.0, sa * base};
    cusift_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.fx = (float)f, cam.fy = (float)f, cam.cx = (float)cx, cam.cy = (float)cy, cam.origin = 0.0f;
    std::vector<SiftPoint> f1((size_t)n), f2((size_t)n);
    std::memset(f1.data(), 0, sizeof(SiftPoint) * n);
    std::memset(f2.data(), 0, sizeof(SiftPoint) * n);
    std::vector<char> planted((size_t)n);
    std::vector<double> world(3 * (size_t)n, 0.0);
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
          world[3 * (size_t)i] = X, world[3 * (size_t)i + 1] = Y, world[3 * (size_t)i + 2] = Z;
          break;
        }
      } else {
        p.coords2D[0] = (float)(1280.0 * uniform01()), p.coords2D[1] = (float)(960.0 * uniform01());
        q.coords2D[0] = (float)(1280.0 * uniform01()), q.coords2D[1] = (float)(960.0 * uniform01());
      }
      p.coords3D[0] = p.coords3D[1] = p.coords3D[2] = -5.0f;  // stale values: the call owes every record an answer
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

    // ---- one step ----
    SiftData a1, a2;
    upload(a1, f1);
    upload(a2, f2);
    double Rt[12], F[9], sigma[3];
    int numMatches = -1, numFit = -1, numFront = -1, votes[4];
    RegisterPose(a1, a2, &cam, Rt, &numMatches, &numFit, &numFront, 1000, lo, hi, 1.0f, 5, 1.0f, 11, 0, 0, nullptr, F,
                 votes, sigma);
    a1.Synchronize();
    std::printf("RegisterPose: %d inliers, %d fit, %d in front (votes %d %d %d %d), sigma2 / sigma1 = %.4f\n", numMatches,
                numFit, numFront, votes[0], votes[1], votes[2], votes[3], sigma[1] / sigma[0]);
    // the planted pose in the call's direction: R^T and C / |C| = (1, 0, 0)
    double trace = 0.0, ortho = 0.0;
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        trace += Rt[4 * i + j] * R[3 * j + i];  // trace(Rdev * R) with Rdev ~ R^T
        double dot = 0.0;
        for (int k = 0; k < 3; k++) dot += Rt[4 * i + k] * Rt[4 * j + k];
        ortho = std::fmax(ortho, std::fabs(dot - (i == j ? 1.0 : 0.0)));
      }
    const double det = Rt[0] * (Rt[5] * Rt[10] - Rt[6] * Rt[9]) - Rt[1] * (Rt[4] * Rt[10] - Rt[6] * Rt[8]) +
                       Rt[2] * (Rt[4] * Rt[9] - Rt[5] * Rt[8]);
    const double rotErr = std::acos(std::fmin(1.0, std::fmax(-1.0, (trace - 1.0) / 2.0))) * 57.29577951308232;
    const double tn = std::sqrt(Rt[3] * Rt[3] + Rt[7] * Rt[7] + Rt[11] * Rt[11]);
    const double dirErr = std::acos(std::fmin(1.0, std::fmax(-1.0, Rt[3] / tn))) * 57.29577951308232;
    std::printf("rotation off by %.4f degrees, translation direction by %.4f degrees\n", rotErr, dirErr);
    EXPECT(rotErr <= 0.25 && dirErr <= 1.5, "rotation %.4f, direction %.4f degrees", rotErr, dirErr);
    EXPECT(std::fabs(tn - 1.0) <= 1e-12 && ortho <= 1e-12 && std::fabs(det - 1.0) <= 1e-12, "|t| %.17g, R R^T off by %.3g, det %.17g",
           tn, ortho, det);
    int maxVote = 0;
    for (int v : votes) maxVote = v > maxVote ? v : maxVote;
    EXPECT(numFront == maxVote && numFront <= numFit, "%d in front, %d fit", numFront, numFit);
    int lifted = 0, close = 0, liftedAll = 0, halfZero = 0;
    for (int i = 0; i < n; i++) {
      const float *c = a1.h_data[i].coords3D;
      liftedAll += c[2] > 0.0f;
      halfZero += c[2] == 0.0f && (c[0] != 0.0f || c[1] != 0.0f);
      if (!planted[i] || !(c[2] > 0.0f)) continue;
      lifted++;
      const double *w = &world[3 * (size_t)i];
      const double dx = c[0] * base - w[0], dy = c[1] * base - w[1], dz = c[2] * base - w[2];
      close += std::sqrt(dx * dx + dy * dy + dz * dz) <= 0.05 * std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    }
    std::printf("coords3D: %d of %d planted records carry a point, %d of them within 5 %% of the planted one\n", lifted, nIn, close);
    EXPECT(liftedAll == numFront && halfZero == 0, "%d records carry a point, %d in front, %d half written", liftedAll, numFront, halfZero);
    EXPECT(lifted >= (int)std::ceil(0.99 * nIn), "%d of %d planted records carry a point", lifted, nIn);
    EXPECT(close >= (int)std::ceil(0.90 * lifted), "%d of %d points within 5 %%", close, lifted);

    // ---- the pose alone, from the F just returned, on records that carry the match fields ----
    SiftData b1, b2;
    upload(b1, f1);
    upload(b2, f2);
    safeCall(cusift_match(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(b1.d_data), n,
                          reinterpret_cast<const cusift_point *>(b2.d_data), n, 0));
    double Rt2[12];
    int front2 = -1, votes2[4];
    EstimatePose(b1, F, &cam, Rt2, &front2, lo, hi, 1.0f, 0, nullptr, n, votes2);
    b1.Synchronize();
    int same = 0;
    for (int i = 0; i < n; i++) same += std::memcmp(b1.h_data[i].coords3D, a1.h_data[i].coords3D, 3 * sizeof(float)) == 0;
    std::printf("EstimatePose: %d in front\n", front2);
    EXPECT(std::memcmp(Rt, Rt2, sizeof(Rt)) == 0 && front2 == numFront && std::memcmp(votes, votes2, sizeof(votes)) == 0 && same == n,
           "EstimatePose differs from RegisterPose (%d of %d records agree)", same, n);

    // ---- refusal and the degenerate answer, through the C ABI ----
    double Rt3[12];
    int front3 = -7;
    for (double &v : Rt3) v = 9.0;
    const int err = cusift_estimate_pose(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(b1.d_data), n, n, 0, lo, hi, F,
                                         1.0f, nullptr, nullptr, Rt3, &front3, nullptr, nullptr);
    bool untouched = front3 == -7;
    for (double v : Rt3) untouched = untouched && v == 9.0;
    EXPECT(err == CUSIFT_ERR_INVALID && untouched, "a NULL camera gave %d", err);
    const double zeros[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    EstimatePose(b1, zeros, &cam, Rt3, &front3, lo, hi);
    b1.Synchronize();
    const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    int nonzero = 0;
    for (int i = 0; i < n; i++) nonzero += b1.h_data[i].coords3D[0] != 0.0f || b1.h_data[i].coords3D[1] != 0.0f || b1.h_data[i].coords3D[2] != 0.0f;
    EXPECT(std::memcmp(Rt3, ident, sizeof(ident)) == 0 && front3 == 0 && nonzero == 0, "F of zeros: %d in front, %d records carry a point", front3, nonzero);
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
