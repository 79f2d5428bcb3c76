// RegisterPnP and EstimatePnP of include/pnp.h.
//
// Without arguments: a planted scene of its own -- 3-D points in front of a 640 x 480 camera (fx = 520, fy = 470, a
// 1-based principal point) that is turned 0.1 rad about y and moved by (0.5, 0.05, 0.1); every record of frame 1 carries
// its point in coords3D and its partner's descriptor, so the matcher pairs them with a dot product of 1; 0.3 px of noise,
// 40 % gross outliers, every tenth planted record without depth.  Checked:
//   * RegisterPnP: R within 0.25 degrees of the planted rotation, t within 3 % of the planted translation, R orthonormal
//     with determinant +1, at least 95 % of the planted records that carry a depth fit, coords3D untouched;
//   * EstimatePnP on matched records gives the same Rt and counts, byte for byte;
//   * cusift_estimate_pnp refuses a NULL camera and writes nothing; records without depth give [I | 0].
// With arguments `frame1.bin frame2.bin fx fy cx cy origin loops seed lo hi thresh refineThresh out.bin`: RegisterPnP
// (dot-product distance, rule 0) over the two files of raw 588-byte records; out.bin receives Rt[12], the winner's
// [R | t][12] (doubles), numCandidates, numMatches, numFit (ints) and match_error of every record of frame 1 (floats), for
// tests/test_pnp_dropin.py to compare with the Python call's bytes.
// Plain C++ (g++), no HIP headers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cuSIFT.h"
#include "pnp.h"

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

static void upload(SiftData &d, const std::vector<SiftPoint> &src) {
  const int n = (int)src.size();
  InitSiftData(d, n > 0 ? n : 1, true, true);
  if (n > 0) std::memcpy(d.h_data, src.data(), sizeof(SiftPoint) * n);
  d.numPts = n;
  if (n > 0) safeCall(cusift_memcpy_h2d(cusift_dropin::ctx(), d.d_data, d.h_data, sizeof(SiftPoint) * n));
}

static bool read_records(const char *path, std::vector<SiftPoint> &out) {
  std::FILE *f = std::fopen(path, "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  out.resize((size_t)bytes / sizeof(SiftPoint));
  const size_t got = out.empty() ? 0 : std::fread(out.data(), sizeof(SiftPoint), out.size(), f);
  std::fclose(f);
  return bytes % (long)sizeof(SiftPoint) == 0 && got == out.size();
}

static int from_files(char **argv) {
  std::vector<SiftPoint> f1, f2;
  if (!read_records(argv[1], f1) || !read_records(argv[2], f2)) {
    std::printf("FAILED: cannot read the record files\n");
    return 1;
  }
  cusift_camera cam;
  std::memset(&cam, 0, sizeof(cam));
  cam.fx = (float)std::atof(argv[3]), cam.fy = (float)std::atof(argv[4]), cam.cx = (float)std::atof(argv[5]);
  cam.cy = (float)std::atof(argv[6]), cam.origin = (float)std::atof(argv[7]);
  const int loops = std::atoi(argv[8]);
  const uint64_t seed = std::strtoull(argv[9], nullptr, 0);
  const float lo = (float)std::atof(argv[10]), hi = (float)std::atof(argv[11]);
  const float thresh = (float)std::atof(argv[12]), refineThresh = (float)std::atof(argv[13]);
  SiftData a1, a2;
  upload(a1, f1);
  upload(a2, f2);
  double Rt[12], winner[12];
  int counts[3] = {-1, -1, -1};
  RegisterPnP(a1, a2, &cam, Rt, &counts[1], &counts[2], loops, lo, hi, thresh, 5, refineThresh, seed, 0, 0, winner, &counts[0]);
  a1.Synchronize();
  std::printf("RegisterPnP: %d candidates, %d inliers, %d fit\n", counts[0], counts[1], counts[2]);
  std::FILE *f = std::fopen(argv[14], "wb");
  if (!f) {
    std::printf("FAILED: cannot write %s\n", argv[14]);
    return 1;
  }
  std::fwrite(Rt, sizeof(double), 12, f);
  std::fwrite(winner, sizeof(double), 12, f);
  std::fwrite(counts, sizeof(int), 3, f);
  for (size_t i = 0; i < f1.size(); i++) std::fwrite(&a1.h_data[i].match_error, sizeof(float), 1, f);
  std::fclose(f);
  cusift_dropin::shutdown();
  std::printf("PASSED\n");
  return 0;
}

int main(int argc, char **argv) {
  InitCuda(0);
  if (argc == 15) return from_files(argv);
  {
    const int n = 1000;
    const float lo = 0.85f, hi = 0.95f;
    const double fx = 520.0, fy = 470.0, px = 320.0, py = 240.0, ang = 0.1;
    const double C[3] = {0.5, 0.05, 0.1};  // the second camera's centre in frame 1
    const double ca = std::cos(ang), sa = std::sin(ang);
    // X2 = R X1 + t with R a turn about y and t = -R C; the call returns X1 = R^T X2 + C
    const double R[9] = {ca, 0, sa, 0, 1, 0, -sa, 0, ca};
    const double t[3] = {-(R[0] * C[0] + R[2] * C[2]), -C[1], -(R[6] * C[0] + R[8] * C[2])};
    cusift_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.fx = (float)fx, cam.fy = (float)fy, cam.cx = (float)(px + 1.0), cam.cy = (float)(py + 1.0), cam.origin = 1.0f;
    std::vector<SiftPoint> f1((size_t)n), f2((size_t)n);
    std::memset(f1.data(), 0, sizeof(SiftPoint) * n);
    std::memset(f2.data(), 0, sizeof(SiftPoint) * n);
    std::vector<char> planted((size_t)n);
    int nDepth = 0;
    for (int i = 0; i < n; i++) {
      const int j = (i * 7 + 3) % n;  // the partner's slot in frame 2 (7 and 1000 are coprime)
      SiftPoint &p = f1[i], &q = f2[j];
      planted[i] = (i % 5) != 1 && (i % 5) != 3;  // 60 % inliers, interleaved
      for (;;) {  // a point in front of the first camera; a planted one is seen by the second as well
        const double Z = 2.0 + 4.0 * uniform01(), X = (640.0 * uniform01() - px) / fx * Z, Y = (480.0 * uniform01() - py) / fy * Z;
        const double X2 = R[0] * X + R[2] * Z + t[0], Y2 = Y + t[1], Z2 = R[6] * X + R[8] * Z + t[2];
        const double u2 = fx * X2 / Z2 + px, v2 = fy * Y2 / Z2 + py;
        if (planted[i] && (Z2 <= 0.1 || u2 < 0 || u2 >= 640 || v2 < 0 || v2 >= 480)) continue;
        p.coords2D[0] = (float)(fx * X / Z + px), p.coords2D[1] = (float)(fy * Y / Z + py);
        p.coords3D[0] = (float)X, p.coords3D[1] = (float)Y, p.coords3D[2] = (float)Z;
        if (planted[i])
          q.coords2D[0] = (float)(u2 + 0.3 * gauss()), q.coords2D[1] = (float)(v2 + 0.3 * gauss());
        else
          q.coords2D[0] = (float)(640.0 * uniform01()), q.coords2D[1] = (float)(480.0 * uniform01());
        break;
      }
      if (planted[i] && i % 10 == 0) p.coords3D[0] = p.coords3D[1] = p.coords3D[2] = 0.0f;  // no depth: no candidate
      nDepth += planted[i] && p.coords3D[2] != 0.0f;
      double norm = 0.0;
      for (int d = 0; d < 128; d++) {
        p.data[d] = (float)uniform01();
        norm += (double)p.data[d] * p.data[d];
      }
      for (int d = 0; d < 128; d++) q.data[d] = p.data[d] = (float)(p.data[d] / std::sqrt(norm));
    }

    // ---- one step ----
    SiftData a1, a2;
    upload(a1, f1);
    upload(a2, f2);
    double Rt[12], winner[12];
    int numCandidates = -1, numMatches = -1, numFit = -1;
    RegisterPnP(a1, a2, &cam, Rt, &numMatches, &numFit, 2000, lo, hi, 3.0f, 5, 2.0f, 11, 0, 0, winner, &numCandidates);
    a1.Synchronize();
    std::printf("RegisterPnP: %d candidates, %d inliers, %d fit of %d planted records with depth\n", numCandidates, numMatches,
                numFit, nDepth);
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
    const double dx = Rt[3] - C[0], dy = Rt[7] - C[1], dz = Rt[11] - C[2];
    const double tErr = std::sqrt(dx * dx + dy * dy + dz * dz) / std::sqrt(C[0] * C[0] + C[1] * C[1] + C[2] * C[2]);
    std::printf("rotation off by %.4f degrees, translation by %.4f of its length\n", rotErr, tErr);
    EXPECT(rotErr <= 0.25 && tErr <= 0.03, "rotation %.4f degrees, translation %.4f", rotErr, tErr);
    EXPECT(ortho <= 1e-12 && std::fabs(det - 1.0) <= 1e-12, "R R^T off by %.3g, det %.17g", ortho, det);
    EXPECT(numCandidates == n - (600 - nDepth) && numFit >= (int)std::ceil(0.95 * nDepth) && numFit <= numCandidates,
           "%d candidates, %d fit, %d planted with depth", numCandidates, numFit, nDepth);
    int same3D = 0, finiteErr = 0;
    for (int i = 0; i < n; i++) {
      same3D += std::memcmp(a1.h_data[i].coords3D, f1[i].coords3D, 3 * sizeof(float)) == 0;
      finiteErr += std::isfinite(a1.h_data[i].match_error) ? 1 : 0;
    }
    EXPECT(same3D == n && finiteErr >= numCandidates, "%d of %d records keep coords3D, %d carry an error", same3D, n, finiteErr);

    // ---- the estimate alone, on records that carry the match fields ----
    SiftData b1, b2;
    upload(b1, f1);
    upload(b2, f2);
    safeCall(cusift_match(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(b1.d_data), n,
                          reinterpret_cast<const cusift_point *>(b2.d_data), n, 0));
    double Rt2[12], winner2[12];
    int cand2 = -1, matches2 = -1, fit2 = -1;
    EstimatePnP(b1, &cam, Rt2, &matches2, &fit2, 2000, lo, hi, 3.0f, 5, 2.0f, 11, 0, n, winner2, &cand2);
    b1.Synchronize();
    int same = 0;
    for (int i = 0; i < n; i++) same += std::memcmp(&b1.h_data[i].match_error, &a1.h_data[i].match_error, sizeof(float)) == 0;
    std::printf("EstimatePnP: %d candidates, %d inliers, %d fit\n", cand2, matches2, fit2);
    EXPECT(std::memcmp(Rt, Rt2, sizeof(Rt)) == 0 && std::memcmp(winner, winner2, sizeof(winner)) == 0 && cand2 == numCandidates &&
               matches2 == numMatches && fit2 == numFit && same == n,
           "EstimatePnP differs from RegisterPnP (%d of %d records agree)", same, n);

    // ---- refusal and the degenerate answer, through the C ABI ----
    double Rt3[12], winner3[12];
    int ints[3] = {-7, -7, -7};
    for (double &v : Rt3) v = 9.0;
    for (double &v : winner3) v = 9.0;
    const int err = cusift_estimate_pnp(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(b1.d_data), n, n, 0, lo, hi,
                                        nullptr, 100, 3.0f, 5, 2.0f, 1, Rt3, winner3, &ints[0], &ints[1], &ints[2], nullptr,
                                        nullptr, nullptr, nullptr, nullptr);
    bool untouched = ints[0] == -7 && ints[1] == -7 && ints[2] == -7;
    for (double v : Rt3) untouched = untouched && v == 9.0;
    EXPECT(err == CUSIFT_ERR_INVALID && untouched, "a NULL camera gave %d", err);
    std::vector<SiftPoint> flat(f1);
    for (SiftPoint &p : flat) p.coords3D[0] = p.coords3D[1] = p.coords3D[2] = 0.0f;
    SiftData c1;
    upload(c1, flat);
    safeCall(cusift_match(cusift_dropin::ctx(), reinterpret_cast<cusift_point *>(c1.d_data), n,
                          reinterpret_cast<const cusift_point *>(b2.d_data), n, 0));
    EstimatePnP(c1, &cam, Rt3, &ints[1], &ints[2], 100, lo, hi, 3.0f, 5, 2.0f, 1, 0, n, winner3, &ints[0]);
    const double ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    EXPECT(std::memcmp(Rt3, ident, sizeof(ident)) == 0 && std::memcmp(winner3, ident, sizeof(ident)) == 0 && ints[0] == 0 &&
               ints[1] == 0 && ints[2] == 0,
           "no depth anywhere: %d candidates, %d inliers, %d fit", ints[0], ints[1], ints[2]);
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
