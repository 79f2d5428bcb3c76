// RegisterEpipolarSequence (include/epipolar.h), RegisterPoseSequence (include/pose.h) and RegisterPnPSequence
// (include/pnp.h) against the pair calls.
//
// A planted scene of its own: 3-D points in front of a 640 x 480 camera (fx = 520, fy = 470, a 1-based principal point)
// seen from three places -- the second view turned 0.1 rad about y and moved by (0.5, 0.05, 0.1), the third twice that.
// Every frame holds one record per point, in an order of its own, with the point's pixel (0.3 px of noise), the point in
// that camera's coordinates in coords3D and the point's descriptor, so the matcher pairs them with a dot product of 1;
// 30 % of a frame's records are gross outliers.  The frames have 900, 800 and 700 records.
// A fourth frame is a default-constructed SiftData: no records, no buffers.
// Checked, for the pairs (0, 1), (1, 2), (2, 0) and (0, 1) again, and for (0, 3), (3, 1) and (3, 3) with the empty frame
// -- nine zeros, [I | 0], zero counts, no match_error row, flags and points for frame a's records:
//   * every pair of each sequence call equals RegisterEpipolar / RegisterPose / RegisterPnP on fresh copies of the two
//     frames with seed + k, byte for byte: the models, the counts, match_error and -- for the pose -- coords3D;
//   * the sequence calls leave the frames' device records as they were;
//   * the PnP poses lie within 0.25 degrees and 3 % of the planted ones;
//   * an empty pair list is the walk (i, i + 1), byte for byte, and a sequence without frames gives empty outputs.
// Plain C++ (g++), no HIP headers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "cuSIFT.h"
#include "epipolar.h"
#include "pnp.h"
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

static void upload(SiftData &d, const std::vector<SiftPoint> &src) {
  const int n = (int)src.size();
  InitSiftData(d, n > 0 ? n : 1, true, true);
  if (n > 0) std::memcpy(d.h_data, src.data(), sizeof(SiftPoint) * n);
  d.numPts = n;
  if (n > 0) safeCall(cusift_memcpy_h2d(cusift_dropin::ctx(), d.d_data, d.h_data, sizeof(SiftPoint) * n));
}

static const double kFx = 520.0, kFy = 470.0, kPx = 320.0, kPy = 240.0;

// view v: X_v = R_v X_0 + t_v with R_v a turn of v * 0.1 rad about y and t_v = -R_v C_v, C_v = v * (0.5, 0.05, 0.1)
static void to_view(int v, const double X0[3], double Xv[3]) {
  const double ang = 0.1 * v, ca = std::cos(ang), sa = std::sin(ang);
  const double d[3] = {X0[0] - 0.5 * v, X0[1] - 0.05 * v, X0[2] - 0.1 * v};
  Xv[0] = ca * d[0] + sa * d[2], Xv[1] = d[1], Xv[2] = -sa * d[0] + ca * d[2];
}

int main() {
  InitCuda(0);
  const int nPoints = 900, counts[4] = {900, 800, 700, 0};
  const float lo = 0.85f, hi = 0.95f;
  cusift_camera cam;
  std::memset(&cam, 0, sizeof(cam));
  cam.fx = (float)kFx, cam.fy = (float)kFy, cam.cx = (float)(kPx + 1.0), cam.cy = (float)(kPy + 1.0), cam.origin = 1.0f;
  // the points, seen by all three views, and their descriptors
  std::vector<double> world(3 * (size_t)nPoints);
  std::vector<float> desc(128 * (size_t)nPoints);
  for (int i = 0; i < nPoints; i++) {
    for (;;) {
      const double Z = 2.5 + 4.0 * uniform01();
      double X0[3] = {(640.0 * uniform01() - kPx) / kFx * Z, (480.0 * uniform01() - kPy) / kFy * Z, Z};
      bool seen = true;
      for (int v = 1; v < 3; v++) {
        double Xv[3];
        to_view(v, X0, Xv);
        const double u = kFx * Xv[0] / Xv[2] + kPx, w = kFy * Xv[1] / Xv[2] + kPy;
        seen = seen && Xv[2] > 0.5 && u >= 0 && u < 640 && w >= 0 && w < 480;
      }
      if (!seen) continue;
      for (int c = 0; c < 3; c++) world[3 * (size_t)i + c] = X0[c];
      break;
    }
    double norm = 0.0;
    float *d = &desc[128 * (size_t)i];
    for (int k = 0; k < 128; k++) d[k] = (float)uniform01(), norm += (double)d[k] * d[k];
    for (int k = 0; k < 128; k++) d[k] = (float)(d[k] / std::sqrt(norm));
  }
  const int stride[3] = {1, 7, 11};  // coprime with 900: every frame has an order of its own
  std::vector<std::vector<SiftPoint> > recs(4);  // recs[3] stays empty
  for (int v = 0; v < 3; v++) {
    recs[v].resize((size_t)counts[v]);
    std::memset(recs[v].data(), 0, sizeof(SiftPoint) * recs[v].size());
    for (int s = 0; s < counts[v]; s++) {
      const int i = (int)(((long)s * stride[v] + 3 * v) % nPoints);
      SiftPoint &p = recs[v][s];
      double Xv[3];
      to_view(v, &world[3 * (size_t)i], Xv);
      const bool outlier = (i + v) % 10 < 3;  // 30 %, other points in every view
      p.coords2D[0] = (float)(outlier ? 640.0 * uniform01() : kFx * Xv[0] / Xv[2] + kPx + 0.3 * gauss());
      p.coords2D[1] = (float)(outlier ? 480.0 * uniform01() : kFy * Xv[1] / Xv[2] + kPy + 0.3 * gauss());
      p.coords3D[0] = (float)Xv[0], p.coords3D[1] = (float)Xv[1], p.coords3D[2] = (float)Xv[2];
      p.match = -1, p.match_error = 7.0f;
      std::memcpy(p.data, &desc[128 * (size_t)i], sizeof(float) * 128);
    }
  }
  SiftData frame[4];  // frame[3] as constructed: d_data == nullptr, numPts == 0
  std::vector<SiftData *> frames;
  for (int v = 0; v < 4; v++) {
    if (v < 3) upload(frame[v], recs[v]);
    frames.push_back(&frame[v]);
  }
  std::vector<std::pair<int, int> > pairs;
  pairs.push_back(std::make_pair(0, 1)), pairs.push_back(std::make_pair(1, 2));
  pairs.push_back(std::make_pair(2, 0)), pairs.push_back(std::make_pair(0, 1));
  pairs.push_back(std::make_pair(0, 3)), pairs.push_back(std::make_pair(3, 1)), pairs.push_back(std::make_pair(3, 3));
  const int nPairs = (int)pairs.size(), loops = 2000;
  const uint64_t seed = 0xFFFFFFFFFFFFFFFEull;  // seed + k wraps

  // ---- the three sequence calls ----
  std::vector<double> F, Fwin, poseRt, poseF, pnpRt, pnpWin;
  std::vector<int> fMatches, fFit, pMatches, pFit, pFront, nMatches, nFit, nCand;
  std::vector<std::vector<float> > fErr, xyz, nErr;
  std::vector<std::vector<char> > fFlags, nFlags;
  RegisterEpipolarSequence(frames, pairs, F, &fMatches, &fFit, loops, lo, hi, 1.0f, 5, 1.0f, seed, 0, 0, &Fwin, &fErr, &fFlags);
  RegisterPoseSequence(frames, pairs, &cam, poseRt, &pMatches, &pFit, &pFront, loops, lo, hi, 1.0f, 5, 1.0f, seed, 0, 0,
                       nullptr, &poseF, &xyz);
  RegisterPnPSequence(frames, pairs, &cam, pnpRt, &nMatches, &nFit, loops, lo, hi, 3.0f, 5, 2.0f, seed, 0, 0, &pnpWin, &nErr,
                      &nFlags, &nCand);
  EXPECT((int)F.size() == 9 * nPairs && (int)poseRt.size() == 12 * nPairs && (int)pnpRt.size() == 12 * nPairs,
         "%zu, %zu, %zu values", F.size(), poseRt.size(), pnpRt.size());
  for (int v = 0; v < 3; v++) {  // the frames are not written
    frame[v].Synchronize();
    EXPECT(std::memcmp(frame[v].h_data, recs[v].data(), sizeof(SiftPoint) * recs[v].size()) == 0,
           "frame %d was written by a sequence call", v);
  }
  if ((int)F.size() == 9 * nPairs && (int)poseRt.size() == 12 * nPairs && (int)pnpRt.size() == 12 * nPairs)
    for (int k = 0; k < nPairs; k++) {
      const int a = pairs[k].first, b = pairs[k].second, na = counts[a];
      const bool empty = counts[a] == 0 || counts[b] == 0;  // nothing to match: no fit
      const double zeros[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
      // ---- RegisterEpipolar ----
      {
        SiftData d1, d2;
        upload(d1, recs[a]), upload(d2, recs[b]);
        double f[9], win[9];
        int matches = -1, fit = -1;
        RegisterEpipolar(d1, d2, f, &matches, &fit, loops, lo, hi, 1.0f, 5, 1.0f, seed + k, 0, 0, win);
        d1.Synchronize();
        int same = 0;
        for (int i = 0; i < na && (int)fErr[k].size() == na; i++)
          same += std::memcmp(&d1.h_data[i].match_error, &fErr[k][i], sizeof(float)) == 0;
        std::printf("pair (%d, %d) F: %d inliers, %d fit\n", a, b, matches, fit);
        EXPECT(std::memcmp(f, &F[9 * (size_t)k], sizeof(f)) == 0 && std::memcmp(win, &Fwin[9 * (size_t)k], sizeof(win)) == 0 &&
                   matches == fMatches[k] && fit == fFit[k] && (int)fFlags[k].size() == na &&
                   (empty ? fErr[k].empty() && std::memcmp(f, zeros, sizeof(f)) == 0 && matches == 0 && fit == 0
                          : same == na && fit >= 250),
               "pair %d: RegisterEpipolarSequence differs from RegisterEpipolar (%d of %d errors agree)", k, same, na);
        FreeSiftData(d1), FreeSiftData(d2);
      }
      // ---- RegisterPose ----
      {
        SiftData d1, d2;
        upload(d1, recs[a]), upload(d2, recs[b]);
        double rt[12], f[9];
        int matches = -1, fit = -1, front = -1;
        RegisterPose(d1, d2, &cam, rt, &matches, &fit, &front, loops, lo, hi, 1.0f, 5, 1.0f, seed + k, 0, 0, nullptr, f);
        d1.Synchronize();
        int same = 0;
        for (int i = 0; i < na && (int)xyz[k].size() == 3 * na; i++)
          same += std::memcmp(d1.h_data[i].coords3D, &xyz[k][3 * (size_t)i], 3 * sizeof(float)) == 0;
        std::printf("pair (%d, %d) pose: %d inliers, %d fit, %d in front\n", a, b, matches, fit, front);
        EXPECT(std::memcmp(rt, &poseRt[12 * (size_t)k], sizeof(rt)) == 0 && std::memcmp(f, &poseF[9 * (size_t)k], sizeof(f)) == 0 &&
                   matches == pMatches[k] && fit == pFit[k] && front == pFront[k] && same == na &&
                   (int)xyz[k].size() == 3 * na &&
                   (empty ? std::memcmp(rt, ident, sizeof(rt)) == 0 && matches == 0 && fit == 0 && front == 0 : front >= 250),
               "pair %d: RegisterPoseSequence differs from RegisterPose (%d of %d points agree)", k, same, na);
        FreeSiftData(d1), FreeSiftData(d2);
      }
      // ---- RegisterPnP ----
      {
        SiftData d1, d2;
        upload(d1, recs[a]), upload(d2, recs[b]);
        double rt[12], win[12];
        int cand = -1, matches = -1, fit = -1;
        RegisterPnP(d1, d2, &cam, rt, &matches, &fit, loops, lo, hi, 3.0f, 5, 2.0f, seed + k, 0, 0, win, &cand);
        d1.Synchronize();
        int same = 0;
        for (int i = 0; i < na && (int)nErr[k].size() == na; i++)
          same += std::memcmp(&d1.h_data[i].match_error, &nErr[k][i], sizeof(float)) == 0;
        std::printf("pair (%d, %d) PnP: %d candidates, %d inliers, %d fit\n", a, b, cand, matches, fit);
        EXPECT(std::memcmp(rt, &pnpRt[12 * (size_t)k], sizeof(rt)) == 0 && std::memcmp(win, &pnpWin[12 * (size_t)k], sizeof(win)) == 0 &&
                   cand == nCand[k] && matches == nMatches[k] && fit == nFit[k] && (int)nFlags[k].size() == na &&
                   (empty ? nErr[k].empty() && std::memcmp(rt, ident, sizeof(rt)) == 0 && cand == 0 && matches == 0 && fit == 0
                          : same == na),
               "pair %d: RegisterPnPSequence differs from RegisterPnP (%d of %d errors agree)", k, same, na);
        // the planted pose: X_a = R X_b + t, from X_v = R_v (X_0 - C_v)
        double worst = 0.0;
        for (int i = 0; i < 20 && !empty; i++) {
          double Xa[3], Xb[3];
          to_view(a, &world[3 * (size_t)i], Xa), to_view(b, &world[3 * (size_t)i], Xb);
          for (int r = 0; r < 3; r++) {
            const double got = rt[4 * r] * Xb[0] + rt[4 * r + 1] * Xb[1] + rt[4 * r + 2] * Xb[2] + rt[4 * r + 3];
            worst = std::fmax(worst, std::fabs(got - Xa[r]));
          }
        }
        // 0.25 degrees at 6.5 units of depth is 0.028 and 3 % of the baseline |C| = 0.51 is 0.015: 0.045 together
        EXPECT(empty || (worst <= 0.045 && fit >= 250), "pair %d: planted points land %.4f off, %d fit", k, worst, fit);
        FreeSiftData(d1), FreeSiftData(d2);
      }
    }
  // the repeated pair draws from another seed: the winners differ, the refined models agree to a fraction of a pixel
  EXPECT(std::memcmp(&Fwin[0], &Fwin[27], 9 * sizeof(double)) != 0, "pairs 0 and 3 drew the same samples");
  // an empty pair list is the walk (i, i + 1); a sequence without frames gives empty outputs and no error
  {
    std::vector<std::pair<int, int> > none, steps;
    for (int i = 0; i + 1 < 4; i++) steps.push_back(std::make_pair(i, i + 1));
    std::vector<SiftData *> nobody;
    std::vector<double> walk[3], stepped[3], nothing[3];
    std::vector<int> walkFit[3], steppedFit[3];
    for (int explicitly = 0; explicitly < 2; explicitly++) {
      std::vector<double> *m = explicitly ? stepped : walk;
      std::vector<int> *n = explicitly ? steppedFit : walkFit;
      const std::vector<std::pair<int, int> > &list = explicitly ? steps : none;
      RegisterEpipolarSequence(frames, list, m[0], NULL, &n[0], loops, lo, hi, 1.0f, 5, 1.0f, seed);
      RegisterPoseSequence(frames, list, &cam, m[1], NULL, &n[1], NULL, loops, lo, hi, 1.0f, 5, 1.0f, seed);
      RegisterPnPSequence(frames, list, &cam, m[2], NULL, &n[2], loops, lo, hi, 3.0f, 5, 2.0f, seed);
    }
    RegisterEpipolarSequence(nobody, none, nothing[0]);
    RegisterPoseSequence(nobody, none, &cam, nothing[1]);
    RegisterPnPSequence(nobody, none, &cam, nothing[2]);
    for (int c = 0; c < 3; c++) {
      EXPECT(walk[c].size() == (c ? 12u : 9u) * steps.size() && walk[c].size() == stepped[c].size() &&
                 std::memcmp(walk[c].data(), stepped[c].data(), sizeof(double) * walk[c].size()) == 0 &&
                 walkFit[c] == steppedFit[c],
             "call %d: the default pairs differ from the explicit walk (%zu, %zu values)", c, walk[c].size(), stepped[c].size());
      EXPECT(walkFit[c].size() == 3 && walkFit[c][0] >= 250 && walkFit[c][2] == 0, "call %d: the walk's fits", c);
      EXPECT(nothing[c].empty(), "call %d: an empty sequence gave %zu values", c, nothing[c].size());
    }
  }
  for (int v = 0; v < 3; v++) FreeSiftData(frame[v]);
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
