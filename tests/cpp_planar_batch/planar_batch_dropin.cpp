// RegisterPlanarSequence of include/homography.h (cusift_register_planar_batch) against RegisterPlanar per pair.
//
// Three frames: frame 0 with random points, frames 1 and 2 its images under two planted homographies with gross
// outliers; record i of frame 0 has the descriptor of its partner in both, so the matcher pairs them with a dot product
// of 1 and no two best scores tie.  The pair list repeats a first member, reverses a pair and holds a self pair.
// Frame 3 is a default-constructed SiftData, no records and no buffers: the pairs (0, 3), (3, 0) and (3, 3) give what
// RegisterPlanar gives for them -- the identity, no inliers, flags for frame a's records and no match_error row.
// Checked, per pair k: homography, winning hypothesis, numMatches, numFit, match_error of every record and the inlier
// flags have the bits RegisterPlanar gives on fresh copies of the two frames with seed + k; the frames handed to
// RegisterPlanarSequence keep every byte; the refined homography of the planted pairs lies within 0.5 px (corners) of
// the planted one.
// Plain C++ (g++), no HIP headers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
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

static double corner_distance(const float *a, const double *b) {
  double worst = 0.0;
  for (const auto &c : kCorners) {
    const double d0 = (double)a[6] * c[0] + (double)a[7] * c[1] + 1.0, d1 = b[6] * c[0] + b[7] * c[1] + 1.0;
    const double ex = ((double)a[0] * c[0] + (double)a[1] * c[1] + (double)a[2]) / d0 - (b[0] * c[0] + b[1] * c[1] + b[2]) / d1;
    const double ey = ((double)a[3] * c[0] + (double)a[4] * c[1] + (double)a[5]) / d0 - (b[3] * c[0] + b[4] * c[1] + b[5]) / d1;
    worst = std::fmax(worst, std::sqrt(ex * ex + ey * ey));
  }
  return worst;
}

int main() {
  InitCuda(0);
  {
    const double H[2][9] = {{0.92, -0.11, 37.0, 0.08, 1.05, -21.0, 2.1e-5, -3.4e-5, 1.0},
                            {1.04, 0.06, -18.0, -0.05, 0.97, 26.0, -1.3e-5, 2.2e-5, 1.0}};
    const int n0 = 1000, nOther[2] = {1000, 900};  // frame 2 is shorter: the counts differ inside one call
    const float lo = 0.85f, hi = 0.95f;
    std::vector<std::vector<SiftPoint> > f(3);
    f[0].resize(n0);
    std::memset(f[0].data(), 0, sizeof(SiftPoint) * n0);
    for (int i = 0; i < n0; i++) {
      SiftPoint &p = f[0][i];
      p.coords2D[0] = (float)(1280.0 * uniform01()), p.coords2D[1] = (float)(960.0 * uniform01());
      double norm = 0.0;
      for (int d = 0; d < 128; d++) {
        p.data[d] = (float)uniform01();
        norm += (double)p.data[d] * p.data[d];
      }
      for (int d = 0; d < 128; d++) p.data[d] = (float)(p.data[d] / std::sqrt(norm));
    }
    for (int t = 0; t < 2; t++) {
      const int n = nOther[t];
      f[t + 1].resize(n);
      std::memset(f[t + 1].data(), 0, sizeof(SiftPoint) * n);
      for (int i = 0; i < n; i++) {
        const int j = (i * 7 + 3) % n;  // the partner's slot (7 is coprime to 1000 and to 900)
        const SiftPoint &p = f[0][i];
        SiftPoint &q = f[t + 1][j];
        const double x = p.coords2D[0], y = p.coords2D[1];
        const bool inlier = (i % 5) != 1 && (i % 5) != 3;  // 60 % inliers, interleaved
        if (inlier) {
          const double den = H[t][6] * x + H[t][7] * y + 1.0;
          q.coords2D[0] = (float)((H[t][0] * x + H[t][1] * y + H[t][2]) / den + 0.6 * (uniform01() - 0.5));
          q.coords2D[1] = (float)((H[t][3] * x + H[t][4] * y + H[t][5]) / den + 0.6 * (uniform01() - 0.5));
        } else {
          q.coords2D[0] = (float)(1280.0 * uniform01()), q.coords2D[1] = (float)(960.0 * uniform01());
        }
        std::memcpy(q.data, p.data, sizeof(q.data));
      }
    }
    auto upload = [&](SiftData &d, const std::vector<SiftPoint> &src) {
      const int n = (int)src.size();
      if (n == 0) return;  // as constructed: d_data == nullptr, numPts == 0
      InitSiftData(d, n, true, true);
      std::memcpy(d.h_data, src.data(), sizeof(SiftPoint) * n);
      d.numPts = n;
      safeCall(cusift_memcpy_h2d(cusift_dropin::ctx(), d.d_data, d.h_data, sizeof(SiftPoint) * n));
    };

    const uint64_t seed = 11;
    const int loops = 1000;
    std::vector<std::pair<int, int> > pairs = {{0, 1}, {0, 2}, {1, 0}, {0, 1}, {2, 2}, {0, 3}, {3, 0}, {3, 3}};
    f.resize(4);  // frame 3: no records
    std::vector<SiftData> frames(4);
    std::vector<SiftData *> ptrs;
    for (int i = 0; i < 4; i++) {
      upload(frames[i], f[i]);
      ptrs.push_back(&frames[i]);
    }
    std::vector<float> hom, win;
    std::vector<int> matches, fit;
    std::vector<std::vector<float> > errors;
    std::vector<std::vector<char> > flags;
    RegisterPlanarSequence(ptrs, pairs, hom, &matches, &fit, loops, lo, hi, 5.0f, 5, 3.0f, seed, 0, 0, &win, &errors, &flags);
    EXPECT(hom.size() == 9 * pairs.size() && win.size() == hom.size() && matches.size() == pairs.size() &&
               fit.size() == pairs.size() && errors.size() == pairs.size() && flags.size() == pairs.size(),
           "output sizes");
    for (int i = 0; i < 3; i++) {  // the frames keep every byte
      frames[i].Synchronize();
      EXPECT(std::memcmp(frames[i].h_data, f[i].data(), sizeof(SiftPoint) * f[i].size()) == 0, "frame %d was written", i);
    }
    for (size_t k = 0; k < pairs.size() && !failures; k++) {
      const int a = pairs[k].first, b = pairs[k].second, na = (int)f[a].size();
      SiftData d1, d2;
      upload(d1, f[a]);
      upload(d2, f[b]);
      float H1[9], R1[9];
      int m1 = -1, fit1 = -1;
      RegisterPlanar(d1, d2, H1, &m1, &fit1, loops, lo, hi, 5.0f, 5, 3.0f, seed + k, 0, 0, R1);
      d1.Synchronize();
      std::printf("pair %zu (%d, %d): %d inliers, %d fit; pair call %d, %d\n", k, a, b, matches[k], fit[k], m1, fit1);
      EXPECT(std::memcmp(H1, &hom[9 * k], sizeof(H1)) == 0, "pair %zu: homography differs", k);
      EXPECT(std::memcmp(R1, &win[9 * k], sizeof(R1)) == 0, "pair %zu: winner differs", k);
      EXPECT(m1 == matches[k] && fit1 == fit[k], "pair %zu: counts %d %d, pair call %d %d", k, matches[k], fit[k], m1, fit1);
      EXPECT((int)flags[k].size() == na, "pair %zu: %zu flags for %d records", k, flags[k].size(), na);
      if (f[a].empty() || f[b].empty()) {  // nothing to match: no fit, so no match_error row
        const float ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        EXPECT(std::memcmp(ident, &hom[9 * k], sizeof(ident)) == 0 && matches[k] == 0 && fit[k] == 0 && errors[k].empty() &&
                   flags[k] == std::vector<char>((size_t)na, 0),
               "pair %zu: %d inliers, %d fit, %zu errors with an empty frame", k, matches[k], fit[k], errors[k].size());
        continue;
      }
      EXPECT((int)errors[k].size() == na, "pair %zu: %zu errors for %d records", k, errors[k].size(), na);
      int same = 0, marked = 0;
      for (int i = 0; i < na && (int)errors[k].size() == na; i++)
        same += std::memcmp(&d1.h_data[i].match_error, &errors[k][i], sizeof(float)) == 0;
      for (size_t i = 0; i < flags[k].size(); i++) marked += flags[k][i] != 0;
      EXPECT(same == na, "pair %zu: match_error of %d records differs", k, na - same);
      EXPECT(marked == matches[k], "pair %zu: %d flags, %d inliers", k, marked, matches[k]);
      if (k < 2) {
        const double d = corner_distance(&hom[9 * k], H[k]);
        std::printf("pair %zu: corners %.3f px from the planted homography\n", k, d);
        EXPECT(d < 0.5, "pair %zu: refined homography %.3f px from the planted one", k, d);
        EXPECT(matches[k] >= (int)(0.9 * 0.6 * nOther[k]), "pair %zu: %d inliers", k, matches[k]);
      }
    }
    // the default pair list is the walk (i, i + 1), byte for byte; an empty sequence is no error
    std::vector<std::pair<int, int> > none, steps = {{0, 1}, {1, 2}, {2, 3}};
    std::vector<float> walk, stepped;
    RegisterPlanarSequence(ptrs, none, walk, NULL, NULL, loops, lo, hi, 5.0f, 5, 3.0f, seed);
    RegisterPlanarSequence(ptrs, steps, stepped, NULL, NULL, loops, lo, hi, 5.0f, 5, 3.0f, seed);
    EXPECT(walk.size() == 27 && std::memcmp(walk.data(), hom.data(), 9 * sizeof(float)) == 0, "default pairs");
    EXPECT(walk.size() == stepped.size() && std::memcmp(walk.data(), stepped.data(), sizeof(float) * walk.size()) == 0,
           "the default pairs differ from the explicit walk");
    std::vector<SiftData *> nobody;
    RegisterPlanarSequence(nobody, none, walk);
    EXPECT(walk.empty(), "an empty sequence gave %zu floats", walk.size());
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
