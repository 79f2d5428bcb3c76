// MatchSiftDataProjected (include/pnp.h) from plain C++ (g++), no HIP headers: VLFeat descriptor dumps in, with a
// synthetic depth and pose.  Every record of set 1 gets its own pixel back-projected at a depth of 1 + (i mod 13) / 4 --
// none where i mod 7 == 3 -- in float arithmetic that tests/test_cpp_projected.py repeats operation by operation; the pose
// and the camera are the literals below, which that file repeats too.  Three cases:
//   * under POSE at RADIUS the five match fields of every record go to <out.bin>, followed by the number of pairs
//     returned, for the Python test to compare with the bytes of its own call;
//   * under a radius that every pair passes, with a depth everywhere, the call must leave MatchSiftData's bytes in data1's
//     records and return the same pairs;
//   * under a pose of twelve zeros, which passes nothing, every record must come back with match == -1 and no pair.
// Usage: projected_dropin <vlfeat_sift1.bin> <vlfeat_sift2.bin> <score threshold> <ambiguity threshold> <out.bin>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cuSIFT.h"
#include "debug.h"
#include "pnp.h"

static const double POSE[12] = {0.9995, -0.015, -0.03, 0.05, 0.0152, 0.9998, 0.02, -0.03, 0.0297, -0.0204, 0.9993, 0.04};
static const float FX = 800.0f, FY = 790.0f, CX = 400.5f, CY = 300.5f, ORIGIN = 1.0f, RADIUS = 40.0f;

// coords3D of every host record, then the records to the device
static void lift(SiftData &d, bool holes) {
  const float px = CX - ORIGIN, py = CY - ORIGIN;
  for (int i = 0; i < d.numPts; i++) {
    SiftPoint &p = d.h_data[i];
    const float z = (holes && i % 7 == 3) ? 0.0f : 1.0f + 0.25f * (float)(i % 13);
    const float u = (p.coords2D[0] - px) / FX, v = (p.coords2D[1] - py) / FY;
    p.coords3D[0] = u * z, p.coords3D[1] = v * z, p.coords3D[2] = z;
  }
  if (d.numPts > 0)
    safeCall(cusift_memcpy_h2d(cusift_dropin::ctx(), d.d_data, d.h_data, sizeof(SiftPoint) * (size_t)d.numPts));
}

static std::vector<int> pairs_of(std::vector<SiftMatch *> &matches, const SiftData &data1, const SiftData &data2, int *bad) {
  std::vector<int> pairs;
  for (SiftMatch *m : matches) {
    pairs.push_back((int)(m->pt1 - data1.h_data));
    pairs.push_back((int)(m->pt2 - data2.h_data));
    if (m->score != m->pt1->score || m->ambiguity != m->pt1->ambiguity) ++*bad;
    delete m;
  }
  return pairs;
}

int main(int argc, char **argv) {
  if (argc < 6) return 2;
  const float score = (float)std::atof(argv[3]), amb = (float)std::atof(argv[4]);
  InitCuda(0);
  int failures = 0;
  {
    SiftData data1, data2;
    if (ReadVLFeatSiftData(data1, argv[1]) < 0 || ReadVLFeatSiftData(data2, argv[2]) < 0) return 2;
    const int n1 = data1.numPts;
    cusift_camera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.fx = FX, cam.fy = FY, cam.cx = CX, cam.cy = CY, cam.origin = ORIGIN;

    // the case the Python test repeats
    lift(data1, true);
    std::vector<SiftMatch *> found = MatchSiftDataProjected(data1, data2, POSE, &cam, RADIUS, MatchSiftDistanceL2, score, amb);
    int matched = 0, holes = 0;
    for (int i = 0; i < n1; i++) {
      matched += data1.h_data[i].match >= 0;
      holes += i % 7 == 3 && (data1.h_data[i].match != -1 || data1.h_data[i].score != 999.0f);
    }
    const int n_pairs = (int)found.size();
    std::printf("projected: %d of %d records matched, %d pairs\n", matched, n1, n_pairs);
    if (matched == 0 || n_pairs == 0 || n_pairs > matched || holes != 0) ++failures;
    pairs_of(found, data1, data2, &failures);
    std::FILE *f = std::fopen(argv[5], "wb");
    if (!f) return 2;
    for (int i = 0; i < n1; i++) std::fwrite(&data1.h_data[i].score, sizeof(float), 5, f);
    std::fwrite(&n_pairs, sizeof(int), 1, f);
    std::fclose(f);

    // a huge radius and a depth everywhere: MatchSiftData's records and pairs
    lift(data1, false);
    std::vector<SiftMatch *> plain = MatchSiftData(data1, data2, MatchSiftDistanceL2, score, amb);
    const std::vector<int> plain_pairs = pairs_of(plain, data1, data2, &failures);
    const std::vector<SiftPoint> rows(data1.h_data, data1.h_data + n1);
    std::printf("plain: %zu pairs of %d records\n", plain_pairs.size() / 2, n1);
    if (plain_pairs.empty()) ++failures;
    std::memset((void *)&data1.h_data[0].score, 0xCD, 5 * sizeof(float));  // the call must write it again
    std::vector<SiftMatch *> wide = MatchSiftDataProjected(data1, data2, POSE, &cam, 1e6f, MatchSiftDistanceL2, score, amb);
    if (std::memcmp(rows.data(), data1.h_data, sizeof(SiftPoint) * (size_t)n1) != 0) {
      std::printf("radius 1e6: data1's records differ from MatchSiftData's\n");
      ++failures;
    }
    const std::vector<int> wide_pairs = pairs_of(wide, data1, data2, &failures);
    if (wide_pairs != plain_pairs) {
      std::printf("radius 1e6: %zu pairs, MatchSiftData returned %zu\n", wide_pairs.size() / 2, plain_pairs.size() / 2);
      ++failures;
    }

    // twelve zeros pass nothing
    const double zero[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<SiftMatch *> none = MatchSiftDataProjected(data1, data2, zero, &cam, 5.0f, MatchSiftDistanceL2, score, amb);
    int unmatched = 0;
    for (int i = 0; i < n1; i++) unmatched += data1.h_data[i].match == -1 && data1.h_data[i].score == 999.0f;
    std::printf("zero pose: %d of %d records unmatched, %zu pairs\n", unmatched, n1, none.size());
    if (unmatched != n1 || !none.empty()) ++failures;
    for (SiftMatch *m : none) delete m;
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
