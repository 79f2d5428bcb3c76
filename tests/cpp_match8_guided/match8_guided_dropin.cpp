// The guided 8-bit matchers through the drop-in headers (include/matching.h, pnp.h), from plain C++ (g++), no HIP headers.
// The PGM fixture is extracted at two thresholds, which gives two record sets of one scene: a keypoint of set 2 lies where
// its partner of set 1 lies, so the identity homography and -- with both sets lifted at one depth -- the identity pose
// are true models.
//   1. MatchSiftData8Guided under the identity at 2 px against the C call cusift_match8_guided on the same tables: the
//      five match fields of every record are the same bytes, the returned pairs are the records that pass MatchSiftData's
//      filter, and every returned partner lies within the radius.  Fewer pairs than MatchSiftData8 gives, not none.
//   2. At a radius of 1e6 the fields are MatchSiftData8's, byte for byte.
//   3. The same two checks for MatchSiftData8Projected against cusift_match8_projected.
//
//   match8_guided_dropin tests/golden/gray1.pgm
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cuImage.h"
#include "cuSIFT.h"
#include "matching.h"
#include "pnp.h"
#include "rgbd.h"

static bool read_pgm(const char *path, std::vector<float> &img, int &w, int &h) {
  FILE *fp = std::fopen(path, "rb");
  if (!fp) return false;
  int maxv = 0;
  if (std::fscanf(fp, "P5 %d %d %d", &w, &h, &maxv) != 3 || maxv != 255) return false;
  std::fgetc(fp);
  std::vector<unsigned char> raw((size_t)w * h);
  if (std::fread(raw.data(), 1, raw.size(), fp) != raw.size()) return false;
  std::fclose(fp);
  img.assign(raw.begin(), raw.end());
  return true;
}

// the five match fields of every record: score, ambiguity, match, match_xpos, match_ypos
struct Fields {
  float v[5];
};
static std::vector<Fields> fields_of(const SiftData &a) {
  std::vector<Fields> out((size_t)a.numPts);
  for (int i = 0; i < a.numPts; i++) std::memcpy(out[i].v, &a.h_data[i].score, sizeof(Fields));
  return out;
}
static int fields_differ(const std::vector<Fields> &a, const std::vector<Fields> &b) {
  if (a.size() != b.size()) return 1;
  int bad = 0;
  for (size_t i = 0; i < a.size(); i++) bad += std::memcmp(a[i].v, b[i].v, sizeof(Fields)) != 0;
  return bad;
}
static void read_fields(SiftData &a) {
  safeCall(cusift_memcpy2d_d2h(cusift_dropin::ctx(), &a.h_data[0].score, sizeof(SiftPoint), &a.d_data[0].score,
                               sizeof(SiftPoint), 5 * sizeof(float), (size_t)a.numPts));
}

// What a wrapper's result must be, given the fields the C call left in data1: the records that pass MatchSiftData's
// filter at (999, 0.8), in order, each within `radius` of where the model puts its record: the record's own position under
// the identity homography, the pixel of its coords3D under the identity pose and `camera` (not NULL).
static int check_pairs(const char *what, const std::vector<SiftMatch *> &got, SiftData &data1, SiftData &data2, float radius,
                       size_t unguided, const cusift_camera *camera = nullptr) {
  std::vector<int> want;
  for (int i = 0; i < data1.numPts; i++) {
    const SiftPoint &p = data1.h_data[i];
    if (p.score < 999.0f * 999.0f && p.ambiguity < 0.8f * 0.8f && p.match >= 0 && p.match < data2.numPts) want.push_back(i);
  }
  int bad = got.size() != want.size();
  double worst = 0.0;
  for (size_t k = 0; k < got.size() && !bad; k++) {
    const int i = (int)(got[k]->pt1 - data1.h_data);
    bad += i != want[k] || got[k]->pt2 != &data2.h_data[data1.h_data[i].match];
    const float *a = got[k]->pt1->coords2D, *X = got[k]->pt1->coords3D, *b = got[k]->pt2->coords2D;
    const double px = camera ? (double)camera->fx * X[0] / X[2] + camera->cx - camera->origin : a[0];
    const double py = camera ? (double)camera->fy * X[1] / X[2] + camera->cy - camera->origin : a[1];
    worst = std::fmax(worst, std::hypot(b[0] - px, b[1] - py));
  }
  std::printf("%s: %zu pairs (%zu expected, %zu unguided), the farthest partner %.3f px away\n", what, got.size(), want.size(),
              unguided, worst);
  return bad + (got.empty() || got.size() >= unguided || worst >= radius + 1e-3);
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: %s gray1.pgm\n", argv[0]);
    return 2;
  }
  std::vector<float> im;
  int w = 0, h = 0;
  if (!read_pgm(argv[1], im, w, h)) return 2;
  if (!deviceInit(0)) return 2;
  int failures = 0;
  {
    cuImage img(w, h, im.data());
    SiftData data1(8192, true, true), data2(8192, true, true);
    ExtractSift(data1, img, 4, 0.0, 1.0f);
    ExtractSift(data2, img, 4, 0.0, 2.0f);
    if (data1.numPts <= data2.numPts || data2.numPts < 100) ++failures;
    // one depth for every pixel: under [I | 0] and the same camera a record projects onto its own pixel
    const cusift_camera camera = {500.0f, 500.0f, 0.5f * w, 0.5f * h, 0.0f, 1000.0f, 0};
    const std::vector<unsigned short> depth((size_t)w * h, 2000);
    LiftSiftData(data1, depth.data(), w, h, camera);
    LiftSiftData(data2, depth.data(), w, h, camera);
    SiftDescriptors8 desc1, desc2;
    QuantizeSiftData(data1, desc1);
    QuantizeSiftData(data2, desc2);
    cusift_ctx *ctx = cusift_dropin::ctx();
    cusift_point *d1 = reinterpret_cast<cusift_point *>(data1.d_data);
    const cusift_point *d2 = reinterpret_cast<const cusift_point *>(data2.d_data);
    const double ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double pose[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const float radius = 2.0f;

    std::vector<SiftMatch *> plain = MatchSiftData8(data1, desc1, data2, desc2, MatchSiftDistanceL2, 999.0f, 0.8f);
    const std::vector<Fields> plain_fields = fields_of(data1);
    const size_t unguided = plain.size();
    for (SiftMatch *m : plain) delete m;

    // 1. + 2. under H
    safeCall(cusift_match8_guided(ctx, d1, data1.numPts, desc1.d_data, desc1.d_sums, d2, data2.numPts, desc2.d_data,
                                  desc2.d_sums, 1, CUSIFT_GUIDE_HOMOGRAPHY, ident, radius));
    read_fields(data1);
    const std::vector<Fields> c_fields = fields_of(data1);
    std::vector<SiftMatch *> got = MatchSiftData8Guided(data1, desc1, data2, desc2, CUSIFT_GUIDE_HOMOGRAPHY, ident, radius,
                                                        MatchSiftDistanceL2, 999.0f, 0.8f);
    failures += fields_differ(c_fields, fields_of(data1));
    failures += check_pairs("guided", got, data1, data2, radius, unguided);
    for (SiftMatch *m : got) delete m;
    got = MatchSiftData8Guided(data1, desc1, data2, desc2, CUSIFT_GUIDE_HOMOGRAPHY, ident, 1e6f, MatchSiftDistanceL2, 999.0f,
                               0.8f);
    failures += fields_differ(plain_fields, fields_of(data1)) + (got.size() != unguided);
    for (SiftMatch *m : got) delete m;

    // 3. under the pose
    safeCall(cusift_match8_projected(ctx, d1, data1.numPts, desc1.d_data, desc1.d_sums, d2, data2.numPts, desc2.d_data,
                                     desc2.d_sums, 1, pose, &camera, radius));
    read_fields(data1);
    const std::vector<Fields> p_fields = fields_of(data1);
    got = MatchSiftData8Projected(data1, desc1, data2, desc2, pose, &camera, radius, MatchSiftDistanceL2, 999.0f, 0.8f);
    failures += fields_differ(p_fields, fields_of(data1));
    failures += check_pairs("projected", got, data1, data2, radius, unguided, &camera);
    for (SiftMatch *m : got) delete m;
    got = MatchSiftData8Projected(data1, desc1, data2, desc2, pose, &camera, 1e6f, MatchSiftDistanceL2, 999.0f, 0.8f);
    failures += fields_differ(plain_fields, fields_of(data1)) + (got.size() != unguided);
    for (SiftMatch *m : got) delete m;
  }
  cusift_dropin::shutdown();
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
