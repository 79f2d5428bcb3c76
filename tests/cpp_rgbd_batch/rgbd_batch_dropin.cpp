// The reference walks its sequences frame by frame (main.cpp: compareMatchingWithMATLAB, i -> i + 1).  This program
// registers a short sequence made of the reference's own pair -- frames 1, 2, 1 -- in ONE RegisterRGBDSequence call with
// the pair list (0,1) (1,2) (0,2) (1,1), and checks it against RegisterRGBD called pair by pair with the same seeds:
// pair k of the sequence call draws from seed + k, so every Rt must come out with the same bits.  A fourth frame has a
// depth image and no records (a default-constructed SiftData): the pairs (0,3) and (3,1) give the identity, no matches
// and empty rows, as RegisterRGBD does.  An empty pair list is the walk (i, i + 1); no frames give empty outputs.
//
//   rgbd_batch_dropin sift1.bin sift2.bin depth1.u16 depth2.u16 intrinsics.txt
// depth*.u16: 640 x 480 raw little-endian 16-bit samples as stored in the reference's PNGs (the Python test writes them
// from tests/golden/rgbd_depth.npz).  Prints "pair Rt" and "sequence Rt" of the pair (0, 1) in the same format.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "debug.h"
#include "rgbd.h"

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

static const int W = 640, H = 480;
static const uint64_t kSeed = 7;

static bool read_file(const char *path, void *dst, size_t bytes) {
  FILE *fp = std::fopen(path, "rb");
  if (!fp) return false;
  const bool ok = std::fread(dst, 1, bytes, fp) == bytes;
  std::fclose(fp);
  return ok;
}

static void print_rt(const char *what, const float *Rt) {
  std::printf("%s\n", what);
  for (int i = 0; i < 3; i++) std::printf("  % .9g % .9g % .9g % .9g\n", Rt[4 * i], Rt[4 * i + 1], Rt[4 * i + 2], Rt[4 * i + 3]);
}

int main(int argc, char **argv) {
  if (argc < 6) {
    std::printf("usage: %s sift1 sift2 depth1.u16 depth2.u16 intrinsics.txt\n", argv[0]);
    return 2;
  }
  InitCuda(0);
  std::vector<unsigned short> depth1((size_t)W * H), depth2((size_t)W * H);
  double K[9];
  FILE *fp = std::fopen(argv[5], "r");
  bool ok = fp != NULL;
  for (int i = 0; ok && i < 9; i++) ok = std::fscanf(fp, "%lf", &K[i]) == 1;
  if (fp) std::fclose(fp);
  ok = ok && read_file(argv[3], depth1.data(), 2 * depth1.size()) && read_file(argv[4], depth2.data(), 2 * depth2.size());
  if (!ok) {
    std::printf("FAILED: cannot read the inputs\n");
    return 1;
  }
  cusift_camera cam;
  cam.fx = (float)K[0], cam.fy = (float)K[4], cam.cx = (float)K[2], cam.cy = (float)K[5];
  cam.origin = 1.0f, cam.units_per_metre = 1000.0f, cam.encoding = 1;

  SiftData f0, f1, f2, f3;  // f3 as constructed: d_data == nullptr, numPts == 0
  EXPECT(ReadVLFeatSiftData(f0, argv[1]) > 0 && ReadVLFeatSiftData(f1, argv[2]) > 0 && ReadVLFeatSiftData(f2, argv[1]) > 0,
         "cannot read the VLFeat dumps");
  std::vector<SiftData *> frames;
  frames.push_back(&f0), frames.push_back(&f1), frames.push_back(&f2), frames.push_back(&f3);
  std::vector<const unsigned short *> depths;
  depths.push_back(depth1.data()), depths.push_back(depth2.data()), depths.push_back(depth1.data());
  depths.push_back(depth2.data());  // every frame's depth is uploaded, also that of the frame without records
  std::vector<std::pair<int, int> > pairs;
  pairs.push_back(std::make_pair(0, 1)), pairs.push_back(std::make_pair(1, 2)), pairs.push_back(std::make_pair(0, 2));
  pairs.push_back(std::make_pair(1, 1)), pairs.push_back(std::make_pair(0, 3)), pairs.push_back(std::make_pair(3, 1));

  // ---- the whole list in one call (first: it leaves the frames' own records untouched) ----
  std::vector<float> Rt;
  std::vector<int> numInliers, numMatches;
  std::vector<std::vector<std::pair<int, int> > > selected;
  std::vector<std::vector<char> > inliers;
  RegisterRGBDSequence(frames, depths, W, H, cam, pairs, Rt, &numInliers, &numMatches, 1024, 0.05f, RigidTransformType3D,
                       MatchSiftDistanceL2, 1000.0f, 0.6f, kSeed, &selected, &inliers);
  EXPECT(Rt.size() == 12 * pairs.size() && numInliers.size() == pairs.size() && numMatches.size() == pairs.size(),
         "%zu transforms for %zu pairs", Rt.size() / 12, pairs.size());
  EXPECT(numMatches[0] == 330, "%d matches for the pair (0, 1)", numMatches[0]);
  EXPECT(numInliers[0] >= 325 && numInliers[0] <= 327, "%d inliers for the pair (0, 1)", numInliers[0]);

  // ---- pair by pair, on fresh copies of the records, pair k with seed + k ----
  for (size_t k = 0; k < pairs.size(); k++) {
    SiftData a, b;
    if (pairs[k].first != 3) ReadVLFeatSiftData(a, argv[pairs[k].first == 1 ? 2 : 1]);
    if (pairs[k].second != 3) ReadVLFeatSiftData(b, argv[pairs[k].second == 1 ? 2 : 1]);
    float one[12];
    int in = -1, nm = -1;
    std::vector<std::pair<int, int> > sel;
    std::vector<char> flags;
    RegisterRGBD(a, b, depths[pairs[k].first], depths[pairs[k].second], W, H, cam, one, &in, &nm, 1024, 0.05f,
                 RigidTransformType3D, MatchSiftDistanceL2, 1000.0f, 0.6f, kSeed + k, &sel, &flags);
    if (k == 0) {
      print_rt("pair Rt", one);
      print_rt("sequence Rt", Rt.data());
    }
    EXPECT(std::memcmp(one, Rt.data() + 12 * k, sizeof(one)) == 0, "pair %zu: the sequence call gave another Rt", k);
    EXPECT(in == numInliers[k] && nm == numMatches[k], "pair %zu: %d / %d inliers, %d / %d matches", k, in, numInliers[k],
           nm, numMatches[k]);
    EXPECT(sel == selected[k], "pair %zu: other selected matches", k);
    EXPECT(flags == inliers[k], "pair %zu: other inlier flags", k);
    if (pairs[k].first == 3 || pairs[k].second == 3) {
      const float ident[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
      EXPECT(std::memcmp(ident, Rt.data() + 12 * k, sizeof(ident)) == 0 && numMatches[k] == 0 && numInliers[k] == 0 &&
                 selected[k].empty() && inliers[k].empty(),
             "pair %zu: %d matches, %d inliers, %zu selected with an empty frame", k, numMatches[k], numInliers[k],
             selected[k].size());
    }
    std::printf("pair (%d, %d): matches %d, inliers %d\n", pairs[k].first, pairs[k].second, numMatches[k], numInliers[k]);
  }
  // an empty pair list is the walk (i, i + 1), byte for byte; a sequence without frames gives empty outputs and no error
  std::vector<std::pair<int, int> > none, steps;
  for (int i = 0; i + 1 < 4; i++) steps.push_back(std::make_pair(i, i + 1));
  std::vector<float> walk, stepped;
  std::vector<int> walkIn, walkM, steppedIn, steppedM;
  RegisterRGBDSequence(frames, depths, W, H, cam, none, walk, &walkIn, &walkM, 1024, 0.05f, RigidTransformType3D,
                       MatchSiftDistanceL2, 1000.0f, 0.6f, kSeed);
  RegisterRGBDSequence(frames, depths, W, H, cam, steps, stepped, &steppedIn, &steppedM, 1024, 0.05f, RigidTransformType3D,
                       MatchSiftDistanceL2, 1000.0f, 0.6f, kSeed);
  EXPECT(walk.size() == 36 && walk.size() == stepped.size() &&
             std::memcmp(walk.data(), stepped.data(), sizeof(float) * walk.size()) == 0 && walkIn == steppedIn && walkM == steppedM,
         "the default pairs differ from the explicit walk");
  EXPECT(walk.size() >= 12 && std::memcmp(walk.data(), Rt.data(), 12 * sizeof(float)) == 0, "the walk's pair (0, 1)");
  std::vector<SiftData *> nobody;
  std::vector<const unsigned short *> noDepths;
  RegisterRGBDSequence(nobody, noDepths, W, H, cam, none, walk, &walkIn, &walkM, 1024, 0.05f, RigidTransformType3D,
                       MatchSiftDistanceL2, 1000.0f, 0.6f, kSeed);
  EXPECT(walk.empty() && walkIn.empty() && walkM.empty(), "an empty sequence gave %zu floats", walk.size());
  std::printf(failures ? "FAILED (%d)\n" : "PASSED\n", failures);
  return failures ? 1 : 0;
}
