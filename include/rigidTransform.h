// rigidTransform.h -- drop-in for the reference's extras/rigidTransform.h on top of the C ABI: RANSAC estimate of the
// rigid motion between two sets of matched 3-D points (SiftPoint::coords3D), x ~ R y + t.
// Same enum, signatures and defaults (extras/rigidTransform.h:16-34); sampling, the per-hypothesis estimate, the inlier
// count, the selection and the final refit all run on the GPU in cusift_estimate_rigid() (cusift_amd_extras.h says
// exactly what it computes and where it deliberately leaves the reference).  Plain C++: no HIP headers, no cuRAND.
#ifndef CUSIFT_AMD_RIGIDTRANSFORM_H
#define CUSIFT_AMD_RIGIDTRANSFORM_H

#include <cstddef>
#include <cstring>
#include <ctime>
#include <vector>

#include "cuSIFT.h"
#include "cusift_amd_extras.h"
#include "matching.h"

typedef enum { RigidTransformType2D, RigidTransformType3D } RigidTransformType;

// h_coord: numPts x 6 (reference-frame xyz, moving-frame xyz); Rt_relative: 12 floats, [R | t] row-major.
// h_indices: numLoops x 3 sample indices, or NULL: drawn on the device, seeded with time(0) like the reference
// (extras/rigidTransform.cu:411).  Unlike the reference (:444) h_indices is only read.  h_inliers: numPts flags of the
// winning hypothesis, or NULL.
inline void EstimateRigidTransformH(const float *h_coord, float *Rt_relative, int *numInliers, int numLoops, int numPts,
                                    float thresh2, RigidTransformType type = RigidTransformType2D,
                                    int *h_indices = NULL, char *h_inliers = NULL) {
  const uint64_t seed = h_indices == NULL ? (uint64_t)std::time(0) : 0;
  safeCall(cusift_estimate_rigid(cusift_dropin::ctx(), h_coord, numPts, h_indices, numLoops, thresh2,
                                 type == RigidTransformType3D ? 1 : 0, seed, Rt_relative, numInliers, NULL, h_inliers,
                                 NULL, NULL, NULL));
}

// Convenience function over a vector of SiftMatch (coords3D of pt1 = reference frame, of pt2 = moving frame);
// thresh is a distance, not its square.
inline void EstimateRigidTransform(std::vector<SiftMatch *> matches, float *Rt_relative, int *numInliers, int numLoops,
                                   float thresh, RigidTransformType type, int *h_indices = NULL,
                                   char *h_inliers = NULL) {
  std::vector<float> h_coord(6 * matches.size());
  for (size_t i = 0; i < matches.size(); i++) {
    std::memcpy(&h_coord[6 * i], matches[i]->pt1->coords3D, sizeof(float) * 3);
    std::memcpy(&h_coord[6 * i + 3], matches[i]->pt2->coords3D, sizeof(float) * 3);
  }
  EstimateRigidTransformH(h_coord.data(), Rt_relative, numInliers, numLoops, (int)matches.size(), thresh * thresh, type,
                          h_indices, h_inliers);
}

#endif  // CUSIFT_AMD_RIGIDTRANSFORM_H
