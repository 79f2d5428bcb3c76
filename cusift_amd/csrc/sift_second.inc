// sift_second.inc -- second-peak orientations, the two kernels that run one wave per record: included at the end of
// sift_keypoints.hip, because they call its device functions (the units are built without relocatable device code, so a
// device function is callable only from the unit that holds it).  The scan between them, the host layer and the
// contract's implementation notes are in sift_second.hip; the contract is include/cusift_amd_extras.h's
// (cusift_second_orientations_batch).
//
//   second_peak_kernel      repeats the orientation stage of every valid record and leaves marks[image * max_pts + j] =
//                           the orientation of the histogram's second peak, or a NaN: no duplicate.
//   second_describe_kernel  walks the duplicates the scan has placed: copies the parent's record, sets the orientation and
//                           describes at it.
// Both are describe_given_kernel's frame called again -- RecordWalk, valid_keypoint, stage_given (octave rule, octave
// units, patch), with_sampler, store_descriptor -- so a record gets the histogram and the descriptor bits that kernel
// would give it.  Neither changes a byte of a record below its image's count.

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) second_peak_kernel(
    OctaveTable T, const cusift_point *__restrict__ points, int max_pts, const unsigned int *__restrict__ counters,
    int n_images, float q, float inv_q, float ratio, unsigned int flags, float *__restrict__ marks) {
  __shared__ KpShared S;
  __shared__ unsigned int s_prefix[kMaxFlatImages + 1];
  const int lane = threadIdx.x;
  const bool from_scale = (flags & CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE) != 0u;
  RecordWalk walk(s_prefix, (unsigned int)max_pts, n_images, lane, [&](int i) { return counters[i]; });

  for (unsigned int g = blockIdx.x; g < walk.total; g += gridDim.x) {  // wave-uniform
    const unsigned int idx = walk.locate(g);
    const cusift_point *pt = points + (long)walk.im * max_pts + idx;
    float *mark = marks + (long)walk.im * max_pts + idx;
    const float x = uniform(pt->coords2D[0]), y = uniform(pt->coords2D[1]), scale = uniform(pt->scale);
    const float rec_sub = uniform(pt->subsampling);
    if (!valid_keypoint(x, y, scale)) {
      if (lane == 0) *mark = __builtin_nanf("");
      continue;
    }
    // (the orientation's histogram does not depend on the sampler: same bits from the patch and from global memory)
    const int o = describe_octave_of(T, rec_sub, scale, from_scale);
    const GivenKeypoint K = stage_given(S, T, o, walk.im, x, y, scale, 0.0f, lane);
    const float px = K.px, py = K.py, kscale = K.kscale;
    float o2;
    with_sampler<kDescPatch>(K.use_patch, S.patch, K.pg, K.V, q, inv_q, [&](const auto &tex) {
      o2 = kp_orientation<true>(S, tex, kp_orientation_prep(S, tex, px, py, kscale, lane), px, py, kscale, lane, ratio);
    });
    if (lane == 0) *mark = o2;
    wave_sync();
  }
}

// dup_count[i]: the duplicates the scan placed for image i (counters[i] already counts them); parent[i * max_pts + k]: the
// record that duplicate k repeats; marks: the peak kernel's.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) second_describe_kernel(
    OctaveTable T, cusift_point *__restrict__ points, int max_pts, const unsigned int *__restrict__ counters,
    const unsigned int *__restrict__ dup_count, const unsigned int *__restrict__ parent, const float *__restrict__ marks,
    int n_images, float q, float inv_q, int root_sift, unsigned int flags) {
  __shared__ KpShared S;
  __shared__ unsigned int s_prefix[kMaxFlatImages + 1];
  const int lane = threadIdx.x;
  const bool from_scale = (flags & CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE) != 0u;
  RecordWalk walk(s_prefix, (unsigned int)max_pts, n_images, lane, [&](int i) { return dup_count[i]; });
  const DescLaneConsts C = desc_lane_consts(lane, q, inv_q);

  for (unsigned int g = blockIdx.x; g < walk.total; g += gridDim.x) {  // wave-uniform
    const unsigned int k = walk.locate(g);
    const int im = walk.im;
    const long base = (long)im * max_pts;
    // the scan's bounds, held again here: parent < first <= first + k < max_pts, or the item is left alone
    const unsigned int m = (unsigned int)__builtin_amdgcn_readfirstlane((int)dup_count[im]);
    const unsigned int cnt = (unsigned int)__builtin_amdgcn_readfirstlane((int)counters[im]);
    const unsigned int par = (unsigned int)__builtin_amdgcn_readfirstlane((int)parent[base + k]);
    if (cnt > (unsigned int)max_pts || m > cnt || par >= cnt - m) continue;
    const unsigned int first = cnt - m;  // the image's records before the stage
    const cusift_point *src = points + base + par;
    cusift_point *pt = points + base + first + k;
    const float ori = uniform(marks[base + par]);
    const float x = uniform(src->coords2D[0]), y = uniform(src->coords2D[1]), scale = uniform(src->scale);
    const float rec_sub = uniform(src->subsampling);
    const int o = describe_octave_of(T, rec_sub, scale, from_scale);
    // The parent's 147 dwords with the new orientation and the octave's subsampling; the 128 of `data` are left to the
    // descriptor's stores below, so every word of the record is written once, by one lane.
    const unsigned int *s = reinterpret_cast<const unsigned int *>(src);
    unsigned int *d = reinterpret_cast<unsigned int *>(pt);
    constexpr int kWords = (int)(sizeof(cusift_point) / 4), kOriWord = (int)(offsetof(cusift_point, orientation) / 4),
                  kSubWord = (int)(offsetof(cusift_point, subsampling) / 4),
                  kDataWord = (int)(offsetof(cusift_point, data) / 4);
    static_assert(sizeof(cusift_point) == 588 && kDataWord <= 64 && kWords - (kDataWord + 128) <= 64,
                  "one word per lane covers the head, one the tail");
    if (lane < kDataWord) d[lane] = lane == kOriWord ? sm_bits(ori) : lane == kSubWord ? sm_bits(T.sub[o]) : s[lane];
    if (kDataWord + 128 + lane < kWords) d[kDataWord + 128 + lane] = s[kDataWord + 128 + lane];
    const GivenKeypoint K = stage_given(S, T, o, im, x, y, scale, ori, lane);
    float b0, b1;
    with_sampler<kDescPatch>(K.use_patch, S.patch, K.pg, K.V, q, inv_q, [&](const auto &tex) {
      kp_descriptor(S, tex, C, K.px, K.py, K.kscale, ori, lane, b0, b1);
    });
    store_descriptor(S, pt, b0, b1, lane, root_sift);
    wave_sync();
  }
}
