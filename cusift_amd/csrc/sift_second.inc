// sift_second.inc -- second-peak orientations, the two kernels that run one wave per record: included at the end of
// sift_keypoints.hip, because they call its device functions (kp_orientation, kp_descriptor, stage_patch: the units are
// built without relocatable device code, so a device function is callable only from the unit that holds it).  The scan
// between them, the host layer and the contract's implementation notes are in sift_second.hip; the contract is
// include/cusift_amd_extras.h's (cusift_second_orientations_batch).
//
//   second_peak_kernel      walks the records as describe_given_kernel does, repeats the orientation stage of every valid
//                           one (same octave, same units, same patch, same sampler) and leaves marks[image * max_pts + j] =
//                           the orientation of the histogram's second peak, or a NaN: no duplicate.
//   second_describe_kernel  walks the duplicates the scan has placed: copies the parent's record, sets the orientation and
//                           describes at it -- describe_given_kernel's keep-orientation route.
// Neither changes a byte of a record below its image's count.

// The record's octave by cusift_describe_batch's rule (describe_given_kernel): the recorded one, or from the scale.
__device__ __forceinline__ int second_octave_of(const OctaveTable &T, float rec_sub, float scale, bool from_scale) {
  int o = -1;
  if (!from_scale) {
    for (int i = T.n_oct - 1; i >= 0; --i)
      if (sm_bits(rec_sub) == sm_bits(T.sub[i])) o = i;
  }
  if (o < 0) {
    o = 0;
    for (int i = 1; i < T.n_oct; ++i)
      if (scale >= kDescribeLow * T.sub[i]) o = i;
  }
  return o;
}

// The walk of both kernels: running sums of the images' counts (clamped to `cap`) in s_prefix, the total returned.
__device__ __forceinline__ unsigned int second_prefix(unsigned int *s_prefix, const unsigned int *__restrict__ counts,
                                                      unsigned int cap, int n_images, int lane) {
  for (int i = lane; i < n_images; i += 64) {
    const unsigned int c = counts[i];
    s_prefix[i + 1] = c < cap ? c : cap;
  }
  wave_sync();
  running_sums_in_place(s_prefix, n_images, lane);
  wave_sync();
  return s_prefix[n_images];
}

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) second_peak_kernel(
    OctaveTable T, const cusift_point *__restrict__ points, int max_pts, const unsigned int *__restrict__ counters,
    int n_images, float q, float inv_q, float ratio, unsigned int flags, float *__restrict__ marks) {
  __shared__ KpShared S;
  __shared__ unsigned int s_prefix[kMaxFlatImages + 1];
  const int lane = threadIdx.x;
  const bool flat = gridDim.y == 1;  // wave-uniform; the host flattens up to kMaxFlatImages images
  const bool from_scale = (flags & CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE) != 0u;
  unsigned int total;
  int im;
  if (flat) {
    total = second_prefix(s_prefix, counters, (unsigned int)max_pts, n_images, lane);
    im = 0;
  } else {
    im = blockIdx.y;
    const unsigned int c = counters[im];
    total = c < (unsigned int)max_pts ? c : (unsigned int)max_pts;
  }
  total = (unsigned int)__builtin_amdgcn_readfirstlane((int)total);

  for (unsigned int g = blockIdx.x; g < total; g += gridDim.x) {  // wave-uniform
    unsigned int idx = g;
    if (flat) {
      while (__builtin_amdgcn_readfirstlane((int)s_prefix[im + 1]) <= g) ++im;  // ends: g < total = s_prefix[n_images]
      idx = g - (unsigned int)__builtin_amdgcn_readfirstlane((int)s_prefix[im]);
    }
    const cusift_point *pt = points + (long)im * max_pts + idx;
    float *mark = marks + (long)im * max_pts + idx;
    const float x = uniform(pt->coords2D[0]), y = uniform(pt->coords2D[1]), scale = uniform(pt->scale);
    const float rec_sub = uniform(pt->subsampling);
    if (!(finite_bits(x) && finite_bits(y) && finite_bits(scale) && scale > 0.0f)) {  // describe_given_kernel's validity
      if (lane == 0) *mark = __builtin_nanf("");
      continue;
    }
    const int o = second_octave_of(T, rec_sub, scale, from_scale);
    const float sub = T.sub[o];
    const float px = x / sub, py = y / sub, kscale = scale / sub;  // octave units
    const float *img = T.base[o] + (long)im * T.stride[o];
    const int w = T.w[o], h = T.h[o], pitch = T.pitch[o];
    const RowWindow rw{0, h};
    // the patch of describe_given_kernel (the orientation's histogram does not depend on the sampler: same bits)
    const float reach = fmaxf(7.5f * (12.0f / 16.0f * kscale) * 1.41422f + 1.0f + 0.01f, 6.0f);
    PatchGeom pg;
    int pw, ph;
    const bool use_patch = patch_for_reach(px, py, reach, pg, pw, ph);
    if (use_patch) stage_patch(img, w, h, pitch, rw, S.patch, pg, pw, ph, lane);
    wave_sync();
    float o2;
    if (use_patch) {
      if (q > 0.0f) {
        const PatchSampler<kDescPatch, true> tex{S.patch, pg.x0, pg.y0, q, inv_q};
        o2 = kp_orientation<true>(S, tex, kp_orientation_prep(S, tex, px, py, kscale, lane), px, py, kscale, lane, ratio);
      } else {
        const PatchSampler<kDescPatch, false> tex{S.patch, pg.x0, pg.y0, q, inv_q};
        o2 = kp_orientation<true>(S, tex, kp_orientation_prep(S, tex, px, py, kscale, lane), px, py, kscale, lane, ratio);
      }
    } else {
      const GlobalSampler tex{img, w, h, pitch, rw, q, inv_q};
      o2 = kp_orientation<true>(S, tex, kp_orientation_prep(S, tex, px, py, kscale, lane), px, py, kscale, lane, ratio);
    }
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
  const bool flat = gridDim.y == 1;
  const bool from_scale = (flags & CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE) != 0u;
  unsigned int total;
  int im;
  if (flat) {
    total = second_prefix(s_prefix, dup_count, (unsigned int)max_pts, n_images, lane);
    im = 0;
  } else {
    im = blockIdx.y;
    const unsigned int c = dup_count[im];
    total = c < (unsigned int)max_pts ? c : (unsigned int)max_pts;
  }
  total = (unsigned int)__builtin_amdgcn_readfirstlane((int)total);
  const DescLaneConsts C = desc_lane_consts(lane, q, inv_q);

  for (unsigned int g = blockIdx.x; g < total; g += gridDim.x) {  // wave-uniform
    unsigned int k = g;
    if (flat) {
      while (__builtin_amdgcn_readfirstlane((int)s_prefix[im + 1]) <= g) ++im;
      k = g - (unsigned int)__builtin_amdgcn_readfirstlane((int)s_prefix[im]);
    }
    const long base = (long)im * max_pts;
    // the scan's bounds, held again here: parent < first <= first + k < max_pts, or the item is left alone
    const unsigned int m = (unsigned int)__builtin_amdgcn_readfirstlane((int)dup_count[im]);
    const unsigned int cnt = (unsigned int)__builtin_amdgcn_readfirstlane((int)counters[im]);
    const unsigned int par = (unsigned int)__builtin_amdgcn_readfirstlane((int)parent[base + k]);
    if (cnt > (unsigned int)max_pts || m > cnt || par >= cnt - m) continue;
    const unsigned int first = cnt - m;  // the image's records before the stage
    const cusift_point *src = points + base + par;
    cusift_point *pt = points + base + first + k;
    float ori = uniform(marks[base + par]);
    const float x = uniform(src->coords2D[0]), y = uniform(src->coords2D[1]), scale = uniform(src->scale);
    const float rec_sub = uniform(src->subsampling);
    const int o = second_octave_of(T, rec_sub, scale, from_scale);
    const float sub = T.sub[o];
    const float px = x / sub, py = y / sub, kscale = scale / sub;  // octave units
    // The parent's 147 dwords with the new orientation and the octave's subsampling; the 128 of `data` are left to the
    // descriptor's stores below, so every word of the record is written once, by one lane.
    {
      const unsigned int *s = reinterpret_cast<const unsigned int *>(src);
      unsigned int *d = reinterpret_cast<unsigned int *>(pt);
      constexpr int kWords = (int)(sizeof(cusift_point) / 4), kOriWord = (int)(offsetof(cusift_point, orientation) / 4),
                    kSubWord = (int)(offsetof(cusift_point, subsampling) / 4),
                    kDataWord = (int)(offsetof(cusift_point, data) / 4);
      static_assert(sizeof(cusift_point) == 588 && kDataWord <= 64 && kWords - (kDataWord + 128) <= 64,
                    "one word per lane covers the head, one the tail");
      if (lane < kDataWord) d[lane] = lane == kOriWord ? sm_bits(ori) : lane == kSubWord ? sm_bits(sub) : s[lane];
      if (kDataWord + 128 + lane < kWords) d[kDataWord + 128 + lane] = s[kDataWord + 128 + lane];
    }
    const float *img = T.base[o] + (long)im * T.stride[o];
    const int w = T.w[o], h = T.h[o], pitch = T.pitch[o];
    const RowWindow rw{0, h};
    // describe_given_kernel's keep-orientation route, its fall-back to the global sampler included
    const float reach = fmaxf(7.5f * (12.0f / 16.0f * kscale) * 1.41422f + 1.0f + 0.01f, 6.0f);
    PatchGeom pg;
    int pw, ph;
    const bool use_patch = patch_for_reach(px, py, reach, pg, pw, ph) && fabsf(ori) < 1e9f;
    if (use_patch) stage_patch(img, w, h, pitch, rw, S.patch, pg, pw, ph, lane);
    wave_sync();
    float b0, b1;
    if (use_patch) {
      if (q > 0.0f)
        describe_given_one(S, PatchSampler<kDescPatch, true>{S.patch, pg.x0, pg.y0, q, inv_q}, C, px, py, kscale, true, ori,
                           lane, b0, b1);
      else
        describe_given_one(S, PatchSampler<kDescPatch, false>{S.patch, pg.x0, pg.y0, q, inv_q}, C, px, py, kscale, true, ori,
                           lane, b0, b1);
    } else {
      describe_given_one(S, GlobalSampler{img, w, h, pitch, rw, q, inv_q}, C, px, py, kscale, true, ori, lane, b0, b1);
    }
    const int e0 = desc_elem(lane);
    if (root_sift) {
      float *v = S.fin();
      v[e0] = b0;
      v[e0 + 4] = b1;
      wave_sync();
      rootsift_lanes(v, e0, e0 + 4, b0, b1);
    }
    pt->data[e0] = b0;
    pt->data[e0 + 4] = b1;
    wave_sync();
  }
}
