// sift_select.hip -- keep the K strongest keypoints of every image (cusift_ctx_set_keep_strongest, cusift_select_strongest):
// the selection between the detections, which append 64-byte record HEADS to one list per octave (sift_types.h:
// SegmentTable), and describe_all_kernel, which moves the heads into SiftData and describes them.  A keypoint that is
// dropped here costs its head and nothing else.  New functionality: the reference bounds SiftData with maxPts alone.
//
// The total order (first = strongest; include/cusift_amd.h has the contract):
//   1. key = |sharpness| as its IEEE bit pattern, 0 when sharpness is not finite        larger first
//   2. subsampling                                                                       larger first (the coarser octave)
//   3. coords2D[1] (y), then coords2D[0] (x), then scale                                smaller first
// Floats of 2. and 3. are compared through the usual order-preserving map to unsigned integers (ordered_bits), so the
// whole order is one lexicographic comparison of five 32-bit words and nothing below decides with floating point.
//
// Three launches, whatever the images hold, all on the context's stream, no host read-back:
//   select_gather_kernel     every head's cache line is read ONCE; its key goes to a dense array in the arena
//   select_cut_kernel        one workgroup per image: an 8-bit radix select over the dense keys (LDS histograms, integer
//                            atomics) finds the key T of the K-th strongest keypoint; if the group key == T straddles the
//                            cut, the same radix select over the group's secondary words (octave, y, x, scale) finds the
//                            last of it that is kept.  Result: a SelectCut per image.
//   select_partition_kernel  one workgroup per (image, list): flags the kept heads, then fills the holes below the new
//                            count with the kept heads at and above it -- sources and destinations are disjoint ranges,
//                            so nothing is read after it was overwritten -- and writes the list's new count.
// Two records that agree in all five words are interchangeable; where such a group straddles the cut as many of it are
// admitted as the cut has room for (an integer ticket per image), which ones is unspecified.
#include "sift_host.h"

namespace cusift {

constexpr int kGatherThreads = 256, kSelectThreads = 1024;
constexpr unsigned int kNoQuota = 0xffffffffu;

// What select_cut_kernel leaves per image: a head is kept iff (key, sec) comes before or at (key, sec[]) in the total
// order; of the heads AT it at most `quota` are admitted (kNoQuota: all), counted in `ticket`.
struct SelectCut {
  unsigned int key;
  unsigned int sec[4];
  unsigned int quota, ticket, kept;
};
static_assert(sizeof(SelectCut) == 32, "one SelectCut per image, 32 bytes apart");

__device__ __forceinline__ unsigned int ordered_bits(float f) {  // a < b  <=>  ordered_bits(a) < ordered_bits(b)
  const unsigned int b = __float_as_uint(f);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ unsigned int strength_key(float sharpness) {
  const unsigned int b = __float_as_uint(sharpness) & 0x7fffffffu;
  return b < 0x7f800000u ? b : 0u;  // inf and NaN rank last
}
constexpr int kSharpFloat = (int)(offsetof(cusift_point, sharpness) / sizeof(float));
constexpr int kSubFloat = (int)(offsetof(cusift_point, subsampling) / sizeof(float));
static_assert(kSharpFloat == 3 && kSubFloat < 16, "record head layout");

// the secondary words of a head, smaller = earlier: octave (coarser first), y, x, scale
__device__ __forceinline__ void secondary_words(const char *head, unsigned int s[4]) {
  const float4 a = *reinterpret_cast<const float4 *>(head);  // x, y, scale, sharpness
  const float sub = reinterpret_cast<const float *>(head)[kSubFloat];
  s[0] = ~ordered_bits(sub);
  s[1] = ordered_bits(a.y);
  s[2] = ordered_bits(a.x);
  s[3] = ordered_bits(a.z);
}

__device__ __forceinline__ unsigned int held(const SegmentTable &G, int r, int i, int capacity) {
  const unsigned int c = G.count[r][i];
  return c < (unsigned int)capacity ? c : (unsigned int)capacity;
}

// A slot for every lane with `p` set, from a counter in LDS: one atomic per wave.  Called by whole waves.
__device__ __forceinline__ unsigned int wave_slots(bool p, unsigned int *ctr) {
  const unsigned long long m = __ballot(p);
  if (m == 0) return 0;
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
  unsigned int first = 0;
  if (lane == leader) first = atomicAdd(ctr, (unsigned int)__popcll(m));
  first = __shfl(first, leader);
  return first + (unsigned int)__popcll(m & ((1ull << lane) - 1ull));
}

// ------------------------------------------------------------------------------------------------
// keys[(i * n_seg + r) * capacity + j] = key of head j of list r of image i, j < the list's held count
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGatherThreads) select_gather_kernel(SegmentTable G, int capacity,
                                                                        unsigned int *__restrict__ keys) {
  const int r = blockIdx.y, i = blockIdx.z;
  const unsigned int cnt = held(G, r, i, capacity);
  const unsigned int j = blockIdx.x * kGatherThreads + threadIdx.x;
  if (j >= cnt) return;
  const char *head = G.base[r] + ((size_t)i * capacity + j) * kStagedRecBytes;
  keys[((size_t)i * G.n_seg + r) * capacity + j] = strength_key(reinterpret_cast<const float *>(head)[kSharpFloat]);
}

// The bin of a 256-bin histogram in which the `need`-th entry from the TOP lies (1 <= need <= the histogram's total):
// wave 0 leaves the bin, the entries still needed from inside it and the bin's own count in out[0..2].
__device__ __forceinline__ void find_bin_from_top(const unsigned int *hist, unsigned int need, unsigned int *out) {
  const int lane = threadIdx.x;  // < 64
  unsigned int h[4], s = 0;
  for (int b = 0; b < 4; ++b) s += h[b] = hist[4 * lane + b];
  unsigned int suffix = s;  // entries in this lane's bins and all higher ones
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned int other = __shfl_down(suffix, d);
    if (lane + d < 64) suffix += other;
  }
  unsigned int above = suffix - s;
  if (above < need && need <= suffix) {  // exactly one lane
    int b = 3;
    while (b > 0 && above + h[b] < need) above += h[b--];
    out[0] = 4 * lane + b;
    out[1] = need - above;
    out[2] = h[b];
  }
}

// ------------------------------------------------------------------------------------------------
// one workgroup per image: the cut
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSelectThreads) select_cut_kernel(SegmentTable G, int capacity, int keep,
                                                                     const unsigned int *__restrict__ keys,
                                                                     unsigned int *__restrict__ ties,
                                                                     SelectCut *__restrict__ cuts,
                                                                     unsigned int *__restrict__ kept_out) {
  __shared__ unsigned int hist[256];
  __shared__ unsigned int found[3];  // bin, entries needed inside it, entries in it
  __shared__ unsigned int n_ties;
  const int i = blockIdx.x, tid = threadIdx.x;
  const size_t image_base = (size_t)i * G.n_seg * capacity;
  unsigned int total = 0;
  for (int r = 0; r < G.n_seg; ++r) total += held(G, r, i, capacity);

  SelectCut cut;
  cut.key = 0;
  cut.sec[0] = cut.sec[1] = cut.sec[2] = cut.sec[3] = 0xffffffffu;
  cut.quota = kNoQuota;
  cut.ticket = 0;
  cut.kept = total < (unsigned int)keep ? total : (unsigned int)keep;
  if (total > (unsigned int)keep) {  // (uniform) the list is cut: find the keep-th strongest key, 8 bits at a time
    unsigned int prefix = 0, need = (unsigned int)keep, group = total;
    for (int shift = 24; shift >= 0; shift -= 8) {
      const unsigned int fixed = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int r = 0; r < G.n_seg; ++r) {
        const unsigned int cnt = held(G, r, i, capacity);
        const unsigned int *k = keys + image_base + (size_t)r * capacity;
        for (unsigned int j = tid; j < cnt; j += kSelectThreads) {
          const unsigned int key = k[j];
          if ((key & fixed) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
      }
      __syncthreads();
      if (tid < 64) find_bin_from_top(hist, need, found);
      __syncthreads();
      prefix |= found[0] << shift;
      need = found[1];
      group = found[2];
    }
    cut.key = prefix;
    if (need < group) {  // (uniform) the group key == prefix straddles the cut: its first `need` by the secondary words
      if (tid == 0) n_ties = 0;
      __syncthreads();
      unsigned int *tie = ties + image_base;  // the group's heads, as r * capacity + j
      for (int r = 0; r < G.n_seg; ++r) {
        const unsigned int cnt = held(G, r, i, capacity);
        const unsigned int *k = keys + image_base + (size_t)r * capacity;
        for (unsigned int j0 = 0; j0 < cnt; j0 += kSelectThreads) {  // whole waves: wave_slots
          const unsigned int j = j0 + tid;
          const bool mine = j < cnt && k[j] == prefix;
          const unsigned int slot = wave_slots(mine, &n_ties);
          if (mine) tie[slot] = (unsigned int)r * (unsigned int)capacity + j;
        }
      }
      __syncthreads();  // (also makes the workgroup's own stores to `tie` visible to its loads)
      // the need-th SMALLEST of the group's 128-bit secondary values: the radix select again, most significant byte
      // first, bins reversed so that the smallest byte is the top bin; it ends as soon as what is left is all kept
      const unsigned int n_tie = group;
      unsigned int sp[4] = {0u, 0u, 0u, 0u};
      int passes = 0;
#pragma unroll
      for (int word = 0; word < 4; ++word) {
        for (int shift = 24; shift >= 0 && need < group; shift -= 8, ++passes) {
          const unsigned int fixed = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
          if (tid < 256) hist[tid] = 0;
          __syncthreads();
          for (unsigned int e = tid; e < n_tie; e += kSelectThreads) {
            const unsigned int t = tie[e], r = t / (unsigned int)capacity, j = t - r * (unsigned int)capacity;
            unsigned int s[4];
            secondary_words(G.base[r] + ((size_t)i * capacity + j) * kStagedRecBytes, s);
            bool match = (s[word] & fixed) == sp[word];
#pragma unroll
            for (int w = 0; w < word; ++w) match = match && s[w] == sp[w];
            if (match) atomicAdd(&hist[255u - ((s[word] >> shift) & 255u)], 1u);
          }
          __syncthreads();
          if (tid < 64) find_bin_from_top(hist, need, found);
          __syncthreads();
          sp[word] |= (255u - found[0]) << shift;
          need = found[1];
          group = found[2];
        }
      }
      // bits the select did not have to look at: all ones (every head of the remaining group is kept)
#pragma unroll
      for (int word = 0; word < 4; ++word) {
        const int known = min(32, max(0, 8 * passes - 32 * word));
        cut.sec[word] = sp[word] | (known >= 32 ? 0u : 0xffffffffu >> known);
      }
      if (need < group) cut.quota = need;  // heads equal in all five words straddle the cut
    }
  }
  if (tid == 0) {
    cuts[i] = cut;
    if (kept_out) kept_out[i] = cut.kept;
  }
}

// ------------------------------------------------------------------------------------------------
// one workgroup per (list, image): keep what the cut keeps, compacted to the head of the list
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSelectThreads) select_partition_kernel(SegmentTable G, int capacity,
                                                                           unsigned int *__restrict__ keys,
                                                                           unsigned int *__restrict__ holes,
                                                                           SelectCut *__restrict__ cuts) {
  __shared__ unsigned int n_kept, n_holes, n_moved;
  const int r = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
  const unsigned int cnt = held(G, r, i, capacity);
  const SelectCut cut = cuts[i];
  const size_t list_base = ((size_t)i * G.n_seg + r) * capacity;
  unsigned int *flag = keys + list_base;  // the key of head j becomes its "kept" flag
  unsigned int *hole = holes + list_base;
  char *heads = const_cast<char *>(G.base[r]) + (size_t)i * capacity * kStagedRecBytes;
  if (tid == 0) n_kept = n_holes = n_moved = 0;
  __syncthreads();
  for (unsigned int j0 = 0; j0 < cnt; j0 += kSelectThreads) {  // whole waves: the ballot
    const unsigned int j = j0 + tid;
    bool kept = false;
    if (j < cnt) {
      const unsigned int key = flag[j];
      kept = key > cut.key;
      if (key == cut.key) {
        unsigned int s[4];
        secondary_words(heads + (size_t)j * kStagedRecBytes, s);
        int cmp = 0;  // of s against cut.sec, most significant word first
#pragma unroll
        for (int w = 3; w >= 0; --w) cmp = s[w] < cut.sec[w] ? -1 : s[w] > cut.sec[w] ? 1 : cmp;
        kept = cmp < 0 || (cmp == 0 && (cut.quota == kNoQuota || atomicAdd(&cuts[i].ticket, 1u) < cut.quota));
      }
      flag[j] = kept ? 1u : 0u;
    }
    const unsigned long long m = __ballot(kept);
    if ((tid & 63) == 0 && m) atomicAdd(&n_kept, (unsigned int)__popcll(m));
  }
  __syncthreads();  // (also makes the workgroup's own stores to `flag` visible to its loads)
  const unsigned int kept_total = n_kept;
  // a dropped head below the new count is a hole; a kept head at or above it moves into one (as many of each)
  for (unsigned int j0 = 0; j0 < kept_total; j0 += kSelectThreads) {
    const unsigned int j = j0 + tid;
    const bool is_hole = j < kept_total && flag[j] == 0u;
    const unsigned int slot = wave_slots(is_hole, &n_holes);
    if (is_hole) hole[slot] = j;
  }
  __syncthreads();
  for (unsigned int j0 = kept_total / kSelectThreads * kSelectThreads; j0 < cnt; j0 += kSelectThreads) {
    const unsigned int j = j0 + tid;
    const bool moves = j >= kept_total && j < cnt && flag[j] != 0u;
    const unsigned int slot = wave_slots(moves, &n_moved);
    if (moves) {
      const float4 *src = reinterpret_cast<const float4 *>(heads + (size_t)j * kStagedRecBytes);
      float4 *dst = reinterpret_cast<float4 *>(heads + (size_t)hole[slot] * kStagedRecBytes);
      const float4 a = src[0], b = src[1], c = src[2], d = src[3];
      dst[0] = a;
      dst[1] = b;
      dst[2] = c;
      dst[3] = d;
    }
  }
  if (tid == 0) const_cast<unsigned int *>(G.count[r])[i] = kept_total;
}

}  // namespace cusift

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
// scratch of one selection: [keys | tie group / holes | cuts], the first two one word per head of every list
size_t select_scratch_bytes(int n_lists, int n_images, int capacity) {
  const size_t words = align_up_sz((size_t)n_images * n_lists * capacity * sizeof(unsigned int), 256);
  return 2 * words + align_up_sz((size_t)n_images * sizeof(SelectCut), 256);
}

// Enqueues the three kernels on the context's stream.  G: the lists (heads [image][capacity], counters [image], both
// written); d_kept: NULL, or [image] for the images' kept totals.  The caller has checked the arguments.
int select_strongest_impl(cusift_ctx *ctx, const SegmentTable &G, int n_images, int capacity, int keep, char *scratch,
                          unsigned int *d_kept) {
  const size_t words = align_up_sz((size_t)n_images * G.n_seg * capacity * sizeof(unsigned int), 256);
  unsigned int *keys = reinterpret_cast<unsigned int *>(scratch);
  unsigned int *aux = reinterpret_cast<unsigned int *>(scratch + words);
  SelectCut *cuts = reinterpret_cast<SelectCut *>(scratch + 2 * words);
  hipLaunchKernelGGL(select_gather_kernel, dim3(idiv_up(capacity, kGatherThreads), G.n_seg, n_images),
                     dim3(kGatherThreads), 0, ctx->stream, G, capacity, keys);
  TRY(check_launch("select_gather"));
  hipLaunchKernelGGL(select_cut_kernel, dim3(n_images), dim3(kSelectThreads), 0, ctx->stream, G, capacity, keep,
                     (const unsigned int *)keys, aux, cuts, d_kept);
  TRY(check_launch("select_cut"));
  hipLaunchKernelGGL(select_partition_kernel, dim3(G.n_seg, n_images), dim3(kSelectThreads), 0, ctx->stream, G, capacity,
                     keys, aux, cuts);
  return check_launch("select_partition");
}

extern "C" int cusift_select_strongest(cusift_ctx *ctx, void *d_heads, int n_lists, int n_images, int capacity,
                                       unsigned int *d_counts, int keep, unsigned int *d_kept) {
  TRY(enter(ctx));
  if (!d_heads || !d_counts || !d_kept) return fail(CUSIFT_ERR_INVALID, "select_strongest: missing data");
  if (n_lists < 1 || n_lists > kMaxOctaves || n_images < 1 || n_images > 65535 || capacity < 1)
    return fail(CUSIFT_ERR_INVALID, "select_strongest: bad geometry lists=%d (1..%d) images=%d (1..65535) capacity=%d",
                n_lists, kMaxOctaves, n_images, capacity);
  if (keep < 1) return fail(CUSIFT_ERR_INVALID, "select_strongest: keep must be >= 1, got %d", keep);
  if ((size_t)n_lists * capacity > 0x7fffffffu || (size_t)n_images * n_lists * capacity > ((size_t)1 << 32))
    return fail(CUSIFT_ERR_INVALID, "select_strongest: %d lists x %d images x %d heads are too many", n_lists, n_images,
                capacity);
  TRY(ensure_arena(ctx, select_scratch_bytes(n_lists, n_images, capacity)));
  ctx->seg_clean_ptr = nullptr;  // (this call lays the arena out its own way)
  SegmentTable G;
  memset(&G, 0, sizeof(G));
  G.n_seg = n_lists;
  for (int r = 0; r < n_lists; ++r) {
    G.base[r] = static_cast<const char *>(d_heads) + (size_t)r * n_images * capacity * kStagedRecBytes;
    G.count[r] = d_counts + (size_t)r * n_images;
  }
  return select_strongest_impl(ctx, G, n_images, capacity, keep, ctx->arena, d_kept);
}
