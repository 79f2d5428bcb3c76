// sift_context.hip -- the context of the C ABI (include/cusift_amd.h): errors, device selection, the scratch arena, the
// launch policy, the side stream, the stage timers and the memory helpers.  Host logic follows cuSIFT.cu / cutils.h (cited
// per function); nothing here allocates, frees or reads back between stages once the arena is sized.
#include "sift_host.h"

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

int cusift_fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

static int fold_spans(cusift_ctx *ctx) {
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  for (auto &s : ctx->spans) {
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, s.start, s.stop));
    ctx->ms[s.stage] += t;
    ctx->launches[s.stage] += 1;
    ctx->event_pool.push_back(s.start);
    ctx->event_pool.push_back(s.stop);
  }
  ctx->spans.clear();
  return CUSIFT_OK;
}

// Arena offsets (Plan) are multiples of 256 and hipMalloc returns memory aligned to at least that, so whatever lives in
// the arena is 256-byte aligned: the octave driver decides its kernels without looking at an arena address.
int ensure_arena(cusift_ctx *ctx, size_t bytes) {
  if (bytes <= ctx->arena_bytes) return CUSIFT_OK;
  ctx->seg_clean_ptr = nullptr;
  TRY(grow_scratch(ctx, ctx->arena, ctx->arena_bytes, bytes, "arena ", true));
  if ((uintptr_t)ctx->arena % 256) return fail(CUSIFT_ERR_HIP, "hipMalloc returned an arena that is not 256-byte aligned");
  return CUSIFT_OK;
}

void scale_down_taps(ScaleDownTaps &T, float variance) {
  // cuSIFT.cu:320-341 (the pyramid passes variance = 0.5, cuSIFT.cu:185)
  float k[5], sum = 0.0f;
  for (int j = 0; j < 5; j++) {
    k[j] = (float)expf(-(double)(j - 2) * (j - 2) / 2.0 / variance);
    sum += k[j];
  }
  for (int j = 0; j < 5; j++) k[j] /= sum;
  T.k[0] = k[0];
  T.k[1] = k[1];
  T.k[2] = k[2];
}

void frac_consts(int frac_bits, float &q, float &inv_q) {
  // (<= 11 bits: the texture model's weight product A B / 2^q is then exact in fp32 -- sift_keypoints.hip, bilinear_weights)
  if (frac_bits > 0 && frac_bits <= 11) {
    q = (float)(1 << frac_bits);
    inv_q = 1.0f / q;
  } else {
    q = 0.0f;
    inv_q = 0.0f;
  }
}

// Every ctx-taking entry point starts here: a NULL check and the selection of the context's device BEFORE any
// allocation or launch (a process may hold contexts on several GPUs; the current device is per thread).
int enter(cusift_ctx *ctx) {
  if (!ctx) return fail(CUSIFT_ERR_INVALID, "ctx is NULL");
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != ctx->device) HIP_TRY(hipSetDevice(ctx->device));
  return CUSIFT_OK;
}

int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(CUSIFT_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
  return CUSIFT_OK;
}

// ------------------------------------------------------------------------------------------------
// process / device
// ------------------------------------------------------------------------------------------------
extern "C" const char *cusift_last_error(void) { return g_err.c_str(); }
extern "C" const char *cusift_version(void) { return "cusift_amd 0.1 (gfx950)"; }

extern "C" int cusift_device_count(int *count) {
  if (!count) return fail(CUSIFT_ERR_INVALID, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  *count = n;
  return CUSIFT_OK;
}

extern "C" int cusift_init(int device) {
  // InitCuda, cutils.h:71-92: clamp into [0, n-1], select
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(CUSIFT_ERR_NO_DEVICE, "no HIP device available");
  device = std::max(0, std::min(n - 1, device));
  HIP_TRY(hipSetDevice(device));
  return CUSIFT_OK;
}

// OPT-IN since round 4 (cusift_ctx_set_policy(ctx, CUSIFT_POLICY_SIDE_STREAM, 1 | 2), or CUSIFT_OCTAVE_OVERLAP=1 | 2 in the
// environment of an unchanged caller): whether a second stream runs beside the first depends on what else the process
// has created, and a context that decided that by itself -- by timing -- was a silent performance cliff under a
// profiler, on a busy box, or in a host with streams of its own.  1 trusts the caller: the stream is created and used.
// 2 keeps the probe below as an explicit request.
// A second stream only helps if the device runs it BESIDE the context's stream.  HIP maps streams onto a few hardware
// queues (GPU_MAX_HW_QUEUES, 4 by default) in the order of their first use, and the queues onto the compute pipes of
// the command processor round robin.  Two streams on one hardware queue run one after the other; two queues on one
// pipe run their kernels at the same time but the pipe serves one queue's packets while the other queue's wait, a few
// microseconds each -- worse than one queue for a chain of short launches (measured, 64 x 1080p: 1.29-1.35 ms beside each other, 1.55
// on one queue, 1.88 on one pipe: four streams in use before this one and 8 hardware queues).  Which case a new stream
// lands in depends on what else the process has created -- so the context finds out: a chain of sixteen 5 us probe
// kernels on its own stream is timed alone and while a 120 us probe runs on the candidate, and the candidate is kept
// only if the chain takes about as long in both cases.  Up to four candidates (consecutive hardware queues sit on
// different pipes); if none passes, the context never forks.  One-time cost: under a millisecond and a wait for the
// context's stream, at the first call that would fork.
__global__ void __launch_bounds__(64) spin_kernel(long ticks) {
  const long t0 = (long)wall_clock64();  // the 100 MHz constant clock
  while ((long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

int ensure_side_stream(cusift_ctx *ctx) {
  // (policy value 2 is "after the probe": a stream taken without it -- under value 1 or 3 -- does not qualify; it is
  // let go, once idle, and the probe runs)
  if (ctx->side && ctx->knobs.octave_overlap == 2 && !ctx->side_probed) {
    HIP_TRY(hipStreamSynchronize(ctx->side));
    HIP_TRY(hipStreamDestroy(ctx->side));
    ctx->side = nullptr;
  }
  if (ctx->side) return CUSIFT_OK;
  if (ctx->side_failed) return fail(CUSIFT_ERR_HIP, "no side stream runs beside the context's stream");
  if (!ctx->ev_fork) HIP_TRY(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
  if (!ctx->ev_join) HIP_TRY(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  constexpr int kChain = 16;
  constexpr long kShort = 500, kLong = 12000;  // 5 us, 120 us
  int rc = CUSIFT_OK;
  if (ctx->knobs.octave_overlap != 2) {  // 1 / 3: no probe -- the caller says a second stream is worth having
    ctx->side_probed = false;
    hipError_t e = hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (e != hipSuccess) {
      ctx->side = nullptr;
      ctx->side_failed = true;
      return fail(CUSIFT_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    }
    return CUSIFT_OK;
  }
  hipStream_t rejected[4] = {nullptr, nullptr, nullptr, nullptr};  // kept alive until the end so that each try is a NEW queue
  int n_rejected = 0;
  for (int attempt = 0; attempt < 4 && !ctx->side && rc == CUSIFT_OK; ++attempt) {
    hipStream_t cand = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&cand, hipStreamNonBlocking);
    if (e != hipSuccess) {
      rc = fail(CUSIFT_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
      break;
    }
    float alone = 1e30f, beside_ms = 1e30f;
    auto chain = [&](bool with_candidate, float &best) -> hipError_t {
      hipError_t err;
      if ((err = hipStreamSynchronize(cand)) != hipSuccess) return err;
      if ((err = hipStreamSynchronize(ctx->stream)) != hipSuccess) return err;
      if ((err = hipEventRecord(e0, ctx->stream)) != hipSuccess) return err;
      if (with_candidate) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, cand, kLong);
      for (int k = 0; k < kChain; ++k) hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, ctx->stream, kShort);
      if ((err = hipEventRecord(e1, ctx->stream)) != hipSuccess) return err;
      if ((err = hipEventSynchronize(e1)) != hipSuccess) return err;
      float ms = 0.f;
      if ((err = hipEventElapsedTime(&ms, e0, e1)) != hipSuccess) return err;
      best = std::min(best, ms);
      return hipStreamSynchronize(cand);
    };
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, cand, 1L);  // first use: the candidate's hardware queue is created here
    for (int rep = 0; rep < 2 && e == hipSuccess; ++rep) {
      e = chain(false, alone);
      if (e == hipSuccess) e = chain(true, beside_ms);
    }
    if (e != hipSuccess) {
      (void)hipStreamDestroy(cand);
      rc = fail(CUSIFT_ERR_HIP, "side stream probe failed: %s", hipGetErrorString(e));
      break;
    }
    const bool beside = beside_ms < 1.25f * std::max(alone, 0.08f);
    if (beside) {
      ctx->side = cand;
      ctx->side_probed = true;
    } else
      rejected[n_rejected++] = cand;
  }
  for (int i = 0; i < n_rejected; ++i) (void)hipStreamDestroy(rejected[i]);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (rc == CUSIFT_OK && !ctx->side) rc = fail(CUSIFT_ERR_HIP, "no side stream runs beside the context's stream");
  if (rc != CUSIFT_OK) ctx->side_failed = true;  // the callers go on with one stream
  return rc;
}

extern "C" void cusift_default_params(cusift_params *p) {
  if (!p) return;
  p->num_octaves = 5;
  p->init_blur = 0.0;
  p->peak_thresh = 3.0f;
  p->edge_thresh = 10.0f;  // the only value the reference uses (test/detector.cpp:46)
  p->lowest_scale = 0.0f;
  p->subsampling = 1.0f;
  p->max_pts = 1024;  // SiftData ctor default (cuSIFT.h:56)
  p->tex_frac_bits = 8;
  p->fused_detect = 1;
  p->root_sift = 0;
  p->concurrent_batches = 1;
  p->upsample = 0;
}

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
static int ctx_create_impl(cusift_ctx **out, int device, void *hip_stream, bool borrow) {
  if (!out) return fail(CUSIFT_ERR_INVALID, "out is NULL");
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(CUSIFT_ERR_NO_DEVICE, "no HIP device available");
  if (device < 0 || device >= n) return fail(CUSIFT_ERR_INVALID, "device %d out of range [0,%d)", device, n);
  HIP_TRY(hipSetDevice(device));
  cusift_ctx *ctx = new cusift_ctx();
  ctx->device = device;
  (void)hipDeviceGetAttribute(&ctx->num_cus, hipDeviceAttributeMultiprocessorCount, device);
  if (ctx->num_cus < 1) ctx->num_cus = 256;
  if (borrow) {
    ctx->stream = (hipStream_t)hip_stream;  // NULL = the null stream
  } else {
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete ctx;
      return fail(CUSIFT_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    }
    ctx->owns_stream = true;
  }
  hipError_t e = hipMalloc((void **)&ctx->d_counter1, 256);
  if (e == hipSuccess) e = hipMalloc((void **)&ctx->d_queue, kQueueShards * 128);
  if (e == hipSuccess) e = hipHostMalloc((void **)&ctx->h_counter1, 256, hipHostMallocDefault);
  if (e != hipSuccess) {
    if (ctx->d_counter1) (void)hipFree(ctx->d_counter1);
    if (ctx->d_queue) (void)hipFree(ctx->d_queue);
    if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return fail(CUSIFT_ERR_NOMEM, "hipMalloc failed: %s", hipGetErrorString(e));
  }
  *out = ctx;
  return CUSIFT_OK;
}

extern "C" int cusift_ctx_create(cusift_ctx **out, int device, void *hip_stream) {
  return ctx_create_impl(out, device, hip_stream, hip_stream != nullptr);
}

extern "C" int cusift_ctx_create_borrowed(cusift_ctx **out, int device, void *hip_stream) {
  return ctx_create_impl(out, device, hip_stream, true);
}

extern "C" int cusift_ctx_destroy(cusift_ctx *ctx) {
  if (!ctx) return CUSIFT_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  for (auto &s : ctx->spans) {
    (void)hipEventDestroy(s.start);
    (void)hipEventDestroy(s.stop);
  }
  for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
  if (ctx->arena) (void)hipFree(ctx->arena);
  if (ctx->dog) (void)hipFree(ctx->dog);
  if (ctx->u8_stage) (void)hipFree(ctx->u8_stage);
  if (ctx->register_scratch) (void)hipFree(ctx->register_scratch);
  if (ctx->pairs_scratch) (void)hipFree(ctx->pairs_scratch);
  if (ctx->match_scratch) (void)hipFree(ctx->match_scratch);
  if (ctx->match_col_scratch) (void)hipFree(ctx->match_col_scratch);
  if (ctx->q8_scratch) (void)hipFree(ctx->q8_scratch);
  if (ctx->tracks_scratch) (void)hipFree(ctx->tracks_scratch);
  if (ctx->bundle_scratch) (void)hipFree(ctx->bundle_scratch);
  if (ctx->d_counter1) (void)hipFree(ctx->d_counter1);
  if (ctx->d_queue) (void)hipFree(ctx->d_queue);
  if (ctx->h_counter1) (void)hipHostFree(ctx->h_counter1);
  if (ctx->side) {
    (void)hipStreamSynchronize(ctx->side);
    (void)hipStreamDestroy(ctx->side);
  }
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
  if (ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return CUSIFT_OK;
}

extern "C" int cusift_ctx_synchronize(cusift_ctx *ctx) {
  TRY(enter(ctx));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CUSIFT_OK;
}

extern "C" void *cusift_ctx_stream(cusift_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
extern "C" int cusift_ctx_device(cusift_ctx *ctx) { return ctx ? ctx->device : -1; }

extern "C" int cusift_ctx_wait(cusift_ctx *ctx, cusift_ctx *other) {
  TRY(enter(ctx));
  if (!other) return fail(CUSIFT_ERR_INVALID, "other is NULL");
  if (other == ctx || other->stream == ctx->stream) return CUSIFT_OK;  // same stream: already ordered
  if (other->device != ctx->device) return fail(CUSIFT_ERR_INVALID, "contexts live on different devices");
  hipEvent_t ev = nullptr;
  HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, other->stream);
  if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, ev, 0);
  (void)hipEventDestroy(ev);  // destruction is deferred until the event has completed
  if (e != hipSuccess) return fail(CUSIFT_ERR_HIP, "cusift_ctx_wait: %s", hipGetErrorString(e));
  return CUSIFT_OK;
}

// scratch of cusift_extract_bands: [counters of the bands | running sums | a list of heads per band]
size_t bands_arena_bytes(int n_bands, int max_pts) { return 512 + (size_t)max_pts * kStagedRecBytes * (size_t)n_bands; }

extern "C" int cusift_ctx_reserve_bands(cusift_ctx *ctx, int n_bands, int max_pts) {
  TRY(enter(ctx));
  if (n_bands < 0 || n_bands > kMaxMultiOctaves || max_pts < 1)
    return fail(CUSIFT_ERR_INVALID, "reserve_bands: 0..%d bands, max_pts >= 1", kMaxMultiOctaves);
  return n_bands ? ensure_arena(ctx, bands_arena_bytes(n_bands, max_pts)) : CUSIFT_OK;
}

extern "C" size_t cusift_ctx_arena_bytes(cusift_ctx *ctx) { return ctx ? ctx->arena_bytes + ctx->dog_bytes : 0; }
extern "C" unsigned long cusift_ctx_forks(cusift_ctx *ctx) { return ctx ? ctx->forks : 0; }

extern "C" int cusift_ctx_set_policy(cusift_ctx *ctx, int key, int value) {
  if (!ctx) return fail(CUSIFT_ERR_INVALID, "ctx is NULL");
  Knobs &k = ctx->knobs;
  switch (key) {
    case CUSIFT_POLICY_SIDE_STREAM:
      if (value < 0 || value > 3) return fail(CUSIFT_ERR_INVALID, "CUSIFT_POLICY_SIDE_STREAM: 0..3");
      if (value != k.octave_overlap) ctx->side_failed = false;  // a new request gets a new try
      k.octave_overlap = value;
      return CUSIFT_OK;
    case CUSIFT_POLICY_OCTAVE_LISTS:
      if (value < -1 || value > 1) return fail(CUSIFT_ERR_INVALID, "CUSIFT_POLICY_OCTAVE_LISTS: -1, 0 or 1");
      k.stage_all = value;
      return CUSIFT_OK;
    case CUSIFT_POLICY_GENERIC_KERNELS: k.force_generic = value != 0; return CUSIFT_OK;
    case CUSIFT_POLICY_LAUNCH_PER_OCTAVE: k.no_multi = value != 0; return CUSIFT_OK;
    case CUSIFT_POLICY_MATCH_SPLITS:
      if (value < 0) return fail(CUSIFT_ERR_INVALID, "CUSIFT_POLICY_MATCH_SPLITS: >= 0");
      k.match_splits = value;
      return CUSIFT_OK;
    case CUSIFT_POLICY_TILED_PER_OCTAVE: k.tiled_per_octave = value != 0; return CUSIFT_OK;
    case CUSIFT_POLICY_PYRAMID_IN_DETECT:
      if (value < -1 || value > 2) return fail(CUSIFT_ERR_INVALID, "CUSIFT_POLICY_PYRAMID_IN_DETECT: -1, 0, 1 or 2");
      k.pyramid_in_detect = value;
      return CUSIFT_OK;
  }
  return fail(CUSIFT_ERR_INVALID, "unknown policy key %d", key);
}

// Sticky per context, read by resolve_plan (sift_driver.hip) on every extraction; K against max_pts is checked there.
extern "C" int cusift_ctx_set_keep_strongest(cusift_ctx *ctx, int k) {
  if (!ctx) return fail(CUSIFT_ERR_INVALID, "ctx is NULL");
  if (k < 0) return fail(CUSIFT_ERR_INVALID, "keep_strongest: K must be >= 0 (0 = off), got %d", k);
  ctx->keep_strongest = k;
  return CUSIFT_OK;
}
int cusift_keep_strongest_of(const cusift_ctx *ctx) { return ctx ? ctx->keep_strongest : 0; }

// Sticky per context, read by the six cusift_register_* calls (sift_register.hip) when they enqueue their matcher.
extern "C" int cusift_ctx_set_cross_check(cusift_ctx *ctx, int on) {
  if (!ctx) return fail(CUSIFT_ERR_INVALID, "ctx is NULL");
  if (on != 0 && on != 1) return fail(CUSIFT_ERR_INVALID, "cross_check: 0 (off) or 1 (on), got %d", on);
  ctx->cross_check = on;
  return CUSIFT_OK;
}

extern "C" int cusift_ctx_set_match_bits(cusift_ctx *ctx, int bits) {
  if (!ctx) return fail(CUSIFT_ERR_INVALID, "ctx is NULL");
  if (bits != 32 && bits != 8) return fail(CUSIFT_ERR_INVALID, "match_bits: 32 (fp32) or 8 (bytes), got %d", bits);
  ctx->match_bits = bits;
  return CUSIFT_OK;
}

extern "C" int cusift_ctx_get_policy(cusift_ctx *ctx, int key, int *value) {
  if (!ctx || !value) return fail(CUSIFT_ERR_INVALID, "ctx / value is NULL");
  const Knobs &k = ctx->knobs;
  switch (key) {
    case CUSIFT_POLICY_SIDE_STREAM: *value = k.octave_overlap; return CUSIFT_OK;
    case CUSIFT_POLICY_OCTAVE_LISTS: *value = k.stage_all; return CUSIFT_OK;
    case CUSIFT_POLICY_GENERIC_KERNELS: *value = k.force_generic; return CUSIFT_OK;
    case CUSIFT_POLICY_LAUNCH_PER_OCTAVE: *value = k.no_multi; return CUSIFT_OK;
    case CUSIFT_POLICY_MATCH_SPLITS: *value = k.match_splits; return CUSIFT_OK;
    case CUSIFT_POLICY_TILED_PER_OCTAVE: *value = k.tiled_per_octave; return CUSIFT_OK;
    case CUSIFT_POLICY_PYRAMID_IN_DETECT: *value = k.pyramid_in_detect; return CUSIFT_OK;
  }
  return fail(CUSIFT_ERR_INVALID, "unknown policy key %d", key);
}

// ---- events on a context's stream: what TimerGPU (cutils.h:94-114) is made of ----
struct cusift_event {
  hipEvent_t ev = nullptr;
  int device = 0;
};

extern "C" int cusift_event_create(cusift_ctx *ctx, cusift_event **out) {
  if (!out) return fail(CUSIFT_ERR_INVALID, "out is NULL");
  *out = nullptr;
  TRY(enter(ctx));
  cusift_event *e = new cusift_event();
  e->device = ctx->device;
  hipError_t r = hipEventCreate(&e->ev);
  if (r != hipSuccess) {
    delete e;
    return fail(CUSIFT_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(r));
  }
  *out = e;
  return CUSIFT_OK;
}

extern "C" int cusift_event_record(cusift_event *ev, cusift_ctx *ctx) {
  if (!ev) return fail(CUSIFT_ERR_INVALID, "event is NULL");
  TRY(enter(ctx));
  HIP_TRY(hipEventRecord(ev->ev, ctx->stream));
  return CUSIFT_OK;
}

extern "C" int cusift_event_wait(cusift_event *ev, cusift_ctx *ctx) {
  if (!ev) return fail(CUSIFT_ERR_INVALID, "event is NULL");
  TRY(enter(ctx));
  if (ev->device != ctx->device) return fail(CUSIFT_ERR_INVALID, "event and context are on different devices");
  HIP_TRY(hipStreamWaitEvent(ctx->stream, ev->ev, 0));
  return CUSIFT_OK;
}

extern "C" int cusift_event_elapsed_ms(cusift_event *start, cusift_event *stop, float *ms) {
  if (!start || !stop || !ms) return fail(CUSIFT_ERR_INVALID, "event / ms is NULL");
  HIP_TRY(hipSetDevice(stop->device));
  HIP_TRY(hipEventSynchronize(stop->ev));
  HIP_TRY(hipEventElapsedTime(ms, start->ev, stop->ev));
  return CUSIFT_OK;
}

extern "C" int cusift_event_destroy(cusift_event *ev) {
  if (!ev) return CUSIFT_OK;
  (void)hipSetDevice(ev->device);
  (void)hipEventDestroy(ev->ev);
  delete ev;
  return CUSIFT_OK;
}

extern "C" int cusift_ctx_timing_enable(cusift_ctx *ctx, int on) {
  TRY(enter(ctx));
  if (!on && ctx->timing) TRY(fold_spans(ctx));
  ctx->timing = on != 0;
  return CUSIFT_OK;
}

extern "C" int cusift_ctx_timing_read(cusift_ctx *ctx, float ms[CUSIFT_NUM_STAGES], int launches[CUSIFT_NUM_STAGES]) {
  TRY(enter(ctx));
  TRY(fold_spans(ctx));
  for (int i = 0; i < CUSIFT_NUM_STAGES; ++i) {
    if (ms) ms[i] = ctx->ms[i];
    if (launches) launches[i] = ctx->launches[i];
  }
  return CUSIFT_OK;
}

extern "C" int cusift_ctx_timing_reset(cusift_ctx *ctx) {
  TRY(enter(ctx));
  TRY(fold_spans(ctx));
  for (int i = 0; i < CUSIFT_NUM_STAGES; ++i) {
    ctx->ms[i] = 0.f;
    ctx->launches[i] = 0;
  }
  return CUSIFT_OK;
}

extern "C" int cusift_kernel_occupancy(const char *kernel, int *blocks_per_cu, int *threads_per_block) {
  if (!kernel || !blocks_per_cu || !threads_per_block) return fail(CUSIFT_ERR_INVALID, "NULL argument");
  const std::string k(kernel);
  int n = 0, t = 256;
  hipError_t e = hipErrorInvalidValue;
  if (k == "detect_fused")  // single-wave workgroups, a 10.5 KB candidate list each
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, detect_fused_kernel<false, (int)sizeof(cusift_point), false>, t = 64,
                                                     kDetectWaveLdsFloats * sizeof(float));
  else if (k == "laplace_multi") e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, laplace_multi_fast_kernel<2>, t, 0);
  else if (k == "find_points") e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, find_points_fast_kernel, t, 0);
  else if (k == "scale_down") e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, scale_down_fast_kernel, t, 0);
  else if (k == "describe_all") e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, describe_all_kernel, t = 64, 0);
  else if (k == "orientations") e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, orientations_kernel, t = 64, 0);
  else if (k == "descriptors") e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, descriptors_kernel, t = 64, 0);
  else return fail(CUSIFT_ERR_INVALID, "unknown kernel '%s'", kernel);
  if (e != hipSuccess) return fail(CUSIFT_ERR_HIP, "occupancy query failed: %s", hipGetErrorString(e));
  *blocks_per_cu = n;
  *threads_per_block = t;
  return CUSIFT_OK;
}

// ------------------------------------------------------------------------------------------------
// memory helpers
// ------------------------------------------------------------------------------------------------
extern "C" int cusift_malloc(void **d_ptr, size_t bytes) {
  if (!d_ptr) return fail(CUSIFT_ERR_INVALID, "d_ptr is NULL");
  *d_ptr = nullptr;
  hipError_t e = hipMalloc(d_ptr, bytes ? bytes : 1);
  if (e != hipSuccess) return fail(CUSIFT_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  return CUSIFT_OK;
}

extern "C" int cusift_free(void *d_ptr) {
  if (d_ptr) HIP_TRY(hipFree(d_ptr));
  return CUSIFT_OK;
}

extern "C" int cusift_malloc_host(void **h_ptr, size_t bytes) {
  if (!h_ptr) return fail(CUSIFT_ERR_INVALID, "h_ptr is NULL");
  *h_ptr = nullptr;
  hipError_t e = hipHostMalloc(h_ptr, bytes ? bytes : 1, hipHostMallocDefault);
  if (e != hipSuccess) return fail(CUSIFT_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  return CUSIFT_OK;
}

extern "C" int cusift_free_host(void *h_ptr) {
  if (h_ptr) HIP_TRY(hipHostFree(h_ptr));
  return CUSIFT_OK;
}

extern "C" int cusift_memset(cusift_ctx *ctx, void *d_ptr, int value, size_t bytes) {
  if (!ctx || !d_ptr) return fail(CUSIFT_ERR_INVALID, "NULL argument");
  TRY(enter(ctx));
  HIP_TRY(hipMemsetAsync(d_ptr, value, bytes, ctx->stream));
  return CUSIFT_OK;
}

extern "C" int cusift_memcpy_h2d(cusift_ctx *ctx, void *d_dst, const void *h_src, size_t bytes) {
  if (!ctx || !d_dst || !h_src) return fail(CUSIFT_ERR_INVALID, "NULL argument");
  TRY(enter(ctx));
  HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CUSIFT_OK;
}

extern "C" int cusift_memcpy_d2h(cusift_ctx *ctx, void *h_dst, const void *d_src, size_t bytes) {
  if (!ctx || !h_dst || !d_src) return fail(CUSIFT_ERR_INVALID, "NULL argument");
  TRY(enter(ctx));
  HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CUSIFT_OK;
}

extern "C" int cusift_memcpy_d2d(cusift_ctx *ctx, void *d_dst, const void *d_src, size_t bytes) {
  if (!ctx || !d_dst || !d_src) return fail(CUSIFT_ERR_INVALID, "NULL argument");
  TRY(enter(ctx));
  if (bytes == 0) return CUSIFT_OK;
  HIP_TRY(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CUSIFT_OK;
}

extern "C" int cusift_image_h2d(cusift_ctx *ctx, float *d_dst, int dst_pitch, const float *h_src, int w, int h) {
  if (!ctx || !d_dst || !h_src || w < 1 || h < 1 || dst_pitch < w) return fail(CUSIFT_ERR_INVALID, "bad argument");
  TRY(enter(ctx));
  // cuImage::HostToDevice, cuImage.cu:83-92: dense host rows -> pitched device rows
  HIP_TRY(hipMemcpy2DAsync(d_dst, sizeof(float) * dst_pitch, h_src, sizeof(float) * w, sizeof(float) * w, h,
                           hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CUSIFT_OK;
}

extern "C" int cusift_image_d2h(cusift_ctx *ctx, float *h_dst, const float *d_src, int src_pitch, int w, int h) {
  if (!ctx || !h_dst || !d_src || w < 1 || h < 1 || src_pitch < w) return fail(CUSIFT_ERR_INVALID, "bad argument");
  TRY(enter(ctx));
  HIP_TRY(hipMemcpy2DAsync(h_dst, sizeof(float) * w, d_src, sizeof(float) * src_pitch, sizeof(float) * w, h,
                           hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return CUSIFT_OK;
}

