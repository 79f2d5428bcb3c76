// cuSIFT.h -- drop-in C++ surface of danielsuo/cuSIFT's extraction path for MI355X.
//
// A program written against the reference's cuSIFT.h / cuImage.h / cutils.h (the live `SiftData` class API of
// test/detector.cpp:41-49, or the legacy InitSiftData / ExtractSift / FreeSiftData trio of main.cpp:99-103,
// 324-349) compiles against this one header and links libcusift_amd.so.  Everything here is a thin
// inline shim over the C ABI in cusift_amd.h (SiftData::Describe: cusift_describe_batch of cusift_amd_extras.h): no HIP
// headers, no CUDA types.
//
// Differences from the reference, on purpose:
//   * the methods that took a cudaTextureObject_t (cuSIFT.h:68-71) are internal helpers of the reference
//     and are not exported; LaplaceMulti/FindPointsMulti/... are reachable through the C ABI instead;
//   * errors: the reference prints and exit(-1)s (cutils.h:24-48); so does safeCall() below, with the
//     library's message.  Define CUSIFT_NO_EXIT to get a std::runtime_error instead;
//   * SiftData's parameter fields are initialised (the reference leaves them indeterminate, cuSIFT.cu:13-32);
//   * copying a SiftData/cuImage is disabled (the reference double-frees).
#ifndef CUSIFT_AMD_DROPIN_H
#define CUSIFT_AMD_DROPIN_H

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>
#include <stdexcept>
#include <utility>
#include <vector>

#include "cusift_amd.h"
#include "cusift_amd_extras.h"  // cusift_describe_batch (SiftData::Describe)

// ---- cutils.h:15-18 -------------------------------------------------------------------------------
inline int iDivUp(int a, int b) { return (a % b != 0) ? (a / b + 1) : (a / b); }
inline int iDivDown(int a, int b) { return a / b; }
inline int iAlignUp(int a, int b) { return (a % b != 0) ? (a - a % b + b) : a; }
inline int iAlignDown(int a, int b) { return a - a % b; }

// ---- cutils.h:20-48: failure = message + exit(-1) ---------------------------------------------------
inline void cusift_check_(int rc, const char *what, const char *file, int line) {
  if (rc == CUSIFT_OK) return;
#ifdef CUSIFT_NO_EXIT
  (void)file;
  (void)line;
  throw std::runtime_error(std::string(what) + ": " + cusift_last_error());
#else
  std::fprintf(stderr, "safeCall() runtime error in file <%s>, line %i : %s (%s).\n", file, line, cusift_last_error(),
               what);
  std::exit(-1);
#endif
}
#define safeCall(expr) cusift_check_((expr), #expr, __FILE__, __LINE__)

namespace cusift_dropin {
// The reference keeps one implicit global context (default stream + file-scope device symbols,
// cuSIFT_D.cu:13-20), so one extraction at a time per process.  Here the implicit context is one lazily created
// cusift_ctx PER CALLING THREAD (its own stream and scratch arena) on the device chosen by InitCuda(): a
// single-threaded program behaves exactly as before, and a program that calls SiftData::Extract / ExtractSift from N
// host threads -- each with its own SiftData and cuImage objects, nothing else changed -- has N extractions in
// flight on the device (tests/cpp/threads_dropin.cpp).  Objects may cross threads: buffers belong to the device, not
// to a context.  Contexts live as long as the process (the reference's global state is never torn down either) unless
// shutdown() is called.
inline std::atomic<int> &device_slot() {
  static std::atomic<int> dev{0};
  return dev;
}
// A thread's context is PARKED when the thread ends, not destroyed: a destructor of thread-local storage is no place
// for GPU runtime calls (tools that intercept HIP keep thread-local state of their own, gone by then -- rocprofv3 aborts),
// and the next thread that needs a context on that device takes a parked one, arena and all: a program has as many
// contexts as it ever had threads extracting at once.  shutdown() destroys the calling thread's context and every parked one.
struct ctx_pool {
  std::mutex m;
  std::vector<std::pair<int, cusift_ctx *>> parked;
};
inline ctx_pool &pool() {
  static ctx_pool *p = new ctx_pool;  // never destroyed: threads may end during the process's own exit
  return *p;
}
struct thread_ctx {
  cusift_ctx *c = nullptr;
  int dev = -1;
  void park() {
    if (!c) return;
    std::lock_guard<std::mutex> lock(pool().m);
    pool().parked.emplace_back(dev, c);
    c = nullptr;
  }
  ~thread_ctx() { park(); }
};
inline thread_ctx &thread_slot() {
  static thread_local thread_ctx t;
  return t;
}
inline cusift_ctx *&ctx_slot() { return thread_slot().c; }
inline cusift_ctx *ctx() {
  thread_ctx &t = thread_slot();
  const int dev = device_slot().load(std::memory_order_relaxed);
  if (t.c && t.dev != dev) t.park();  // InitCuda() chose another device since this thread last extracted
  if (!t.c) {
    {
      std::lock_guard<std::mutex> lock(pool().m);
      auto &v = pool().parked;
      for (size_t i = 0; i < v.size(); ++i)
        if (v[i].first == dev) {
          t.c = v[i].second;
          v.erase(v.begin() + (long)i);
          break;
        }
    }
    if (!t.c) {
      safeCall(cusift_ctx_create(&t.c, dev, nullptr));
      // An unchanged caller of the reference's API has no handle on the launch policy; the one knob such a caller may
      // want -- octave 0's detection on a second stream, for large single batches -- is read HERE, in the shim that is
      // compiled into the caller, from CUSIFT_OCTAVE_OVERLAP (0..3 = CUSIFT_POLICY_SIDE_STREAM's values).  The library
      // itself reads no environment variable on the extraction path (until round 5 it read this one).
      if (const char *e = std::getenv("CUSIFT_OCTAVE_OVERLAP")) {
        const int v = std::atoi(e);
        if (v >= 0 && v <= 3) safeCall(cusift_ctx_set_policy(t.c, CUSIFT_POLICY_SIDE_STREAM, v));
      }
    }
    t.dev = dev;
  }
  return t.c;
}
inline void shutdown() {  // the calling thread's context and every parked one (call it where GPU calls are safe)
  thread_ctx &t = thread_slot();
  if (t.c) cusift_ctx_destroy(t.c);
  t.c = nullptr;
  std::lock_guard<std::mutex> lock(pool().m);
  for (auto &e : pool().parked) cusift_ctx_destroy(e.second);
  pool().parked.clear();
}
// SiftData's host records: pinned memory (the reference: malloc, cuSIFT.cu:24).  The class owns and frees the
// buffer (cuSIFT.cu:34-50), callers only index it (test/detector.cpp:56) -- pinned, the read-back at the end of
// every Extract is one DMA instead of a staged copy, and it does not serialise with other threads' transfers.
inline void *host_alloc(size_t bytes) {
  void *p = nullptr;
  safeCall(cusift_malloc_host(&p, bytes));
  return p;
}
inline void host_free(void *p) {
  if (p) cusift_free_host(p);
}
}  // namespace cusift_dropin

// ---- cutils.h:71-92 -------------------------------------------------------------------------------
inline void InitCuda(int devNum) {
  int n = 0;
  cusift_device_count(&n);
  if (!n) {
    std::cerr << "No GPU devices available" << std::endl;
    return;
  }
  if (devNum > n - 1) devNum = n - 1;
  if (devNum < 0) devNum = 0;
  cusift_dropin::device_slot().store(devNum);  // for every thread: each re-creates its context on its next call
  safeCall(cusift_init(devNum));
}

// ---- cutils.h:21-69: safeThreadSync / checkMsg / deviceInit -------------------------------------------------
// safeThreadSync(): cudaThreadSynchronize + exit(-1) on error -> wait for the drop-in context's stream.
// checkMsg(msg): the reference polls cudaGetLastError() after its own kernel launches; here every launch lives behind a
//   C-ABI entry point that returns a status (already routed through safeCall), so there is no sticky launch error left
//   to poll: the macro evaluates its argument and is otherwise a no-op, which keeps reference-style code compiling.
// deviceInit(dev): clamp into [0, n-1] and select, false if there is no device (cutils.h:50-69).
inline void cusift_safe_thread_sync_(const char *file, int line) {
  if (cusift_ctx_synchronize(cusift_dropin::ctx()) != CUSIFT_OK) {
#ifdef CUSIFT_NO_EXIT
    throw std::runtime_error(std::string("threadSynchronize(): ") + cusift_last_error());
#else
    std::fprintf(stderr, "threadSynchronize() runtime error in file '%s' in line %i : %s.\n", file, line,
                 cusift_last_error());
    std::exit(-1);
#endif
  }
}
#define safeThreadSync() cusift_safe_thread_sync_(__FILE__, __LINE__)
#define checkMsg(msg) ((void)(msg))
inline bool deviceInit(int dev) {
  int n = 0;
  cusift_device_count(&n);
  if (n == 0) {
    std::fprintf(stderr, "error: no GPU devices available.\n");
    return false;
  }
  if (dev < 0) dev = 0;
  if (dev > n - 1) dev = n - 1;
  InitCuda(dev);
  return true;
}

// ---- cutils.h:94-140 ------------------------------------------------------------------------------
// As in the reference: an event is recorded on the stream at construction, read() records a second one, waits for it and
// returns the GPU time between the two in milliseconds (cudaEventRecord / cudaEventSynchronize / cudaEventElapsedTime,
// cutils.h:98-113).  The stream is the drop-in context's: every kernel of this shim runs there, and a `cudaStream_t`
// of the caller has no meaning on this side (the argument is kept so that `TimerGPU timer(0)` compiles).
class TimerGPU {
 public:
  explicit TimerGPU(void * /*stream*/ = nullptr) {
    cusift_event_create(cusift_dropin::ctx(), &start);
    cusift_event_create(cusift_dropin::ctx(), &stop);
    if (start) cusift_event_record(start, cusift_dropin::ctx());
  }
  ~TimerGPU() {
    cusift_event_destroy(start);
    cusift_event_destroy(stop);
  }
  TimerGPU(const TimerGPU &) = delete;
  TimerGPU &operator=(const TimerGPU &) = delete;
  float read() {
    float ms = 0.0f;
    if (!start || !stop || cusift_event_record(stop, cusift_dropin::ctx()) != CUSIFT_OK ||
        cusift_event_elapsed_ms(start, stop, &ms) != CUSIFT_OK)
      return 0.0f;
    return ms;
  }

 private:
  cusift_event *start = nullptr, *stop = nullptr;
};

class TimerCPU {
 public:
  explicit TimerCPU(float /*freq_MHz*/) : t0(std::chrono::steady_clock::now()) {}
  float read() { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

 private:
  std::chrono::steady_clock::time_point t0;
};

// ---- cuImage.h:8-26, cuImage.cu ---------------------------------------------------------------------
class cuImage {
 public:
  int width, height;
  int pitch;      // in floats
  float *h_data;  // dense rows (width floats), borrowed unless h_internalAlloc
  float *d_data;  // pitched rows, owned iff d_internalAlloc
  float *t_data;  // kept for layout compatibility; never used (the reference's texture array)
  bool d_internalAlloc;
  bool h_internalAlloc;

  cuImage() : width(0), height(0), pitch(0), h_data(nullptr), d_data(nullptr), t_data(nullptr),
              d_internalAlloc(false), h_internalAlloc(false) {}
  // cuImage.cu:53-60
  cuImage(int w, int h, float *host, bool download = true)
      : width(0), height(0), pitch(0), h_data(nullptr), d_data(nullptr), t_data(nullptr), d_internalAlloc(false),
        h_internalAlloc(false) {
    AllocateWithHostMemory(w, h, host);
    if (download) HostToDevice();
  }
  ~cuImage() { release(); }
  cuImage(const cuImage &) = delete;
  cuImage &operator=(const cuImage &) = delete;

  // cuImage.cu:11-13
  void AllocateWithHostMemory(int w, int h, float *host) { Allocate(w, h, iAlignUp(w, 128), false, nullptr, host); }

  // cuImage.cu:16-46.  Wraps caller memory when given, allocates otherwise (pitch is honoured as passed).
  void Allocate(int w, int h, int p, bool withHost, float *dev = nullptr, float *host = nullptr) {
    release();
    width = w;
    height = h;
    pitch = p;
    d_data = dev;
    h_data = host;
    t_data = nullptr;
    if (d_data == nullptr) {
      void *ptr = nullptr;
      safeCall(cusift_malloc(&ptr, sizeof(float) * (size_t)pitch * (size_t)height));
      d_data = static_cast<float *>(ptr);
      d_internalAlloc = true;
    }
    if (withHost && h_data == nullptr) {
      h_data = static_cast<float *>(cusift_dropin::host_alloc(sizeof(float) * (size_t)pitch * (size_t)height));
      h_internalAlloc = true;
    }
  }

  // cuImage.cu:83-117: return milliseconds
  double HostToDevice() {
    TimerGPU timer;
    if (d_data != nullptr && h_data != nullptr)
      safeCall(cusift_image_h2d(cusift_dropin::ctx(), d_data, pitch, h_data, width, height));
    return timer.read();
  }
  double DeviceToHost() {
    TimerGPU timer;
    if (d_data != nullptr && h_data != nullptr)
      safeCall(cusift_image_d2h(cusift_dropin::ctx(), h_data, d_data, pitch, width, height));
    return timer.read();
  }

 private:
  void release() {
    if (d_internalAlloc && d_data != nullptr) cusift_free(d_data);
    if (h_internalAlloc) cusift_dropin::host_free(h_data);
    d_data = h_data = t_data = nullptr;
    d_internalAlloc = h_internalAlloc = false;
  }
};

// ---- cuSIFT.h:10-30 -------------------------------------------------------------------------------
class SiftPoint {
 public:
  float coords2D[2];
  float scale;
  float sharpness;
  float edgeness;
  float orientation;
  float score;
  float ambiguity;
  int match;
  float match_xpos;
  float match_ypos;
  float match_error;
  float subsampling;
  float empty[3];
  float data[128];
  float coords3D[3];
};
static_assert(sizeof(SiftPoint) == sizeof(cusift_point) && sizeof(SiftPoint) == 588, "SiftPoint is a 588-byte record");

// The reference times every Extract with a TimerGPU and prints the result (cuSIFT.cu:64,117-119).  With CUSIFT_QUIET
// nothing is printed, so nothing is timed either: two event creations, two records, a wait and two destructions per
// call are runtime-wide locks that callers on several threads would queue on.
#ifndef CUSIFT_QUIET
#define CUSIFT_REPORT_TIMER(name) TimerGPU name
#define CUSIFT_REPORT_READ(name) (name).read()
#else
#define CUSIFT_REPORT_TIMER(name) (void)0
#define CUSIFT_REPORT_READ(name) 0.0
#endif

// ---- cuSIFT.h:32-74, cuSIFT.cu:13-120 ---------------------------------------------------------------
class SiftData {
 public:
  int numPts;  // number of available SIFT points
  int maxPts;  // number of allocated SIFT points
  SiftPoint *h_data;
  SiftPoint *d_data;

  // parameters (cuSIFT.h:44-51); defaults are the values of test/detector.cpp:42-48
  int numOctaves;
  int numScales;  // never read on the live path of the reference either (NUM_SCALES is compile-time 5)
  double initBlur;
  float initSubsampling;
  float peakThresh;
  float edgeThresh;
  float lowestScale;
  // new: emit RootSIFT descriptors from Extract (fused into the descriptor kernel; the reference's commented-out
  // ExtractRootSift, cuSIFT.cu:122-134, ran ConvertSiftToRootSift as a second pass).  Last field: layout of the
  // reference's members is unchanged.
  bool rootSift;
  // new: also search Lowe's octave -1 -- Extract enlarges the image 2x on the device first (cusift_params.upsample;
  // upstream CudaSift's scaleUp) and numOctaves counts from the enlarged octave: its keypoints come last, with
  // subsampling 0.5 * the call's.  Meant for initBlur <= 0.5.  Trailing field, default false: source-compatible, the
  // layout of the reference's members is unchanged.  (initSubsampling stays unread, as in the reference.)
  bool scaleUp;
  // new: keep only the keepStrongest strongest keypoints of the image (by |sharpness|; ties: the coarser octave, then y,
  // x, scale -- cusift_ctx_set_keep_strongest), selected on the device before anything is described.  0 (default): all,
  // up to maxPts.  At most maxPts.  Handed to the calling thread's context on every Extract.  Trailing field, default 0.
  int keepStrongest;
  // new: second-peak orientations -- every keypoint whose orientation histogram has a second peak above
  // secondOrientation x the first is followed, behind the image's records, by a duplicate at that orientation with its own
  // descriptor (cusift_ctx_set_second_orientation; the duplication the reference leaves compiled out, cuSIFT_D.cu:380).
  // 0 (default): off; 0.8f is the reference's constant.  Handed to the calling thread's context on every Extract.
  // Trailing field, default 0.
  float secondOrientation;

  // cuSIFT.cu:13-32
  explicit SiftData(int maxPts_ = 1024, bool host = false, bool dev = false)
      : numPts(0), maxPts(0), h_data(nullptr), d_data(nullptr), numOctaves(5), numScales(5), initBlur(0.0),
        initSubsampling(1.0f), peakThresh(0.1f), edgeThresh(10.0f), lowestScale(0.0f), rootSift(false), scaleUp(false),
        keepStrongest(0), secondOrientation(0.0f) {
    allocate(maxPts_, host, dev);
  }
  ~SiftData() { release(); }
  SiftData(const SiftData &) = delete;
  SiftData &operator=(const SiftData &) = delete;

  // cuSIFT.cu:52-59
  void Synchronize() {
    if (h_data && d_data && numPts > 0)
      safeCall(cusift_memcpy_d2h(cusift_dropin::ctx(), h_data, d_data, sizeof(SiftPoint) * (size_t)numPts));
  }

  // New (not in the reference): puts the host AND device copies into the canonical order -- octave blocks coarsest
  // first as extracted, inside an octave by y, x, scale.  The append order inside an octave is that of an atomic
  // counter, racy in the reference as well (atomicInc, cuSIFT_D.cu:512); sort when arrays, not just sets, must
  // repeat from run to run.  Needs the host copy (host = true).
  void SortCanonical() {
    if (!h_data || numPts <= 0) return;
    safeCall(cusift_sort_points_host(as_c(h_data), numPts));
    if (d_data)
      safeCall(cusift_memcpy_h2d(cusift_dropin::ctx(), d_data, h_data, sizeof(SiftPoint) * (size_t)numPts));
  }

  // cuSIFT.cu:61-120: dense host image -> numPts, d_data, h_data
  void Extract(float *im, int width, int height, float subsampling = 1.0f) {
    CUSIFT_REPORT_TIMER(timer);
    require_device("Extract");
    cusift_params p = params(subsampling);
    safeCall(cusift_ctx_set_keep_strongest(cusift_dropin::ctx(), keepStrongest));
    safeCall(cusift_ctx_set_second_orientation(cusift_dropin::ctx(), secondOrientation));
    safeCall(cusift_extract_host(cusift_dropin::ctx(), im, width, height, &p, as_c(d_data), as_c(h_data), &numPts));
    report(CUSIFT_REPORT_READ(timer));
  }

  // legacy ExtractSift on a device-resident cuImage (main.cpp:102-103,327-328)
  void Extract(cuImage &img, float subsampling = 1.0f) {
    CUSIFT_REPORT_TIMER(timer);
    require_device("ExtractSift");
    if (img.d_data == nullptr) {
      std::printf("ExtractSift: missing data\n");
      return;
    }
    cusift_params p = params(subsampling);
    safeCall(cusift_ctx_set_keep_strongest(cusift_dropin::ctx(), keepStrongest));
    safeCall(cusift_ctx_set_second_orientation(cusift_dropin::ctx(), secondOrientation));
    safeCall(cusift_extract(cusift_dropin::ctx(), img.d_data, img.width, img.height, img.pitch, &p, as_c(d_data),
                            as_c(h_data), &numPts));
    report(CUSIFT_REPORT_READ(timer));
  }

  // New (not in the reference, which describes only what it detects): orientation + descriptor of the numPts records
  // in d_data as they stand -- an earlier Extract's, or keypoints put there by AddSiftData (debug.h): coords2D and scale
  // in image pixels -- in place and in their order, over cusift_describe_batch with this object's numOctaves, scaleUp
  // and rootSift.  flags: CUSIFT_DESCRIBE_KEEP_ORIENTATION (the records' orientations are used as they are, 0 = upright),
  // CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE (ignore the records' subsampling).  Blocking; refreshes h_data when there is one.
  void Describe(cuImage &img, unsigned flags = 0, float subsampling = 1.0f) {
    require_device("DescribeSift");
    if (img.d_data == nullptr) {
      std::printf("DescribeSift: missing data\n");
      return;
    }
    if (numPts <= 0) return;
    cusift_params p = params(subsampling);
    p.max_pts = numPts;  // one image, every record of it
    safeCall(cusift_describe_batch(cusift_dropin::ctx(), img.d_data, 1, img.width, img.height, img.pitch,
                                   (size_t)img.pitch * img.height, &p, as_c(d_data), nullptr, flags));
    safeCall(cusift_ctx_synchronize(cusift_dropin::ctx()));
    Synchronize();
  }

  // New: the second-peak stage on the numPts records in d_data as they stand (an Extract's, or Describe's) -- appends
  // the duplicates behind them, up to maxPts, over cusift_second_orientations_batch with this object's numOctaves,
  // scaleUp and rootSift, and updates numPts.  flags: CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE.  Blocking; refreshes h_data.
  void SecondOrientations(cuImage &img, float ratio = 0.8f, unsigned flags = 0, float subsampling = 1.0f) {
    require_device("SecondOrientationsSift");
    if (img.d_data == nullptr) {
      std::printf("SecondOrientationsSift: missing data\n");
      return;
    }
    if (numPts <= 0) return;
    cusift_params p = params(subsampling);
    void *d_count = nullptr;
    unsigned int count = (unsigned int)numPts;
    safeCall(cusift_malloc(&d_count, sizeof(count)));
    safeCall(cusift_memcpy_h2d(cusift_dropin::ctx(), d_count, &count, sizeof(count)));
    safeCall(cusift_second_orientations_batch(cusift_dropin::ctx(), img.d_data, 1, img.width, img.height, img.pitch,
                                              (size_t)img.pitch * img.height, &p, as_c(d_data),
                                              static_cast<unsigned int *>(d_count), ratio, flags));
    safeCall(cusift_memcpy_d2h(cusift_dropin::ctx(), &count, d_count, sizeof(count)));
    safeCall(cusift_free(d_count));
    numPts = (int)count;
    Synchronize();
  }

  // cuSIFT.cu:383-395 (always returns 0.0 like every launch wrapper of the reference)
  double ConvertSiftToRootSift() {
    if (d_data && numPts > 0) {
      safeCall(cusift_rootsift(cusift_dropin::ctx(), as_c(d_data), numPts));
      safeCall(cusift_ctx_synchronize(cusift_dropin::ctx()));
    }
    return 0.0;
  }

  // used by InitSiftData / FreeSiftData
  void allocate(int maxPts_, bool host, bool dev) {
    release();
    numPts = 0;
    maxPts = maxPts_;
    const size_t bytes = sizeof(SiftPoint) * (size_t)(maxPts_ > 0 ? maxPts_ : 0);
    if (host && bytes) h_data = static_cast<SiftPoint *>(cusift_dropin::host_alloc(bytes));
    if (dev && bytes) {
      void *ptr = nullptr;
      safeCall(cusift_malloc(&ptr, bytes));
      d_data = static_cast<SiftPoint *>(ptr);
    }
  }
  void release() {
    if (d_data != nullptr) cusift_free(d_data);
    d_data = nullptr;
    cusift_dropin::host_free(h_data);
    h_data = nullptr;
    numPts = 0;
    maxPts = 0;
  }

 private:
  static cusift_point *as_c(SiftPoint *p) { return reinterpret_cast<cusift_point *>(p); }
  cusift_params params(float subsampling) const {
    cusift_params p;
    cusift_default_params(&p);
    p.num_octaves = numOctaves;
    p.init_blur = initBlur;
    p.peak_thresh = peakThresh;
    p.edge_thresh = edgeThresh;
    p.lowest_scale = lowestScale;
    p.subsampling = subsampling;
    p.max_pts = maxPts;
    p.root_sift = rootSift ? 1 : 0;
    p.upsample = scaleUp ? 1 : 0;
    return p;
  }
  void require_device(const char *who) const {
    if (d_data == nullptr || maxPts < 1) {
      std::fprintf(stderr, "%s: SiftData has no device buffer (construct with dev = true)\n", who);
      std::exit(-1);
    }
  }
  static void report(double ms) {
#ifndef CUSIFT_QUIET
    // the reference prints this line on every call (inverted guard, cuSIFT.cu:117-119)
    std::printf("Total time incl memory =      %.2f ms\n", ms);
#else
    (void)ms;
#endif
  }
};

// ---- free functions ----------------------------------------------------------------------------------
// cuSIFT.cu:313-353
inline double ScaleDown(cuImage &res, cuImage &src, float variance) {
  if (res.d_data == nullptr || src.d_data == nullptr) {
    std::printf("ScaleDown: missing data\n");
    return 0.0;
  }
  safeCall(cusift_scale_down(cusift_dropin::ctx(), res.d_data, res.pitch, (size_t)res.pitch * res.height, src.d_data,
                             src.width, src.height, src.pitch, (size_t)src.pitch * src.height, 1, variance));
  safeCall(cusift_ctx_synchronize(cusift_dropin::ctx()));
  return 0.0;
}

// Legacy API named by the north star (signatures from main.cpp:99-103,207-211,324-328,348-349 and the
// commented bodies at cuSIFT.cu:123-134,272-303).  edgeThresh has no legacy argument: 10.0 as everywhere.
inline void InitSiftData(SiftData &data, int num, bool host, bool dev) { data.allocate(num, host, dev); }
inline void FreeSiftData(SiftData &data) { data.release(); }
// scaleUp (new, trailing, default false): SiftData::scaleUp for this call.  keepStrongest (new, trailing, 0 when left
// out): SiftData::keepStrongest for this call -- the form with it is an overload, the shorter one hands on 0.
inline void ExtractSift(SiftData &siftData, cuImage &img, int numOctaves, double initBlur, float thresh, float lowestScale,
                        float subsampling, bool scaleUp, int keepStrongest) {
  siftData.numOctaves = numOctaves;
  siftData.initBlur = initBlur;
  siftData.peakThresh = thresh;
  siftData.lowestScale = lowestScale;
  siftData.edgeThresh = 10.0f;
  siftData.rootSift = false;
  siftData.scaleUp = scaleUp;
  siftData.keepStrongest = keepStrongest;
  siftData.Extract(img, subsampling);
}
inline void ExtractSift(SiftData &siftData, cuImage &img, int numOctaves, double initBlur, float thresh,
                        float lowestScale = 0.0f, float subsampling = 1.0f, bool scaleUp = false) {
  ExtractSift(siftData, img, numOctaves, initBlur, thresh, lowestScale, subsampling, scaleUp, 0);
}
// New: SiftData::Describe in the legacy style -- descriptors for the records siftData already holds on the device.
inline void DescribeSift(SiftData &siftData, cuImage &img, int numOctaves, float subsampling = 1.0f, unsigned flags = 0) {
  siftData.numOctaves = numOctaves;
  siftData.Describe(img, flags, subsampling);
}
// New: SiftData::SecondOrientations in the legacy style -- the second-peak duplicates of the records siftData holds.
inline void SecondOrientationsSift(SiftData &siftData, cuImage &img, int numOctaves, float ratio = 0.8f,
                                   float subsampling = 1.0f, unsigned flags = 0) {
  siftData.numOctaves = numOctaves;
  siftData.SecondOrientations(img, ratio, flags, subsampling);
}
// The reference's ExtractRootSift is commented out ("TODO: bring rootsift back", cuSIFT.cu:122-134: ExtractSift,
// then ConvertSiftToRootSift, then Synchronize; its argument list lost thresh/lowestScale).  Same result in one
// pass: RootSIFT is the descriptor kernel's epilogue.
inline void ExtractRootSift(SiftData &siftData, cuImage &img, int numOctaves, double initBlur, float thresh,
                            float lowestScale = 0.0f, float subsampling = 1.0f) {
  siftData.numOctaves = numOctaves;
  siftData.initBlur = initBlur;
  siftData.peakThresh = thresh;
  siftData.lowestScale = lowestScale;
  siftData.edgeThresh = 10.0f;
  siftData.rootSift = true;
  siftData.Extract(img, subsampling);
  siftData.rootSift = false;
}

#endif  // CUSIFT_AMD_DROPIN_H
