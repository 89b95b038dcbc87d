// Library-wide host code of libfsem: nothing here belongs to one metric, and there are no kernels.
//   side_stream, stream_wait, cu_count   per-device helpers of the launchers (fsem_internal.h)
//   fsem_strerror, fsem_version, fsem_build_id, fsem_host_buffer_mapped   (include/fsem.h)
//   the build-id and build-arch markers the host layer reads from the file (_build.py)
#include <atomic>
#include <mutex>

#include "fsem_build_marker.h"
#include "fsem_internal.h"

using namespace fsem;

namespace {
constexpr int kMaxDev = 64;  // devices the per-device tables below cover

// The join events of one host thread, one per device, released when the thread exits
// (errors ignored: at process exit the runtime may already be gone).
struct ThreadEvents {
  hipEvent_t ev[kMaxDev] = {};
  ~ThreadEvents() {
    for (hipEvent_t &e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};
}  // namespace

hipStream_t fsem::side_stream(hipStream_t st) {
  static std::mutex mu;
  static hipStream_t side[kMaxDev] = {};
  int cur = 0;
  hipDevice_t dev = 0;
  if (hipGetDevice(&cur) != hipSuccess || hipStreamGetDevice(st, &dev) != hipSuccess) return st;
  // created on the current device only; a stream of another device keeps its work on one stream
  if (dev != cur || dev < 0 || dev >= kMaxDev) return st;
  std::lock_guard<std::mutex> lock(mu);
  if (!side[dev] && hipStreamCreateWithFlags(&side[dev], hipStreamNonBlocking) != hipSuccess) {
    side[dev] = nullptr;
    return st;
  }
  return side[dev];
}

int fsem::stream_wait(hipStream_t waiter, hipStream_t producer) {
  if (waiter == producer) return FSEM_OK;
  // One event per (host thread, device), recorded anew for every edge.  This relies on the
  // HIP (as CUDA) snapshot semantics of hipStreamWaitEvent: a wait waits for the record that is
  // the event's most recent one WHEN THE WAIT IS ENQUEUED, so re-recording the event for the
  // next edge (possibly on another stream) does not move an earlier wait.  No other thread
  // records this event.
  thread_local ThreadEvents tev;
  hipEvent_t *ev = tev.ev;
  hipDevice_t dev = 0;
  if (hipStreamGetDevice(producer, &dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return FSEM_ELAUNCH;
  if (!ev[dev]) {
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return FSEM_ELAUNCH;
    if (cur != dev && hipSetDevice(dev) != hipSuccess) return FSEM_ELAUNCH;
    const bool made = hipEventCreateWithFlags(&ev[dev], hipEventDisableTiming) == hipSuccess;
    if (cur != dev) (void)hipSetDevice(cur);
    if (!made) {
      ev[dev] = nullptr;
      return FSEM_ELAUNCH;
    }
  }
  const bool ok = hipEventRecord(ev[dev], producer) == hipSuccess && hipStreamWaitEvent(waiter, ev[dev], 0) == hipSuccess;
  return ok ? FSEM_OK : FSEM_ELAUNCH;
}

int fsem::cu_count() {
  static std::atomic<int> cache[kMaxDev];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDev) return 256;
  int n = cache[dev].load(std::memory_order_relaxed);
  if (n > 0) return n;
  n = 256;
  (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
  cache[dev].store(n, std::memory_order_relaxed);
  return n;
}

extern "C" const char *fsem_strerror(int code) {
  switch (code) {
    case FSEM_OK: return "ok";
    case FSEM_EINVAL: return "invalid argument";
    case FSEM_EWORKSPACE: return "workspace too small";
    case FSEM_ELAUNCH: return "HIP launch failed";
    case FSEM_ESHORT: return "input too short for the metric";
    case FSEM_ERATE: return "unsupported sample-rate pair";
    default: return "unknown error";
  }
}

extern "C" int fsem_version(void) { return 11; }  // 11: + fsem_sdr_*; 10: + fsem_pesq_wb_frames_f32; 9: + fsem_pesq_bad_intervals_*, fsem_pesq_pool_f32; 8: + fsem_time_align_p862_*; 7: + fsem_host_buffer_mapped; 6: + fsem_build_id; 5: + fsem_time_align_utt_*; 4: + fsem_pre_emphasize_f32; 3: + fsem_time_align_*, fsem_pesq_distances_*

// The build's content hash, without the marker's prefix (fsem_build_marker.h).
extern "C" const char *fsem_build_id(void) { return kBuildIdMarker + kBuildIdPrefix; }

// The drop-in call's scores go straight into its pinned host buffer when the runtime maps that
// buffer into the device address space at the same address (hipHostMalloc memory on ROCm).
extern "C" int fsem_host_buffer_mapped(const void *p) {
  if (!p) return 0;
  void *d = nullptr;
  if (hipHostGetDevicePointer(&d, const_cast<void *>(p), 0) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return d == p ? 1 : 0;
}
