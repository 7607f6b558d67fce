// Host-side helpers shared by the C-ABI sources: error plumbing, device arrays owned by their handle, kernel attributes.
// Host code only: nothing here is compiled for the device.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "../../include/vrag_amd.h"

namespace vrag {

void set_error(const char* fmt, ...);   // csrc/capi.hip: the message vrag_last_error() returns on this thread

}  // namespace vrag

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess) {                                                                 \
      vrag::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
      return VRAG_ERR_HIP;                                                                  \
    }                                                                                       \
  } while (0)
#define ARG_CHECK(cond, ...)         \
  do {                               \
    if (!(cond)) {                   \
      vrag::set_error(__VA_ARGS__);  \
      return VRAG_ERR_INVALID;       \
    }                                \
  } while (0)
// The entry points that take a device index: one that is not visible is refused (a negative index is each caller's own check).
#define DEVICE_CHECK(device)                                                         \
  do {                                                                               \
    if (vrag_device_count() <= (device)) {                                           \
      vrag::set_error("no HIP device %d visible (no CPU fallback)", (int)(device));  \
      return VRAG_ERR_NO_DEVICE;                                                     \
    }                                                                                \
  } while (0)

namespace vrag {

// Records `ev` on `st`; the event (no timing) is created on its first use.  The handles' upload_done / lists_done events.
inline hipError_t record_event(hipEvent_t& ev, hipStream_t st) {
  if (!ev) {
    const hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  return hipEventRecord(ev, st);
}

// Device array of T owned by its holder (scratch of an index handle, weights and workspace of an encoder): freed with it.
template <typename T>
struct DevArray {
  T* p = nullptr;
  size_t n = 0;   // elements allocated
  DevArray() = default;
  DevArray(const DevArray&) = delete;
  DevArray& operator=(const DevArray&) = delete;
  DevArray(DevArray&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  DevArray& operator=(DevArray&& o) noexcept {   // frees what this array held
    if (this != &o) {
      if (p) (void)hipFree(p);
      p = o.p, n = o.n;
      o.p = nullptr, o.n = 0;
    }
    return *this;
  }
  ~DevArray() {
    if (p) (void)hipFree(p);
  }
  // At least `need` elements: a no-op when the array is large enough, else the old allocation is freed and exactly `need`
  // elements are allocated.  Contents undefined after a reallocation.
  hipError_t grow(size_t need) {
    if (need <= n) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), need * sizeof(T));
    if (e == hipSuccess) n = need;
    else p = nullptr;
    return e;
  }
};

// dst = src on stream st; an empty src still leaves a valid one-element allocation.
template <typename T>
hipError_t upload(DevArray<T>& dst, const std::vector<T>& src, hipStream_t st) {
  hipError_t e = dst.grow(std::max<size_t>(src.size(), 1));
  if (e == hipSuccess && !src.empty()) e = hipMemcpyAsync(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, st);
  return e;
}

// Pinned host array of T owned by its holder (staging buffers of a handle): DevArray's shape over hipHostMalloc / hipHostFree.
template <typename T>
struct PinnedArray {
  T* p = nullptr;
  size_t n = 0;   // elements allocated
  PinnedArray() = default;
  PinnedArray(const PinnedArray&) = delete;
  PinnedArray& operator=(const PinnedArray&) = delete;
  PinnedArray(PinnedArray&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
  PinnedArray& operator=(PinnedArray&& o) noexcept {   // frees what this array held
    if (this != &o) {
      if (p) (void)hipHostFree(p);
      p = o.p, n = o.n;
      o.p = nullptr, o.n = 0;
    }
    return *this;
  }
  ~PinnedArray() {
    if (p) (void)hipHostFree(p);
  }
  // As DevArray::grow, with the hipHostMalloc flags of the new allocation (hipHostMallocMapped: a device-visible word).
  hipError_t grow(size_t need, unsigned flags = hipHostMallocDefault) {
    if (need <= n) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), need * sizeof(T), flags);
    if (e == hipSuccess) n = need;
    else p = nullptr;
    return e;
  }
};

// Untyped device allocation freed with its owner (temporaries of one call; growable buffers of a handle).  Unlike DevArray, every
// alloc() starts afresh, empty arrays still get a valid pointer, and reserve() grows with headroom.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p, bytes = o.bytes;
      o.p = nullptr, o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  hipError_t alloc(size_t n) {   // fresh contents; at least 16 bytes so that empty arrays are valid pointers
    reset();
    n = std::max<size_t>(n, 16);
    hipError_t e = hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    else p = nullptr;
    return e;
  }
  hipError_t reserve(size_t n) { return n <= bytes ? hipSuccess : alloc(n + n / 2); }   // contents not kept
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Raises the dynamic-LDS limit of one kernel instantiation to `bytes` on its first launch in the process.  Thread-safe (handles
// behind different mutexes launch the same kernels); a failed call is returned to the caller and tried again on the next launch.
template <auto Kernel>
hipError_t set_max_dynamic_lds(int bytes) {
  static std::atomic<bool> done{false};
  static std::mutex mu;
  if (done.load(std::memory_order_acquire)) return hipSuccess;
  std::lock_guard<std::mutex> lk(mu);
  if (done.load(std::memory_order_relaxed)) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.store(true, std::memory_order_release);
  return e;
}

}  // namespace vrag
