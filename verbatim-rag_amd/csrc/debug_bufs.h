// Device staging of the unit-test hooks (include/vrag_amd_debug.h): the one place where a hook's host buffers become device
// copies with a canary behind each, and where the canaries are checked after the launches.  Host code of the harness library
// only (libvrag_amd_dbg.so): included by debug_api.hip and by the VRAG_DEBUG_API region of fulltext.hip.
#pragma once
#include <algorithm>
#include <deque>
#include <vector>

#include "host_util.h"

namespace vrag {

// The device a hook runs on: called after every argument check and before anything is allocated.
inline int use_device(int device) {
  if (vrag_device_count() <= device) {
    set_error("no HIP device %d visible", device);
    return VRAG_ERR_NO_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
  return VRAG_OK;
}

// p + offset where p is there; an optional buffer that is absent stays a null pointer.
template <typename T>
T* at(T* p, size_t offset) { return p ? p + offset : nullptr; }

// Device copies of a hook's buffers.  Each is [data | pad zero bytes | 4 KiB of 0xA5] in an allocation of its own; the launches
// must leave every canary as it was.  The first failure of a staging call sticks in `err` and the later ones do nothing.
struct DbgBufs {
  static constexpr size_t kCanary = 4096;
  static constexpr unsigned char kCanaryByte = 0xA5;
  struct B {
    void* host_out;   // null = nothing is copied back
    size_t bytes;     // the data: from the host (or zeros), copied back to host_out
    size_t pad;       // zero bytes a kernel may read behind the data, in front of the canary; never copied back
    const char* name;
    DevBuf dev;
  };
  std::deque<B> bufs;
  hipError_t err = hipSuccess;
  const unsigned* sat = nullptr;   // clamp_word()
  int32_t* sat_out = nullptr;

  template <typename T>
  T* add(const void* host, void* host_out, size_t count, const char* name, size_t pad) {
    const size_t bytes = count * sizeof(T);
    bufs.push_back(B{host_out, bytes, pad, name, DevBuf()});
    B& b = bufs.back();
    if (err == hipSuccess) err = b.dev.alloc(bytes + pad + kCanary);
    if (err == hipSuccess && bytes) err = host ? hipMemcpy(b.dev.p, host, bytes, hipMemcpyHostToDevice) : hipMemset(b.dev.p, 0, bytes);
    if (err == hipSuccess && pad) err = hipMemset(b.dev.as<char>() + bytes, 0, pad);
    if (err == hipSuccess) err = hipMemset(b.dev.as<char>() + bytes + pad, kCanaryByte, kCanary);
    return b.dev.as<T>();
  }
  // A mandatory buffer of `count` elements of T: an empty one is still a valid device pointer.  in: copied to the device;
  // inout: also copied back by finish(); scratch: zeros, the hook's own.
  template <typename T>
  T* in(const void* host, size_t count, const char* name, size_t pad_bytes = 0) { return add<T>(host, nullptr, count, name, pad_bytes); }
  template <typename T>
  T* inout(void* host, size_t count, const char* name, size_t pad_bytes = 0) { return add<T>(host, host, count, name, pad_bytes); }
  template <typename T>
  T* scratch(size_t count, const char* name, size_t pad_bytes = 0) { return add<T>(nullptr, nullptr, count, name, pad_bytes); }
  // An optional buffer: a null host pointer stages nothing and reaches the launcher as a null pointer.
  template <typename T>
  T* in_opt(const void* host, size_t count, const char* name) { return host ? in<T>(host, count, name) : nullptr; }
  template <typename T>
  T* inout_opt(void* host, size_t count, const char* name) { return host ? inout<T>(host, count, name) : nullptr; }
  // The launch's fp16 clamp word, zeroed; finish() reports it in *f16_saturated (0 / 1).
  unsigned* clamp_word(int32_t* f16_saturated) {
    sat_out = f16_saturated;
    unsigned* w = scratch<unsigned>(1, "f16_sat");
    sat = w;
    return w;
  }
  // Before the first launch: everything staged so far is on the device.
  hipError_t staged() {
    if (err == hipSuccess) err = hipDeviceSynchronize();
    return err;
  }
  // After the launches (e = their status): synchronises, checks every canary in staging order and copies the in / out buffers
  // back, unless a HIP call failed.  `hook` names the hook in the message.
  int finish(const char* hook, hipError_t e) {
    if (e == hipSuccess) e = hipDeviceSynchronize();
    unsigned saturated = 0;
    if (e == hipSuccess && sat) e = hipMemcpy(&saturated, sat, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && sat) *sat_out = saturated ? 1 : 0;
    std::vector<unsigned char> canary(kCanary);
    const char* clobbered = nullptr;
    for (B& b : bufs) {
      if (e != hipSuccess) break;
      e = hipMemcpy(canary.data(), b.dev.as<char>() + b.bytes + b.pad, kCanary, hipMemcpyDeviceToHost);
      if (e == hipSuccess && !clobbered && !std::all_of(canary.begin(), canary.end(), [](unsigned char v) { return v == kCanaryByte; }))
        clobbered = b.name;
      if (e == hipSuccess && b.host_out && b.bytes) e = hipMemcpy(b.host_out, b.dev.p, b.bytes, hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) {
      set_error("debug %s run failed: %s", hook, hipGetErrorString(e));
      return VRAG_ERR_HIP;
    }
    if (clobbered) {
      set_error("debug %s run: the launch wrote past the end of %s", hook, clobbered);
      return VRAG_ERR_HIP;
    }
    return VRAG_OK;
  }
};

}  // namespace vrag
