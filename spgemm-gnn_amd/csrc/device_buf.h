// Owning device allocation: the pointer and its byte size, freed in the destructor.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

namespace maxk {

// MAXK_PLAN_MALLOC=contiguous (read once): see DeviceBuf::alloc.
__attribute__((visibility("hidden"))) inline bool plan_malloc_contiguous() {
  static const bool on = [] {
    const char* e = std::getenv("MAXK_PLAN_MALLOC");
    return e && std::strcmp(e, "contiguous") == 0;
  }();
  return on;
}

// Move-only. Converts to T*, so a buffer stands wherever the raw pointer stood: as a kernel
// argument, in a boolean test, in pointer arithmetic. Not part of the library's exported
// symbols.
template <class T>
class __attribute__((visibility("hidden"))) DeviceBuf {
 public:
  DeviceBuf() = default;
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;
  DeviceBuf(DeviceBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) {
    o.p_ = nullptr;
    o.bytes_ = 0;
  }
  DeviceBuf& operator=(DeviceBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      bytes_ = o.bytes_;
      o.p_ = nullptr;
      o.bytes_ = 0;
    }
    return *this;
  }
  ~DeviceBuf() { reset(); }

  // `count` elements (what was held is freed first). streamed: one of the large streamed plan
  // arrays (forward edge words, backward records), for which MAXK_PLAN_MALLOC=contiguous asks
  // the runtime for physically contiguous memory (hipDeviceMallocContiguous), falling back to
  // hipMalloc when it cannot (round 6 experiment on allocation-dependent kernel times, DESIGN
  // §7). Only that refused attempt's error is cleared: an error pending from an earlier launch
  // stays for the caller's next check.
  hipError_t alloc(size_t count, bool streamed = false) {
    reset();
    const size_t bytes = count * sizeof(T);
    void* q = nullptr;
    if (streamed && plan_malloc_contiguous()) {
      if (hipExtMallocWithFlags(&q, bytes, hipDeviceMallocContiguous) != hipSuccess) {
        (void)hipGetLastError();
        q = nullptr;
      }
    }
    if (!q) {
      const hipError_t e = hipMalloc(&q, bytes);
      if (e != hipSuccess) return e;
    }
    p_ = static_cast<T*>(q);
    bytes_ = bytes;
    return hipSuccess;
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    bytes_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t bytes() const { return bytes_; }

 private:
  T* p_ = nullptr;
  size_t bytes_ = 0;
};

}  // namespace maxk
