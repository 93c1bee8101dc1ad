// hmpc_device_buffer.h -- the two owner types of the device memory a handle holds (hmpc_handle.h).  Errors come back as hipError_t: what
// to make of one (HIP_TRY, the error text) is the caller's business.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

// One hipMalloc allocation and its size in bytes.  Move-only; the destructor frees.  (Hidden, like OutputBuffer: the types are no part of
// the library's ABI.)
template <class T>
class __attribute__((visibility("hidden"))) DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer &) = delete;
  DeviceBuffer &operator=(const DeviceBuffer &) = delete;
  DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr, o.bytes_ = 0; }
  DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, bytes_ = o.bytes_;
      o.p_ = nullptr, o.bytes_ = 0;
    }
    return *this;
  }
  ~DeviceBuffer() { reset(); }

  T *get() const { return p_; }
  size_t bytes() const { return bytes_; }

  // frees at once: only for a buffer nothing enqueued can still be using (reserve() is the one that waits)
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr, bytes_ = 0;
  }

  // `count` elements, contents undefined; whatever the object held before is freed first (see reset)
  hipError_t alloc(size_t count) {
    reset();
    const hipError_t e = hipMalloc((void **)&p_, count * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    else bytes_ = count * sizeof(T);
    return e;
  }

  // `count` elements with every byte set to `byte`.  The object holds the buffer only if allocation AND fill succeeded: a reader never
  // meets a buffer that exists but was not filled.
  hipError_t alloc_filled(size_t count, int byte) {
    hipError_t e = alloc(count);
    if (e == hipSuccess && bytes_ > 0 && (e = hipMemset(p_, byte, bytes_)) != hipSuccess) reset();
    return e;
  }

  // grows to at least `bytes` (contents undefined).  The old allocation is freed only once nothing can still be using it: its users' stream
  // is synchronised first, or the whole device when they may be on any stream (whole_device).
  hipError_t reserve(size_t bytes, hipStream_t stream, bool whole_device) {
    if (p_ && bytes <= bytes_) return hipSuccess;
    if (p_) {
      hipError_t e = whole_device ? hipDeviceSynchronize() : hipStreamSynchronize(stream);
      if (e != hipSuccess) return e;
      e = hipFree(p_);
      p_ = nullptr, bytes_ = 0;
      if (e != hipSuccess) return e;
    }
    const hipError_t e = hipMalloc((void **)&p_, bytes);
    if (e != hipSuccess) p_ = nullptr;
    else bytes_ = bytes;
    return e;
  }

 private:
  T *p_ = nullptr;
  size_t bytes_ = 0;
};

// Where an output goes: the caller's buffer while one is set, else the handle's own, allocated on first need.
template <class T>
class __attribute__((visibility("hidden"))) OutputBuffer {
 public:
  void set_caller(T *p) { caller_ = p; }  // nullptr = the handle's own
  hipError_t ensure(size_t count) { return (caller_ || own_.get()) ? hipSuccess : own_.alloc(count); }
  T *get() const { return caller_ ? caller_ : own_.get(); }

 private:
  DeviceBuffer<T> own_;
  T *caller_ = nullptr;
};
