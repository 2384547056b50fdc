// smr_devbuf.hpp -- host only: what the engine owns on the device.  DevBuf<T> is a device array that frees itself (movable, not copyable;
// converts to T* where a kernel argument or a copy wants the pointer), DevStream a HIP stream.  A struct made of them needs no free list:
// deleting the context, dropping an index slot or leaving the scope of a throw-away batch releases exactly what was allocated.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

struct smr_ctx;
int dev_fail(smr_ctx* c, const char* call, hipError_t e);      // the context's error := "<call>: <HIP's message>" (smr_engine.hip); returns SMR_ERR_DEVICE

template <class T> class DevBuf {
  T* p_ = nullptr;
  size_t cap_ = 0;              // elements

 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  ~DevBuf() { release(); }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t cap() const { return cap_; }

  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr; cap_ = 0;
  }
  // exactly `count` elements (at least one), whatever is there now; the contents are not kept
  int alloc(smr_ctx* c, size_t count) {
    release();
    if (count == 0) count = 1;
    const hipError_t e = hipMalloc((void**)&p_, count * sizeof(T));
    if (e != hipSuccess) { p_ = nullptr; return dev_fail(c, "hipMalloc", e); }
    cap_ = count;
    return 0;
  }
  // the same for a buffer the caller can do without: false when the device has no room (no error is set; the buffer is empty then)
  bool try_alloc(size_t count) {
    release();
    if (count == 0) count = 1;
    if (hipMalloc((void**)&p_, count * sizeof(T)) != hipSuccess) { p_ = nullptr; (void)hipGetLastError(); return false; }
    cap_ = count;
    return true;
  }
  // grow-only: a new array when this one holds fewer than `need` elements
  int reserve(smr_ctx* c, size_t need) { return (p_ && cap_ >= need) ? 0 : alloc(c, need); }
  // a staging buffer for `total` elements of which a kernel may touch `slack` more: when it is too small, a new one with an eighth to spare,
  // rounded up to 4 Ki elements (the next, slightly larger call fits as well)
  int reserve_headroom(smr_ctx* c, size_t total, size_t slack) {
    return cap_ >= total + slack ? 0 : alloc(c, (size_t)((total + (total >> 3) + 4095u) & ~4095ull));
  }
};

struct DevStream {
  hipStream_t s = nullptr;
  DevStream() = default;
  DevStream(const DevStream&) = delete;
  DevStream& operator=(const DevStream&) = delete;
  ~DevStream() { if (s) (void)hipStreamDestroy(s); }
  operator hipStream_t() const { return s; }
};
