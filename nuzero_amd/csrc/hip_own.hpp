// Host-only owners of HIP resources: a device block, a page-locked host block, an event, a stream.  Move-only; each
// frees what it holds in its destructor, so a handle that keeps them as members needs no free list.  A lifecycle group
// is a struct of these with one all-or-nothing ensure(); kernel argument structs only borrow their get() pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <utility>

namespace nz {

template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
  DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }   // (o frees the old block)
  ~DevBuf() { reset(); }
  T* get() const { return p_; }
  size_t size() const { return n_; }            // elements
  // at least n elements: the block it has if that is enough, else a new one (the contents are NOT carried over);
  // false, and empty, when the allocation fails
  bool ensure(size_t n) {
    if (n <= n_) return true;
    reset();
    if (hipMalloc((void**)&p_, n * sizeof(T)) == hipSuccess) n_ = n; else p_ = nullptr;
    return p_ != nullptr;
  }
  void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// the same over page-locked host memory (read-backs and uploads of the move loops: from pageable memory every copy is staged)
template <typename T>
class PinnedBuf {
 public:
  PinnedBuf() = default;
  PinnedBuf(PinnedBuf&& o) noexcept { *this = std::move(o); }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }
  ~PinnedBuf() { reset(); }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  T& operator[](size_t i) const { return p_[i]; }
  bool ensure(size_t n) {
    if (n <= n_) return true;
    reset();
    if (hipHostMalloc((void**)&p_, n * sizeof(T), hipHostMallocDefault) == hipSuccess) n_ = n; else p_ = nullptr;
    return p_ != nullptr;
  }
  void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; n_ = 0; }
 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept { *this = std::move(o); }
  Event& operator=(Event&& o) noexcept { std::swap(e_, o.e_); return *this; }
  ~Event() { if (e_) (void)hipEventDestroy(e_); }
  hipEvent_t get() const { return e_; }
  bool create(unsigned flags = hipEventDefault) {         // on first use; true when there is an event
    if (!e_ && hipEventCreateWithFlags(&e_, flags) != hipSuccess) e_ = nullptr;
    return e_ != nullptr;
  }
 private:
  hipEvent_t e_ = nullptr;
};

class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept { *this = std::move(o); }
  Stream& operator=(Stream&& o) noexcept { std::swap(s_, o.s_); return *this; }
  ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
  hipStream_t get() const { return s_; }
  bool create(unsigned flags = hipStreamDefault) {
    if (!s_ && hipStreamCreateWithFlags(&s_, flags) != hipSuccess) s_ = nullptr;
    return s_ != nullptr;
  }
 private:
  hipStream_t s_ = nullptr;
};

}  // namespace nz
