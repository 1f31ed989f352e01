// sf_buf.h -- the owners of a handle's device memory, pinned memory and events (host side only).
//
// Every d_* / h_* member of a handle (sf_flow, SfNsfAr, SfNsf1, sf_mlp, sf_opt) is one of the three types below: the member IS its
// free, so destroying a handle is `delete`, and a group of buffers that is built all-or-nothing is built in a local struct and
// moved into the handle at the end -- a failure part-way returns, and the local frees what it took.
// Kernel argument structs keep raw pointers (get() or the implicit conversion).  Three rules:
//   * grow() frees BEFORE it allocates (peak memory is the new size, not old + new), to exactly the size asked for;
//   * the free is plain hipFree, whose implicit device synchronisation is what lets a buffer go while kernels that read it
//     may still be queued -- no hipFreeAsync, no pool;
//   * no owner has static storage.  Objects that live until process exit (the `static d_tr` trace buffers, the pinned staging
//     of sf_hostio.hip, the tools' SfScratch) keep raw pointers and are never freed: a destructor that calls into HIP after the
//     runtime has been torn down crashes at interpreter exit.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

// The runtime function an owner called last on this thread.  The message of a failed owner operation is "<expression>: <runtime
// function>: <hip error>" (sf_hip_message, sf_internal.h): the expression alone would name only the member function.
inline const char*& sf_buf_last_call() {
  static thread_local const char* fn = "";
  return fn;
}

template <class T>
class SfBuf {
 public:
  SfBuf() = default;
  SfBuf(SfBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
  SfBuf& operator=(SfBuf&& o) noexcept {
    if (this != &o) { (void)reset(); p_ = std::exchange(o.p_, nullptr); cap_ = std::exchange(o.cap_, 0); }
    return *this;
  }
  ~SfBuf() { (void)reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }
  size_t cap() const { return cap_; }   // elements
  hipError_t reset() {
    if (!p_) return hipSuccess;
    T* p = std::exchange(p_, nullptr);
    cap_ = 0;
    sf_buf_last_call() = "hipFree";
    return hipFree(p);
  }
  hipError_t alloc(size_t n) {
    sf_buf_last_call() = "hipMalloc";
    if (p_) return hipErrorInvalidValue;   // (an owner is never allocated over)
    hipError_t e = hipMalloc(&p_, n * sizeof(T));
    if (e == hipSuccess) cap_ = n;
    else p_ = nullptr;
    return e;
  }
  hipError_t grow(size_t n) {
    if (cap_ >= n) return hipSuccess;
    hipError_t e = reset();
    return e == hipSuccess ? alloc(n) : e;
  }
  hipError_t upload(const std::vector<T>& v) {   // blocking copy: in place before anything is queued on any stream
    hipError_t e = alloc(v.size());
    if (e != hipSuccess) return e;
    sf_buf_last_call() = "hipMemcpy";
    return hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

template <class T>
class SfPinned {
 public:
  SfPinned() = default;
  SfPinned(SfPinned&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  SfPinned& operator=(SfPinned&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); }
    return *this;
  }
  ~SfPinned() { reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }
  void reset() { if (p_) (void)hipHostFree(std::exchange(p_, nullptr)); }
  hipError_t alloc(size_t n) {
    sf_buf_last_call() = "hipHostMalloc";
    if (p_) return hipErrorInvalidValue;
    hipError_t e = hipHostMalloc((void**)&p_, n * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }

 private:
  T* p_ = nullptr;
};

class SfEvent {
 public:
  SfEvent() = default;
  SfEvent(SfEvent&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  SfEvent& operator=(SfEvent&& o) noexcept {
    if (this != &o) { reset(); e_ = std::exchange(o.e_, nullptr); }
    return *this;
  }
  ~SfEvent() { reset(); }
  hipEvent_t get() const { return e_; }
  operator hipEvent_t() const { return e_; }
  void reset() { if (e_) (void)hipEventDestroy(std::exchange(e_, nullptr)); }
  hipError_t create() {   // on demand: a no-op once it exists
    if (e_) return hipSuccess;
    sf_buf_last_call() = "hipEventCreate";
    return hipEventCreate(&e_);
  }

 private:
  hipEvent_t e_ = nullptr;
};
