// sf_scratch.h -- the per-device scratch of a catalogue tool (TARP, imputation, the out-of-distribution check), host side.
// A tool owns one SfScratch; an entry point opens one SfScratchCall on it for its whole length:
//   SfScratchCall ws(g_scratch, "sf_entry_point", stream);   // takes the tool's lock
//   const int sub_a = ws.add(bytes_a), sub_b = ws.add(bytes_b);   // the layout: every sub-buffer, rounded up to 256 bytes
//   if (int rc = ws.reserve()) return rc;                    // device, event, grow, wait for the previous call
//   int32_t* a = ws.get<int32_t>(sub_a); ...                 // pointers come from the same list as the size
//   if (int rc = ws.check()) return rc;                      // a handle outside the reserved layout: an error, not an assert
//   ... launches; on a HIP error `return ws.fail(what, e);` ...
//   return ws.finish();                                      // records the event
// The list of add() calls is the only source of both the bytes requested and the pointers handed out.  From the first
// reserve() on, every way out of the scope records the slot's event on the caller's stream exactly once (finish(), or the
// destructor behind an error return), so the next call -- on whatever stream -- waits for everything this one queued.
// Two regions per slot grow independently; region 1 may be laid out again in the middle of a call (clear(1), add, reserve(1)).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "sf_internal.h"

struct SfScratch {
  std::mutex mu;
  struct Slot {
    void* p[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0};
    hipEvent_t ev = nullptr;
    bool used = false;
  } slot[SF_MAX_DEVICES];
};

class SfScratchCall {
 public:
  SfScratchCall(SfScratch& s, const char* who, hipStream_t st) : lock_(s.mu), s_(s), who_(who), st_(st) {}
  ~SfScratchCall() {
    if (armed_) (void)hipEventRecord(slot_->ev, st_);
  }
  SfScratchCall(const SfScratchCall&) = delete;
  SfScratchCall& operator=(const SfScratchCall&) = delete;

  // one more sub-buffer of the region's layout; the handle goes to get() after reserve()
  int add(size_t bytes, int region = 0) {
    Layout& l = lay_[region];
    if (l.reserved || l.n == kMaxSubs) { bad_ = true; return -1; }
    l.off[l.n + 1] = l.off[l.n] + ((bytes + 255) & ~(size_t)255);
    return region * kMaxSubs + l.n++;
  }
  void clear(int region) { lay_[region] = Layout(); }

  int reserve(int region = 0) {
    hipError_t e;
    if (bad_) return check();
    if (!slot_) {
      int dev = 0;
      e = hipGetDevice(&dev);
      if (e != hipSuccess || dev < 0 || dev >= SF_MAX_DEVICES) {
        sf_set_error(std::string(who_) + ": no usable device: " + hipGetErrorString(e));
        return SF_ERR_NO_DEVICE;
      }
      SfScratch::Slot& sl = s_.slot[dev];
      if (!sl.ev && (e = hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming)) != hipSuccess) return fail("event", e);
      slot_ = &sl;
    }
    Layout& l = lay_[region];
    void*& p = slot_->p[region];
    size_t& cap = slot_->cap[region];
    const size_t total = l.off[l.n];
    if (cap < total) {
      if (p && (e = hipFree(p)) != hipSuccess) return fail("hipFree", e);  // waits for the work that uses it
      p = nullptr;
      cap = 0;
      if ((e = hipMalloc(&p, total)) != hipSuccess) return fail("hipMalloc", e);
      cap = total;
    }
    if (!armed_) {
      if (slot_->used && (e = hipStreamWaitEvent(st_, slot_->ev, 0)) != hipSuccess) return fail("hipStreamWaitEvent", e);
      slot_->used = armed_ = true;
    }
    l.reserved = true;
    return SF_OK;
  }

  template <class T>
  T* get(int h) {
    const int region = h / kMaxSubs, i = h % kMaxSubs;
    if (h < 0 || region > 1 || !lay_[region].reserved || i >= lay_[region].n || lay_[region].off[i + 1] > slot_->cap[region]) {
      bad_ = true;
      return nullptr;
    }
    return reinterpret_cast<T*>((char*)slot_->p[region] + lay_[region].off[i]);
  }
  // after the add() / get() calls: did every one of them stay inside the layout?
  int check() {
    if (!bad_) return SF_OK;
    sf_set_error(std::string(who_) + ": scratch: a sub-buffer outside the reserved layout");
    return SF_ERR_STATE;
  }

  int fail(const char* what, hipError_t e) {
    sf_set_error(std::string(who_) + ": " + what + ": " + hipGetErrorString(e));
    return SF_ERR_HIP;
  }
  int finish() {
    armed_ = false;
    const hipError_t e = hipEventRecord(slot_->ev, st_);
    return e == hipSuccess ? SF_OK : fail("hipEventRecord", e);
  }

 private:
  static constexpr int kMaxSubs = 8;
  struct Layout {
    size_t off[kMaxSubs + 1] = {0};   // off[i] .. off[i + 1]: sub-buffer i; off[n]: the bytes the region needs
    int n = 0;
    bool reserved = false;
  };
  std::lock_guard<std::mutex> lock_;
  SfScratch& s_;
  const char* who_;
  hipStream_t st_;
  SfScratch::Slot* slot_ = nullptr;
  Layout lay_[2];
  bool armed_ = false, bad_ = false;
};
