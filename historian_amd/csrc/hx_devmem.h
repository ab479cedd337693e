// Who owns device memory, page-locked host memory and events: the three move-only types below, and nobody else.
// An object of the C ABI holds them as members; a call that needs a buffer for its own duration holds it as a local.  Either
// way the destructor releases, on every way out.  An object that must synchronise with its device first does so in its own
// destructor's body, which runs before its members' destructors.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace hx {

// live DevBuf and PinnedBuf allocations of the process: what hx_live_allocations returns (events are not counted)
inline std::atomic<int64_t> g_live_allocations{0};

// one allocation, of hipMalloc (PINNED false) or of hipHostMalloc: what DevBuf and PinnedBuf share.  Like DevEvents it can be
// move-constructed (a std::vector of owners may grow) and neither copied nor assigned: the move constructor suppresses the rest.
template <bool PINNED>
class OwnedAlloc {
 public:
  OwnedAlloc() = default;
  OwnedAlloc(OwnedAlloc&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  ~OwnedAlloc() { reset(); }
  void reset() {
    if (!p_) return;
    (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
    g_live_allocations.fetch_sub(1, std::memory_order_relaxed);
  }
  template <class T> T* as() const { return static_cast<T*>(p_); }
  explicit operator bool() const { return p_ != nullptr; }

 protected:
  // alloc() is reset(), then took(hipMalloc(&p_, ...)): a refused allocation leaves nothing held
  bool took(hipError_t rc) {
    if (rc != hipSuccess) p_ = nullptr;
    if (p_) g_live_allocations.fetch_add(1, std::memory_order_relaxed);
    return rc == hipSuccess;
  }
  void* p_ = nullptr;
};

// exactly the bytes asked for (a caller that wants an address for zero bytes asks for one byte)
struct DevBuf : OwnedAlloc<false> {
  bool alloc(size_t bytes) { reset(); return took(hipMalloc(&p_, bytes)); }
};
struct PinnedBuf : OwnedAlloc<true> {
  bool alloc(size_t bytes, unsigned flags) { reset(); return took(hipHostMalloc(&p_, bytes, flags)); }
};

// N events.  create() makes those that do not exist yet, so an object may create its events late (and ask again at no cost).
template <int N>
class DevEvents {
 public:
  DevEvents() = default;
  DevEvents(DevEvents&& o) noexcept { for (int i = 0; i < N; ++i) e_[i] = std::exchange(o.e_[i], nullptr); }
  ~DevEvents() {
    for (hipEvent_t e : e_)
      if (e) (void)hipEventDestroy(e);
  }
  bool create(unsigned flags = hipEventDefault) {
    for (hipEvent_t& e : e_)
      if (!e && hipEventCreateWithFlags(&e, flags) != hipSuccess) { e = nullptr; return false; }
    return true;
  }
  hipEvent_t operator[](int i) const { return e_[i]; }

 private:
  hipEvent_t e_[N] = {};
};

}  // namespace hx
