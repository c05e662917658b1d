// Sub-buffers of one device buffer, sized by the same take() calls that carve it.  HIP-free (like host_logic.h), so that
// tests/host_sanitize/ compiles exactly this code with g++ -fsanitize=address,undefined.
#pragma once
#include <cstddef>

namespace sc_host {

// A layout is a function of an Arena that take()s its buffers and does nothing else.  Run on a measuring arena (no base) it
// yields the bytes it needs; run again on a buffer of that many bytes it yields the pointers (api_internal.h:
// carve_scratch).  Every region starts on a 256-byte boundary.  A region of no elements still occupies one byte, so its
// address is valid and no other region's: kernels may be handed the pointer of an empty table.
class Arena {
 public:
  Arena() = default;                                                        // measures
  Arena(void* base, size_t capacity) : base_((char*)base), cap_(capacity) {}  // carves
  template <typename T>
  T* take(size_t count) {
    const size_t at = (off_ + 255) / 256 * 256;
    const size_t bytes = count ? count * sizeof(T) : 1;
    off_ = at + bytes;
    if (!base_) return nullptr;
    if (off_ > cap_) {   // the layout took more than it measured: the caller gets no pointer to write through
      overrun_ = true;
      return nullptr;
    }
    return reinterpret_cast<T*>(base_ + at);
  }
  size_t bytes() const { return off_; }
  bool overrun() const { return overrun_; }

 private:
  char* base_ = nullptr;
  size_t cap_ = 0, off_ = 0;
  bool overrun_ = false;
};

}  // namespace sc_host
