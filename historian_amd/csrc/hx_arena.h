// The host image of a batch's inputs, as it will lie on the device: pieces put one behind the other, each at the next multiple
// of the arena's alignment, and a list of the pointer members (of job records, anywhere on the host) that shall point into
// the device copy once it has an address.  Behind the image the device allocation may hold a reserved tail: arrays with no
// host copy, which kernels fill on the device.  Host-only: no HIP here.
#pragma once
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

namespace hx {

struct Arena {
  std::vector<char> host;           // the image
  size_t reserved = 0;              // bytes of the tail
  explicit Arena(size_t alignment) : align_(alignment) {}

  // a piece of the image (src null: zeroes); returns its offset
  size_t put(const void* src, size_t bytes) {
    const size_t off = (host.size() + align_ - 1) & ~(align_ - 1);
    host.resize(off + bytes);
    if (src && bytes) memcpy(host.data() + off, src, bytes);
    return off;
  }
  size_t reserve(size_t bytes) { return put(nullptr, bytes); }
  // `member` shall point at image offset `off`
  template <class T> void point(T*& member, size_t off) { fix_.emplace_back(&member, off); }
  // n elements put, and `member` shall point at them
  template <class T> void put(T*& member, const std::remove_const_t<T>* src, size_t n) { point(member, put(src, sizeof(T) * n)); }
  // n elements of the tail (each array a multiple of 16 bytes), and `member` shall point at them
  template <class T> void reserve(T*& member, size_t n) {
    fix_tail_.emplace_back(&member, reserved);
    reserved += (sizeof(T) * n + 15) & ~(size_t)15;
  }
  // the tail begins at the image's size rounded up to 16; the device allocation holds both
  size_t tail_at() const { return (host.size() + 15) & ~(size_t)15; }
  size_t device_bytes() const { return tail_at() + reserved; }
  // the device copy lies at `base`: every registered member gets its address
  void bind(char* base) const {
    for (const auto& f : fix_) set(f.first, base + f.second);
    for (const auto& f : fix_tail_) set(f.first, base + tail_at() + f.second);
  }

 private:
  static void set(void* member, const char* p) { memcpy(member, &p, sizeof(p)); }
  size_t align_;
  std::vector<std::pair<void*, size_t>> fix_, fix_tail_;
};

}  // namespace hx
