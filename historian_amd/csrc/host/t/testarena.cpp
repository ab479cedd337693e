// The staging arena of the batches (csrc/hx_arena.h), stand-alone: no device, no library.  For both alignments the batches use
// (256: pair-fill and guide-alignment batches; 16: branch and sibling batches) a sequence of pieces - sizes around the
// alignments, an empty piece, a piece without a source - is put; every offset is checked against the closed formula, the
// image against the bytes put, and bind() against base + offset for the image's and the reserved tail's members alike.
// `make sanitize` builds and runs it under AddressSanitizer and UBSan.  Returns the number of failures.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../hx_arena.h"

static int failures = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) { ++failures; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

static void arenaCases(const size_t a) {
  hx::Arena ar(a);
  const size_t sizes[] = {1, 15, 16, 17, 0, 255, 256, 257, 1, 0, 16};
  const size_t n = sizeof(sizes) / sizeof(sizes[0]), no_source = 3;      // (piece 3, 17 bytes, is put without a source)
  std::vector<std::vector<unsigned char>> src(n);
  std::vector<size_t> off(n);
  std::vector<const unsigned char*> member(n, nullptr);
  size_t end = 0;
  for (size_t k = 0; k < n; ++k) {
    src[k].resize(sizes[k]);
    for (size_t i = 0; i < sizes[k]; ++i) src[k][i] = (unsigned char)(1 + (37 * k + 11 * i) % 255);      // (never 0)
    // the three ways in: an offset, an offset for a piece without a source, a member that shall point at the piece
    if (k == no_source) off[k] = ar.put(nullptr, sizes[k]);
    else if (k % 2) off[k] = ar.put(src[k].data(), sizes[k]);
    else {
      ar.put(member[k], src[k].data(), sizes[k]);
      off[k] = ar.host.size() - sizes[k];
    }
    EXPECT(off[k] == ((end + a - 1) & ~(a - 1)));
    end = off[k] + sizes[k];
    EXPECT(ar.host.size() == end);
  }
  // reserve: a piece of zeroes in the image; point: a member at an offset of the caller's choosing
  const size_t r = ar.reserve(24);
  EXPECT(r == ((end + a - 1) & ~(a - 1)) && ar.host.size() == r + 24);
  const double* at_reserve = nullptr;
  ar.point(at_reserve, r);
  for (size_t k = 0; k < n; ++k)
    for (size_t i = 0; i < sizes[k]; ++i) EXPECT((unsigned char)ar.host[off[k] + i] == (k == no_source ? 0 : src[k][i]));
  for (size_t i = 0; i < 24; ++i) EXPECT(ar.host[r + i] == 0);
  for (size_t k = 0; k + 1 < n; ++k)       // padding between the pieces is zero as well
    for (size_t i = off[k] + sizes[k]; i < off[k + 1]; ++i) EXPECT(ar.host[i] == 0);
  // the reserved tail: arrays in multiples of 16 bytes, from the image's size rounded up to 16
  const double *t0 = nullptr, *t3 = nullptr;
  const int32_t* t1 = nullptr;
  unsigned char* t2 = nullptr;
  ar.reserve(t0, 3);       // 24 -> 32 bytes
  ar.reserve(t1, 0);       // none
  ar.reserve(t2, 17);      // 17 -> 32
  ar.reserve(t3, 2);       // 16
  EXPECT(ar.reserved == 80);
  const size_t image = ar.host.size();
  EXPECT(ar.tail_at() == ((image + 15) & ~(size_t)15));
  EXPECT(ar.device_bytes() == ar.tail_at() + 80);
  // bind: nothing is read through the base, so any address will do
  char* const base = reinterpret_cast<char*>((uintptr_t)0x7000000000ull);
  ar.bind(base);
  for (size_t k = 0; k < n; ++k)
    EXPECT(reinterpret_cast<const char*>(member[k]) == (k == no_source || k % 2 ? nullptr : base + off[k]));
  EXPECT(reinterpret_cast<const char*>(at_reserve) == base + r);
  char* const tail = base + ar.tail_at();
  EXPECT(reinterpret_cast<const char*>(t0) == tail);
  EXPECT(reinterpret_cast<const char*>(t1) == tail + 32);
  EXPECT(reinterpret_cast<char*>(t2) == tail + 32);
  EXPECT(reinterpret_cast<const char*>(t3) == tail + 64);
  printf("alignment %zu: image of %zu bytes, tail at %zu, %d failures so far\n", a, image, ar.tail_at(), failures);
}

int main() {
  arenaCases(256);
  arenaCases(16);
  printf("testarena: %d failures\n", failures);
  return failures;
}
