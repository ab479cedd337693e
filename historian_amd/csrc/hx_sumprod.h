// What the column sum-product kernels share (hx_sumprod.hip: counts; hx_ancestors.hip: node posteriors): the
// constant-address-space view of the model's matrices, the LDS matrix-vector product, the reference's rescaling
// threshold, the device buffer guard and the time of the last call's kernels.
#pragma once
#include <hip/hip_runtime.h>
#include "hx_policy.h"

namespace hx {

#define HX_SP_RESCALE 1e-30        // SUMPROD_RESCALE_THRESHOLD (src/sumprod.cpp:8)

// Model matrices are read through the constant address space: their addresses are uniform over the wavefront and
// nothing writes them, so the compiler fetches them with scalar loads and feeds the FMAs from SGPRs.
typedef const __attribute__((address_space(4))) double* CMat;
__device__ __forceinline__ CMat cmat(const double* p) { return (CMat)(unsigned long long)p; }

// Matrix-vector products with a matrix that a wave keeps in LDS (row-major, A x A, 16-byte aligned rows: A even).  Every
// lane reads the same entries (broadcast reads, two entries per ds_read_b128); half a row is fetched half a row ahead of
// its use into registers of its own, so that no read is waited for - written the plain way the compiler, short of
// registers, reused one register pair for every read and waited for each (one multiply-add per ~50 cycles).  Products
// with the transposed matrix (y = x M) use the same routine on a transposed LDS copy: one vector in registers, results
// handed out as they are complete - the kernel stays within 128 registers, four waves per SIMD.
typedef double sp_d2 __attribute__((ext_vector_type(2)));
template <int H>                                    // H entries (H even)
struct LdsPiece {
  sp_d2 v[H / 2];
  __device__ __forceinline__ void fetch(const HX_LDS double* p) {
#pragma unroll
    for (int q = 0; q < H / 2; ++q) v[q] = reinterpret_cast<const HX_LDS sp_d2*>(p)[q];
  }
  __device__ __forceinline__ double at(const int b) const { return (b & 1) ? v[b >> 1].y : v[b >> 1].x; }
};
// y[a] = sum_b M[a][b] x[b], handed out two rows at a time (A even), the way the scratch stores them; two partial sums per
// row and half (the additions do not wait for one another)
template <int A, class Emit>
__device__ __forceinline__ void lds_mat_vec(const HX_LDS double* M, const double (&x)[A], const Emit& emit) {
  constexpr int H0 = ((A / 2) + 1) & ~1, H1 = A - H0;      // a row in two pieces of even length (20 = 10 + 10, 4 = 2 + 2)
  static_assert(H1 >= 0 && (H1 & 1) == 0, "even alphabet sizes");
  LdsPiece<H0> lo;
  LdsPiece<(H1 > 0 ? H1 : 2)> hi;
  lo.fetch(M);
  double ya = 0.;
#pragma unroll
  for (int a = 0; a < A; ++a) {
    if (H1 > 0) hi.fetch(M + a * A + H0);
    double p0 = 0., p1 = 0.;
#pragma unroll
    for (int b = 0; b < H0; b += 2) {
      p0 = __builtin_fma(lo.at(b), x[b], p0);
      p1 = __builtin_fma(lo.at(b + 1), x[b + 1], p1);
    }
    if (a + 1 < A) lo.fetch(M + (a + 1) * A);
    if (H1 > 0) {
#pragma unroll
      for (int b = 0; b < H1; b += 2) {
        p0 = __builtin_fma(hi.at(b), x[H0 + b], p0);
        p1 = __builtin_fma(hi.at(b + 1), x[H0 + b + 1], p1);
      }
    }
    const double y = p0 + p1;
    if (a & 1) emit(a >> 1, ya, y);
    else ya = y;
  }
}

// a device allocation that is freed on every way out of a launcher
struct SpBuf {
  void* p = nullptr;
  ~SpBuf() { if (p) (void)hipFree(p); }
};

extern thread_local float g_sp_ms;             // hx_sumprod.hip: what hx_sumprod_last_kernel_ms reports
const double* device_lse_table(int device);    // hx_api.hip: the 8-byte log_sum_exp table of an initialised device, or null
int api_fail(int code, const char* what);       // hx_api.hip: sets hx_last_error()

}  // namespace hx
