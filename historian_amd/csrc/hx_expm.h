// exp(R t) by one workgroup, with the bits of the host mirror's RateModel::getSubProbMatrix (hx_host_base.cpp; the
// restated gsl_linalg_exponential_ss): b = R t shrunk by 2^-squarings, eB = b / terms + I, eB = (b eB) (1 / count) + I for
// count = terms - 1 .. 1, then `squarings` squarings.  (terms, squarings, shrink) come from the host (hx_history_host.h), so
// what is left is fp64 multiplies, adds and 1. / integer, and the control flow is the same in every thread.
//
// The workgroup's threads share the A x A entries: entry e belongs to thread e mod blockDim.x, R entries a thread at most.
// An entry of a product is accumulated by its one thread over the inner index in increasing order, multiply and add rounded
// separately (the file that includes this is built with -ffp-contract=off), a zero left factor skipped - the host's
// operations in the host's order, whatever the number of waves.  b and eB live in LDS; a workgroup barrier stands between
// the last read of eB by a product and its overwrite, and between the overwrite and the next product's reads.
#pragma once
#include <hip/hip_runtime.h>
#include "hx_history_host.h"

namespace hx {

template <int R>
struct ExpmTile {
  int A;
  int row[R], col[R], ent[R];   // row * A, column and index of the thread's entries (0 for an entry past the matrix)
  bool live[R], diag[R];

  __device__ void init(const int a) {
    A = a;
    const int AA = A * A, T = (int)blockDim.x;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int e = (int)threadIdx.x + T * r;
      live[r] = e < AA;
      const int i = live[r] ? e / A : 0, j = live[r] ? e % A : 0;
      row[r] = i * A; col[r] = j; ent[r] = live[r] ? e : 0;
      diag[r] = live[r] && i == j;
    }
  }

  // acc = P Q, inner index increasing, product and sum rounded separately, a zero left factor skipped
  __device__ void matmul(const double* P, const double* Q, double (&acc)[R]) const {
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.;
    for (int k = 0; k < A; ++k) {
      const double* qk = Q + k * A;
      // All 2 R operands are read before the first is used, and every sum is formed whether it is kept or not: left to
      // itself the compiler turns the skip into a branch per entry with the right factor's read inside it - 2 R LDS
      // latencies in a row per k (measured with one wave a matrix: 0.167 ms for twelve 20 x 20 matrices, 0.063 ms like this).  The empty asm
      // statements only pin values to registers; the arithmetic is the same multiply, add and select.
      double p[R], q[R];
#pragma unroll
      for (int r = 0; r < R; ++r) { p[r] = P[row[r] + k]; q[r] = qk[col[r]]; }
#pragma unroll
      for (int r = 0; r < R; ++r) asm volatile("" : "+v"(p[r]), "+v"(q[r]));
#pragma unroll
      for (int r = 0; r < R; ++r) {
        double s = acc[r] + p[r] * q[r];
        asm volatile("" : "+v"(s));
        acc[r] = p[r] != 0. ? s : acc[r];
      }
    }
  }

  __device__ void store(double* M, const double (&v)[R]) const {
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (live[r]) M[ent[r]] = v[r];
  }

  // rate: [A][A] in global memory; Bm, Em: LDS [A * A] each; out: [A][A] in global memory.  Every thread of the workgroup calls it.
  __device__ void expm(const double* __restrict__ rate, const ExpmShape s, double* Bm, double* Em, double* __restrict__ out) const {
    double b[R], acc[R];
    const double first = 1. / s.terms;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      b[r] = live[r] ? rate[ent[r]] * s.t : 0.;
      b[r] *= s.shrink;
      acc[r] = b[r] * first;
      if (diag[r]) acc[r] += 1.;
    }
    store(Bm, b);
    store(Em, acc);
    __syncthreads();
    for (int count = s.terms - 1; count >= 1; --count) {
      matmul(Bm, Em, acc);
      __syncthreads();
      const double inv = 1. / count;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        acc[r] *= inv;
        if (diag[r]) acc[r] += 1.;
      }
      store(Em, acc);
      __syncthreads();
    }
    for (int q = 0; q < s.squarings; ++q) {
      matmul(Em, Em, acc);
      __syncthreads();
      store(Em, acc);
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (live[r]) out[ent[r]] = acc[r];
  }
};

int api_fail(int code, const char* what);       // hx_api.hip: sets hx_last_error()

// hx_expm.hip.  The plan for an alphabet of A symbols (HX_EXPM_WAVES is read here, once per set of rates), checked against the
// LDS of a CU: false when the alphabet is outside 1 .. 64 or the plan does not fit - for a launcher that checks before it allocates.
bool branch_expm_plan(int A, ExpmPlan* plan);
// One workgroup per (changed node, component): exp(R_cpt t) to mats[slot][cpt][node], slot = bit 1 of the node's info word.
// plan: what branch_expm_plan gave for A.  nodes: [n] on the device; shape: [n][C] on the device; rate: [C][A][A];
// mats: [2][C][N][A][A].  Returns 0, or -1 for a plan no instance serves (nothing is launched then).
int launch_branch_expm(const ExpmPlan& plan, const double* rate, const ExpmShape* shape, const int* nodes, const int* info, int n, int A, int C, int N,
                       double* mats, hipStream_t st);

}  // namespace hx
