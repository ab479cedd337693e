// The strip hand-off (device only): how a wave that sweeps a 64-row strip tells the wave of the strip below that columns of
// its last row are in memory.  Every strip-pipelined fill uses these functions; the rules they rely on are stated here once.
//
//  1. Order.  The vector-memory operations of a wave retire in issue order: `s_waitcnt vmcnt(N)` returns when all but the
//     wave's N youngest have completed, and a load sees every store the wave issued before it.
//  2. Publish behind a drain.  A progress counter is monotonic and says "columns < c of my last row are in memory".  It is
//     written by lane 0 only, and only behind a drain that covers those columns' stores: vmcnt(0), or - for a sweep whose
//     iteration issues a fixed number of stores - the lagged drain below, which publishes a column LAG steps after its stores
//     were issued and waits only for the operations older than the LAG / 2 iterations since.
//  3. Scope.  Waves of one workgroup share a CU and its L1: an LDS counter and a drain are a workgroup-scope release, and
//     the consumer's agent-scope loads (served by L2) never see a stale line.  Across workgroups (MULTI launches: a pair's
//     strips dealt to several workgroups, possibly on other XCDs) the cells are stored write-through, `sc1`, never `nt`,
//     which may stay in the storing XCD's L2; the counter lives in memory and is stored and polled at agent scope.
//  4. No cycle.  Strip s waits for strip s - 1 only and strip 0 waits for nobody, so the waits form a chain, not a circle:
//     every workgroup of a MULTI launch must be resident, and the launchers see to that.
//  5. Giving up.  Only the agent-scope wait can starve (a workgroup that never became resident), so it polls with bounded
//     patience.  A wave that gave up computes no more cells of the pair and must make the pair's result NaN, never a wrong
//     number and never a hang, by one of two conventions: it sets slot [255] of the pair's counters, which the wave of the
//     last strip reads (chain and leaf-linear fills), or it publishes HX_MULTI_POISON, which makes every wave below give up
//     in turn, down to the wave of the last strip (general-profile fills).
#pragma once
#include <hip/hip_runtime.h>
#include <utility>
#include "hx_policy.h"
#include "hx_kernels.h"

namespace hx {

typedef double hd2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ---- waiting -----------------------------------------------------------------------------------------------------------
// Wait until LDS counter `counters[index]` has reached `need`; what the caller loads afterwards stays behind the wait.  SLEEP: the s_sleep
// argument between polls.  `seen` caches the last value read (wave-uniform, in a scalar register) across calls.
template <int SLEEP, class Counter>
__device__ __forceinline__ void lds_wait(Counter* counters, const int index, int& seen, const int need) {
  while (seen < need) {
    seen = __builtin_amdgcn_readfirstlane(counters[index]);
    if (seen < need) __builtin_amdgcn_s_sleep(SLEEP);
  }
  asm volatile("" ::: "memory");
}
template <int SLEEP, class Counter>
__device__ __forceinline__ void lds_wait(Counter* counters, const int index, const int need) {
  while (counters[index] < need) __builtin_amdgcn_s_sleep(SLEEP);
  asm volatile("" ::: "memory");
}

// Wait until another workgroup's counter `counters[index]` has reached `need`, for at most `patience` unsatisfied polls.  True: the wave must
// give up (rule 5) - the patience ran out, or the producer published HX_MULTI_POISON.
template <int SLEEP>
__device__ __forceinline__ bool agent_wait(const HX_GLOBAL int* counters, const int index, int& seen, const int need, const int patience) {
  int polls = 0;
  bool out = false;
  while (seen < need) {
    seen = __builtin_amdgcn_readfirstlane(__hip_atomic_load(counters + index, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (seen < need) {
      if (++polls > patience) { out = true; break; }
      __builtin_amdgcn_s_sleep(SLEEP);
    }
  }
  asm volatile("" ::: "memory");
  return out || seen == HX_MULTI_POISON;
}

// ---- publishing (behind the caller's drain: rule 2) ----------------------------------------------------------------------
// (in LDS: `if (lane == 0) counters[wave] = value`, at the site)
// `dead`: the wave gave up and says so to the waves below (the poison convention)
__device__ __forceinline__ void agent_publish(HX_GLOBAL int* counter, const int lane, const int value, const bool dead = false) {
  if (lane == 0) __hip_atomic_store(counter, dead ? HX_MULTI_POISON : value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the flag convention: slot [255] of the pair's 256 counters
__device__ __forceinline__ void raise_gave_up(HX_GLOBAL int* counters, const int lane) { agent_publish(counters + 255, lane, 1); }

// The wave of a MULTI launch's last strip, before it reads the pair's result: its own stores out, this CU's L1 dropped
// (cells of other workgroups' strips), and - flag convention - whether any wave of the pair gave up.
__device__ __forceinline__ void agent_acquire() {
  drain_stores();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  drain_stores();
}
__device__ __forceinline__ bool acquire_gave_up(const HX_GLOBAL int* counters) {
  agent_acquire();
  return __hip_atomic_load(counters + 255, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

// ---- the lagged publish ----------------------------------------------------------------------------------------------------
// For a sweep of two steps per iteration whose iteration issues at least STORES_PER_ITER vector-memory operations: everything
// stored LAG steps = LAG / 2 iterations ago is older than the wave's STORES_PER_ITER * LAG / 2 youngest operations.
template <int STORES_PER_ITER, int LAG>
__device__ __forceinline__ void drain_lagged() {
  constexpr int WAIT = STORES_PER_ITER * (LAG / 2) < 63 ? STORES_PER_ITER * (LAG / 2) : 63;
  static_assert(WAIT <= STORES_PER_ITER * (LAG / 2) && WAIT <= 63 && LAG % 2 == 0,
                "the wait count must not exceed the operations issued since the published column's stores");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAIT) : "memory");
}

// ---- cells that cross workgroups (rule 3) ---------------------------------------------------------------------------------
template <int N> struct Planes { double v[N]; };
// a cell's N state planes with relaxed agent-scope loads (global_load ... sc1): served by L2, never by a stale L1 line
// (a pack expansion, not a loop: the sweeps' address arithmetic is as if the N loads were written out)
template <int... K>
__device__ __forceinline__ Planes<sizeof...(K)> load_cell_agent(const HX_GLOBAL double* M, const int64_t plane, const int64_t slot,
                                                                std::integer_sequence<int, K...>) {
  return Planes<sizeof...(K)>{{__hip_atomic_load(M + K * plane + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)...}};
}
template <int N>
__device__ __forceinline__ Planes<N> load_cell_agent(const HX_GLOBAL double* M, const int64_t plane, const int64_t slot) {
  return load_cell_agent(M, plane, slot, std::make_integer_sequence<int, N>{});
}
// a step pair's N planes, 16 bytes per lane and plane, write-through.  The s_nop belongs to the store: a vector instruction
// may not overwrite the data registers of a store of more than 8 bytes within two wait states of it, and the compiler does
// not look for that hazard behind inline assembly (it put the next plane's address arithmetic there).
template <int N>
__device__ __forceinline__ void store_pair_through(HX_GLOBAL hd2v* M2, const int64_t plane2, const hd2v (&v)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(&M2[k * plane2]), "v"(v[k]) : "memory");
}

// ---- step windows of the general-profile sweeps ---------------------------------------------------------------------------
// A banded strip sweeps the (up to two) step windows [lo, hi) that hold its in-envelope cells (host: strip_windows; the
// sweeps read them into two arrays at their site, whose form the compiler's placement of them depends on).
// Columns of the strip's last row that are final once window w is drained: those between or after the windows hold no
// in-envelope cell of this strip, so they count as complete as soon as everything before them is.
__device__ __forceinline__ int final_after_window(const int (&lo)[2], const int (&hi)[2], const int w, const int Cc) {
  const int upto = (w == 0 && hi[1] > lo[1]) ? lo[1] - 63 : Cc;
  return upto > Cc ? Cc : upto;
}

}  // namespace hx
