// Hand-offs inside a launch: workgroups store partials, the last one to arrive reads them all back ("hand-offs
// inside a launch").  This is the only place where workgroups of one launch exchange data, and it is written once, here.
// The protocol is the write-through form of the kernel guide's inter-workgroup hand-off (guideline 16, recipe R1; the
// in-launch split-K reduction, second form) - no fences, so each rule below carries the correctness:
//   * every handed-off word goes through kg_pub_store / kg_pub_load (relaxed agent-scope atomics: both bypass the per-CU
//     L1), never through a plain access - ONE plain load in the last arriver may return a stale cached line;
//   * every wave that stored drains (the asm wait below - the compiler's own waits do not count) before the ticket;
//   * where a wave other than the storing one draws the ticket, a workgroup barrier lies between drain and draw;
//   * the "I am last" word is the caller's existing LDS word - no helper here declares a __shared__ object (a second
//     one moves the LDS layout of the kernels that stage through glds);
//   * the counters are the caller's: zeroed once when allocated, and zero again from the moment the last ticket of a
//     launch is drawn (`expected` = all arrivals at that counter in the launch, so nobody touches it afterwards;
//     kg_genblock_bwd alone resets when its last arriver has finished - see there);
//   * launches that share counters (or a workspace) must not overlap: one stream, or an event between them.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void kg_pub_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float kg_pub_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// (64-bit twins: the step counter of kg_input.hip, read by every workgroup and advanced by the last arriver)
__device__ __forceinline__ void kg_pub_store(long long* p, long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ long long kg_pub_load(const long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the storing wave's own stores are acknowledged
__device__ __forceinline__ void kg_pub_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// the pieces of a draw: the ticket's number, the reset (outside this header only kg_genblock_bwd uses them directly)
__device__ __forceinline__ int kg_ticket_number_(int* counter) { return __hip_atomic_fetch_add(counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void kg_ticket_reset_(int* counter) { __hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the draw behind a drain: true for the last of the `expected` arrivals, which has put the counter back to zero
__device__ __forceinline__ bool kg_ticket_take_(int* counter, int expected) {
    const bool last = kg_ticket_number_(counter) == expected - 1;
    if (last) kg_ticket_reset_(counter);
    return last;
}

// ONE lane that stored the partials itself (or nothing was stored): drain, draw
__device__ __forceinline__ bool kg_ticket_draw(int* counter, int expected) {
    kg_pub_drain();
    return kg_ticket_take_(counter, expected);
}

// A whole workgroup, any of whose waves stored: true (in every thread) for the last of `expected` workgroups.  Where only
// thread 0 stored, `if (tid == 0) flag = kg_ticket_draw(..)` and the kernel's own barrier do the same with less.
__device__ __forceinline__ bool kg_arrive_last(int* counter, int expected, int* lds_flag) {
    kg_pub_drain();
    __syncthreads();
    if (threadIdx.x == 0) *lds_flag = kg_ticket_take_(counter, expected);
    __syncthreads();
    return *lds_flag != 0;
}
