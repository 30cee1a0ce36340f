// Device-side pieces shared by the kernels that read or write split planes (gemm_split.hip, gemm_bt.hip, whiten.hip), and the one host-side
// rule that goes with the rendezvous.  Everything here is inlined into its callers: no symbol, no kernel argument depends on this file.
#pragma once
#include "common.h"

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// power-of-two scale that puts |x| <= max at [2^13, 2^14]; max given as the bit pattern of a non-negative float
__device__ __forceinline__ float scale_from_maxbits(unsigned bits) {
    const int ex = (int)((bits >> 23) & 0xff);                 // biased exponent of the maximum: max in [2^(ex-127), 2^(ex-126))
    if (ex == 0 || ex == 0xff) return 1.f;                      // zero / denormal / non-finite maximum: leave unscaled
    int e = 14 - (ex - 126);                                    // max * 2^e in [2^13, 2^14)
    e = e > 100 ? 100 : (e < -100 ? -100 : e);
    return __builtin_bit_cast(float, (unsigned)(e + 127) << 23);
}

// 16-byte unit of (row, k half) in the LDS image of a (rows x 16 k) slab: the XOR swizzle that makes the ds_read_b128 fragment reads conflict free
__device__ __forceinline__ int lds_unit(int row, int kh) { return row * 2 + (kh ^ ((row >> 3) & 1)); }

// XCD-aware mapping of a dispatch slot to a work item (see gemm.hip): workgroup `wid` runs on XCD wid % 8, and every XCD owns one
// contiguous run of the nwg items.
__device__ __forceinline__ int64_t xcd_run_item(int64_t wid, int64_t nwg) {
    const int64_t q = nwg / 8, r = nwg % 8, xcd = wid % 8, j = wid / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}
// The same in 32 bits with q = nwg / 8 and r = nwg % 8 formed by the caller: gemm_bt.hip maps many items per workgroup inside its request
// stream, where 64-bit divisions expand to branchy routines (see its comment) and q, r are loop invariants it keeps in SGPRs.
__device__ __forceinline__ unsigned xcd_run_item(unsigned wid, unsigned q, unsigned r) {
    const unsigned xcd = wid % 8, j = wid / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}

// Rendezvous of the n workgroups that share operand lines: a BOUNDED spin on one counter per group -- a pacing hint, never needed for
// correctness.  A workgroup that waited SYNC_LIMIT for its partners goes on alone and stops waiting after its second time-out, so a launch
// next to kernels that hold some CUs, or two such launches on different streams, cannot deadlock.  Every workgroup adds exactly 2 to its
// group's counter (arrive + depart, or both at once when it no longer waits); the add that completes 2 n resets the word, so the counters
// are zero between launches.
constexpr unsigned long long SYNC_LIMIT = 2000ull;       // wall_clock64 ticks (100 MHz): 20 us

__device__ __forceinline__ void wg_rendezvous(unsigned* ctr, unsigned n, int& patience) {
    if (threadIdx.x == 0) {
        if (patience > 0) {
            __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long t0 = wall_clock64();
            while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < n) {
                if (wall_clock64() - t0 > SYNC_LIMIT) { --patience; break; }
                __builtin_amdgcn_s_sleep(4);
            }
            if (__hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == 2u * n)
                __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else if (__hip_atomic_fetch_add(ctr, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 2u == 2u * n) {
            __hip_atomic_store(ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __builtin_amdgcn_s_barrier();        // bare: requests in flight (LDS-DMA, the previous item's stores) stay in flight
}

// Host: may the tm row tiles of a column strip rendezvous at the start of a work item?  They must be tm consecutive items of one XCD's run
// (xcd_run_item) taken in the same persistent round by tm different workgroups: every XCD's run and every XCD's share of the grid is a whole
// number of strips, and every round is full.
inline bool strip_rendezvous_ok(int64_t tm, int64_t nwg, int64_t grid) {
    return tm >= 2 && nwg % 8 == 0 && nwg >= 16 && (nwg / 8) % tm == 0 && (grid / 8) % tm == 0 && (nwg <= grid || nwg % grid == 0);
}

}  // namespace
