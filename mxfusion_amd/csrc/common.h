// Shared host/device infrastructure of libmxf_gp.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <stdlib.h>
#include <limits.h>
#include <type_traits>
#include "../../include/mxf_gp.h"
#include "pointwise_plan.h"      // grid_for, grid_for_reduce

// Tuning knobs: numbers of the shipped path (grid sizes, periods, block sizes), instruments, and shapes a test forces.  The shipped library
// is built WITHOUT -DMXF_PROBES: every knob is its compile-time default and the library reads no MXF_* environment variable except
// MXF_RCCL_LIB (a path).  The probe build (make probe -> libmxf_gp_probe.so, selected with MXF_GP_LIB by tests/probes/*) reads them from
// the environment once per process.  Knobs that selected a different code path were removed with their paths; DESIGN_HISTORY.md, "Variants
// measured and removed", keeps their numbers.
#ifdef MXF_PROBES
#define MXF_KNOB(name, dflt) (getenv(name) ? atoll(getenv(name)) : (long long)(dflt))
#define MXF_KNOB_SET(name) (getenv(name) != nullptr)
#else
#define MXF_KNOB(name, dflt) ((long long)(dflt))
#define MXF_KNOB_SET(name) (false)
#endif

// Probe build only (MXF_SVGP_STAGES=1): device-time stamps of the SVGP training call's stages, printed (stderr) at the end of the call after a
// device synchronise -- the call's own critical path without a profiler in the way (the profiler's ~30 us per launch makes a 4-sample step
// host-bound and its timeline misleading).  tests/probes/svgp_stages.py
#ifdef MXF_PROBES
struct mxf_stage_log {
    static const int N = 48;
    hipEvent_t ev[N]; const char* name[N]; int n = 0; bool made = false;
    void mark(const char* nm, hipStream_t s) {
        if (!made) { for (int i = 0; i < N; ++i) (void)hipEventCreate(&ev[i]); made = true; }
        if (n < N) { name[n] = nm; (void)hipEventRecord(ev[n], s); ++n; }
    }
    void dump() {
        (void)hipDeviceSynchronize();
        for (int i = 1; i < n; ++i) { float ms = 0.f; (void)hipEventElapsedTime(&ms, ev[0], ev[i]); fprintf(stderr, "  stage %-28s %8.3f ms\n", name[i], ms); }
        fprintf(stderr, "  --\n");
        n = 0;
    }
};
#define MXF_STAGE(h, nm, s) do { static const bool on_ = MXF_KNOB("MXF_SVGP_STAGES", 0) != 0; if (on_) (h)->stages.mark(nm, s); } while (0)
#define MXF_STAGE_DUMP(h) do { static const bool on_ = MXF_KNOB("MXF_SVGP_STAGES", 0) != 0; if (on_) (h)->stages.dump(); } while (0)
#else
#define MXF_STAGE(h, nm, s) do { } while (0)
#define MXF_STAGE_DUMP(h) do { } while (0)
#endif

// In-step durations of the SVGP training call's bulk kernels (mxf_svgp_timing): HIP events around them on the stream each runs on -- what
// bench.py's roofline entries for the in-step passes divide by.  Off by default (two event records per kernel when on).
constexpr int MXF_NT = 8;
struct mxf_timing {
    bool on = false, made = false;
    hipEvent_t ev[2 * MXF_NT];
    bool used[MXF_NT] = {false, false, false, false, false, false, false, false};
    bool init() {
        if (made) return true;
        for (int i = 0; i < 2 * MXF_NT; ++i) if (hipEventCreate(&ev[i]) != hipSuccess) return false;
        made = true;
        return true;
    }
};
enum { MXF_T_PLANES_A = 0, MXF_T_PSI2 = 1, MXF_T_PLANES_B = 2, MXF_T_TGEMM = 3, MXF_T_BWD = 4, MXF_T_CHAIN = 5, MXF_T_VGEMM = 6, MXF_T_CALL = 7 };
#define MXF_T0(h, i, s) do { if ((h)->tm.on) { (void)hipEventRecord((h)->tm.ev[2 * (i)], s); (h)->tm.used[i] = true; } } while (0)
#define MXF_T1(h, i, s) do { if ((h)->tm.on) (void)hipEventRecord((h)->tm.ev[2 * (i) + 1], s); } while (0)

// A device buffer grown on demand (mxf_grow) and a rotating ring of zeroed 32-bit counters (mxf_ring_take).
struct mxf_buf { void* p = nullptr; size_t bytes = 0; };
struct mxf_ring { unsigned* p = nullptr; unsigned cursor = 0; };

struct mxf_ctx {
    mxf_timing tm;
#ifdef MXF_PROBES
    mxf_stage_log stages;
#endif
    int device = 0;
    std::string err;
    // Scratch, never allocated inside a graph capture; mxf_each_buf lists them for mxf_workspace_bytes and mxf_destroy.
    mxf_buf ws;                // general scratch (mxf_ws)
    mxf_buf gram_ws;           // pre-scaled coordinates of mxf_gram (separate: composites hold `ws` while calling mxf_gram)
    mxf_buf bwd_acc;           // MFMA reverse pass (svgp_bwd_mfma.hip; layout: gram_bwd_plan.h): float64 row-side sums [M][16] + 16, scaled coordinates
    mxf_buf pinv;              // ring of 16 x 16 diagonal-block inverses handed from the factoring to the solving workgroups of potrf_tiles_kernel
    size_t pinv_cursor = 0;    // (in doubles)
    int64_t ws_generation = 0; // bumped whenever one of the buffers above is (re-)allocated: device pointers baked into a captured hipGraph are stale after that
    // Internal streams and their events, created on first use, all of a set or none (mxf_side_set / mxf_potrf_set below).
    bool side_ready = false;                        // the SVGP step's independent chains run concurrently (composite.hip)
    hipStream_t side = nullptr, side2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr, ev_aux = nullptr, ev_aux2 = nullptr, ev_su = nullptr;
    hipEvent_t ev_k1 = nullptr, ev_k3 = nullptr;    // the SVGP call's condition norms and value scalars leave the caller's stream
    bool potrf_aux_ready = false;                   // the blocked Cholesky (chol.hip: PotrfCall's stages say who records and waits on what)
    hipStream_t potrf_aux = nullptr;                // look-ahead: the trailing update next to the next panel's factorisation
    hipEvent_t ev_pa = nullptr, ev_pb = nullptr, ev_ph = nullptr;
    hipStream_t potrf_inv = nullptr;                // eager inverse: the products of its row blocks
    hipStream_t potrf_inv_diag = nullptr;           // eager inverse: the inverses of its diagonal blocks (latency-bound small launches)
    hipEvent_t ev_pi = nullptr, ev_pj = nullptr, ev_pc = nullptr;
    double* cond_dev = nullptr; // [ |Kuu + jitter I|_1, |(Kuu + jitter I)^-1|_1 ] of the last SVGP training call (mxf_svgp_last_cond)
    double* cond_host = nullptr; // pinned, device-visible host words, MXF_COND_SLOTS x [running MAX, last] of the condition numbers the training calls published into their slot (mxf_svgp_cond_nowait / mxf_svgp_cond_slot)
    int svgp_form = 0;         // float32 streaming form of the next SVGP training calls (mxf_svgp_configure): 0 explicit inverse, 1 whitened
    int cond_slot = 0;         // the slot the next SVGP training calls publish their condition number into
    void* comm = nullptr;      // RCCL communicator of mxf_comm_init (comm.hip); nullptr on single-GPU handles
    int comm_nranks = 0, comm_rank = -1;
    mxf_ring flags;            // arrival counters for in-kernel workgroup hand-offs (potrf panel); each use leaves 0 behind
    mxf_ring gsync;            // rendezvous counters of the wide split GEMMs (pacing hints only; gemm_split.hip); each use leaves 0 behind
};
template <typename F> static inline void mxf_each_buf(mxf_ctx* h, F f) { for (mxf_buf* b : {&h->ws, &h->gram_ws, &h->bwd_acc, &h->pinv}) f(*b); }
template <typename F> static inline void mxf_each_ring(mxf_ctx* h, F f) { for (mxf_ring* r : {&h->flags, &h->gsync}) f(*r); }

constexpr int MXF_COND_SLOTS = 64;
// the condition words of the SVGP training call: device accumulators + the pinned host slots (allocated on first use)
static inline bool mxf_cond_init(mxf_ctx* h) {
    if (!h->cond_dev) {
        if (hipMalloc((void**)&h->cond_dev, 4 * sizeof(double)) != hipSuccess) { h->cond_dev = nullptr; return false; }
        if (hipMemset(h->cond_dev, 0, 4 * sizeof(double)) != hipSuccess) return false;
    }
    if (!h->cond_host) {
        if (hipHostMalloc((void**)&h->cond_host, 2 * MXF_COND_SLOTS * sizeof(double), hipHostMallocMapped) != hipSuccess) { h->cond_host = nullptr; return false; }
        for (int i = 0; i < 2 * MXF_COND_SLOTS; ++i) h->cond_host[i] = 0.0;
    }
    return true;
}

// A fresh run of `count` zeroed counters from a ring of 2^18 (rotating: a run is reused only after 2^18 / count later launches have been
// queued -- by then the launch that used it has long left them at zero); nullptr = none available.
constexpr unsigned MXF_NRING = 1u << 18;
static inline unsigned* mxf_ring_take(mxf_ring& r, unsigned count) {
    if (!r.p) {
        if (hipMalloc((void**)&r.p, MXF_NRING * sizeof(unsigned)) != hipSuccess) { r.p = nullptr; return nullptr; }
        if (hipMemset(r.p, 0, MXF_NRING * sizeof(unsigned)) != hipSuccess) { (void)hipFree(r.p); r.p = nullptr; return nullptr; }
    }
    if (count > MXF_NRING) return nullptr;
    if (r.cursor + count > MXF_NRING) r.cursor = 0;
    unsigned* p = r.p + r.cursor;
    r.cursor += count;
    return p;
}
// hand-off counters: the caller fails without them
static inline int* mxf_flags(mxf_ctx* h, unsigned count) { return (int*)mxf_ring_take(h->flags, count); }
// rendezvous counters: without them (or for a run longer than a quarter of the ring) the caller launches without rendezvous
static inline unsigned* mxf_gsync(mxf_ctx* h, unsigned count) { return count == 0 || count > MXF_NRING / 4 ? nullptr : mxf_ring_take(h->gsync, count); }

// At least `need` bytes in `b`.  A buffer that is too small is freed -- after a device synchronise: queued launches may still use it -- and
// `want` >= need bytes are allocated (each buffer has its own head-room rule); every (re-)allocation bumps ws_generation.  nullptr: out of memory.
static inline void* mxf_grow(mxf_ctx* h, mxf_buf& b, size_t need, size_t want) {
    if (need <= b.bytes) return b.p;
    if (b.p) { (void)hipDeviceSynchronize(); (void)hipFree(b.p); b = mxf_buf(); }
    ++h->ws_generation;
    if (hipMalloc(&b.p, want) != hipSuccess) { b.p = nullptr; return nullptr; }
    b.bytes = want;
    return b.p;
}
// scratch allocator: returns a pointer valid until the next call that needs more
static inline void* mxf_ws(mxf_ctx* h, size_t bytes) { return mxf_grow(h, h->ws, bytes, bytes + (bytes >> 2) + (1u << 20)); }
static inline void* mxf_gram_ws(mxf_ctx* h, size_t bytes) { return mxf_grow(h, h->gram_ws, bytes, bytes + (bytes >> 2) + (1u << 16)); }

// ring allocator of the Cholesky tile kernel's inverse blocks: the ring holds at least two regions of the largest request, so a region is
// reused no earlier than the launch after next ON THE SAME STREAM -- by then its readers (the previous launch) have finished in stream order.
// (Two streams factoring through ONE handle would share the ring: the C ABI's rule is one handle per thread and calls not re-entrant.)
static inline double* mxf_potrf_inv(mxf_ctx* h, size_t elems) {
    const size_t have = h->pinv.bytes;
    const size_t want = elems * 4 > ((size_t)4 << 20) ? elems * 4 : ((size_t)4 << 20);      // >= 32 MB
    double* ring = (double*)mxf_grow(h, h->pinv, elems * 2 * sizeof(double), want * sizeof(double));
    if (!ring) return nullptr;
    if (h->pinv.bytes != have /* a new ring */ || h->pinv_cursor + elems > h->pinv.bytes / sizeof(double)) h->pinv_cursor = 0;
    double* p = ring + h->pinv_cursor;
    h->pinv_cursor += elems;
    return p;
}

#define MXF_FAIL(h, code, ...)                                   \
    do {                                                         \
        char _b[512];                                            \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                   \
        if (h) (h)->err = _b;                                    \
        return (code);                                           \
    } while (0)

#define MXF_HIP(h, call)                                                                   \
    do {                                                                                   \
        hipError_t _e = (call);                                                            \
        if (_e != hipSuccess)                                                              \
            MXF_FAIL(h, -100 - (int)_e, "%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(_e)); \
    } while (0)

#define MXF_LAUNCH_CHECK(h)                                                                \
    do {                                                                                   \
        hipError_t _e = hipGetLastError();                                                 \
        if (_e != hipSuccess)                                                              \
            MXF_FAIL(h, -100 - (int)_e, "%s:%d kernel launch -> %s", __FILE__, __LINE__, hipGetErrorString(_e)); \
    } while (0)

// The handle's internal streams and events in sets that exist as a whole or not at all: mxf_async_init creates a set (a failure rolls back
// what it had created, and a later call tries again), mxf_destroy releases the same lists.  Unused trailing slots are nullptr.
struct mxf_async_set { bool* ready; hipStream_t* streams[3]; hipEvent_t* events[8]; };
static inline mxf_async_set mxf_side_set(mxf_ctx* h) {
    return {&h->side_ready, {&h->side, &h->side2}, {&h->ev_fork, &h->ev_join, &h->ev_join2, &h->ev_aux, &h->ev_aux2, &h->ev_su, &h->ev_k1, &h->ev_k3}};
}
static inline mxf_async_set mxf_potrf_set(mxf_ctx* h) {
    return {&h->potrf_aux_ready, {&h->potrf_aux, &h->potrf_inv, &h->potrf_inv_diag}, {&h->ev_pa, &h->ev_pb, &h->ev_ph, &h->ev_pi, &h->ev_pj, &h->ev_pc}};
}
static inline void mxf_async_release(const mxf_async_set& g) {
    for (hipEvent_t* e : g.events) if (e && *e) { (void)hipEventDestroy(*e); *e = nullptr; }
    for (hipStream_t* s : g.streams) if (s && *s) { (void)hipStreamDestroy(*s); *s = nullptr; }
    *g.ready = false;
}
static inline bool mxf_async_init(const mxf_async_set& g) {
    if (*g.ready) return true;
    bool ok = true;
    for (hipStream_t* s : g.streams) if (s && ok && hipStreamCreateWithFlags(s, hipStreamNonBlocking) != hipSuccess) { *s = nullptr; ok = false; }
    for (hipEvent_t* e : g.events) if (e && ok && hipEventCreateWithFlags(e, hipEventDisableTiming) != hipSuccess) { *e = nullptr; ok = false; }
    if (!ok) mxf_async_release(g);
    return *g.ready = ok;
}
static inline bool mxf_side_init(mxf_ctx* h) { return mxf_async_init(mxf_side_set(h)); }
static inline bool mxf_potrf_aux_init(mxf_ctx* h) { return mxf_async_init(mxf_potrf_set(h)); }

static inline size_t mxf_esize(int dtype) { return dtype == MXF_F64 ? 8 : 4; }
static inline size_t mxf_align(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// f(std::integral_constant<int, V>) for the V among VS that equals v; NO_CASE: none does
constexpr int NO_CASE = INT_MIN;
template <int... VS, typename F>
int dispatch(int v, F&& f) {
    int rc = NO_CASE;
    (void)((v == VS && ((rc = f(std::integral_constant<int, VS>{})), true)) || ...);
    return rc;
}
// the element type of a dtype tag: dispatch<MXF_F32, MXF_F64>(dtype, [&](auto dt) { using T = mxf_elem_t<decltype(dt)::value>; ... })
template <int DTYPE> using mxf_elem_t = std::conditional_t<DTYPE == MXF_F64, double, float>;
// The pointwise and per-row launchers (elementwise.hip .. transform.hip): launch(T()) with the element type of `dtype`, each launch written
// once in T.  An unknown dtype is the family's refusal; a launcher that returns non-zero has refused itself; otherwise the launch is checked.
static inline int mxf_bad_dtype(mxf_handle h, const char* name, int dtype) { MXF_FAIL(h, -2, "%s: bad dtype %d", name, dtype); }
template <typename F>
int mxf_typed(mxf_handle h, const char* name, int dtype, F&& launch) {
    const int rc = dispatch<MXF_F32, MXF_F64>(dtype, [&](auto dt) {
        using T = mxf_elem_t<decltype(dt)::value>;
        if constexpr (std::is_void_v<decltype(launch(T()))>) { launch(T()); return 0; } else return launch(T());
    });
    if (rc == NO_CASE) return mxf_bad_dtype(h, name, dtype);
    if (rc) return rc;
    MXF_LAUNCH_CHECK(h);
    return 0;
}

// ---- device helpers -------------------------------------------------------------------------
template <typename T> struct Vec16;   // 16-byte vector of T
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef double f64x2_t __attribute__((ext_vector_type(2)));
template <> struct Vec16<float> { typedef f32x4_t type; static constexpr int n = 4; };
template <> struct Vec16<double> { typedef f64x2_t type; static constexpr int n = 2; };

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// wave64 sum with DPP (no LDS traffic); the total is valid in LANE 63 only.
// quad butterflies, row_half_mirror, row_mirror give every lane of a 16-lane row its row sum; row_bcast:15 / :31 fold rows.
#define MXF_DPP_F(v, ctrl, rmask) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, (v)), (ctrl), (rmask), 0xf, false))
__device__ __forceinline__ float wave_sum63(float v) {
    v += MXF_DPP_F(v, 0xB1, 0xf);    // quad_perm [1,0,3,2]
    v += MXF_DPP_F(v, 0x4E, 0xf);    // quad_perm [2,3,0,1]
    v += MXF_DPP_F(v, 0x141, 0xf);   // row_half_mirror
    v += MXF_DPP_F(v, 0x140, 0xf);   // row_mirror
    v += MXF_DPP_F(v, 0x142, 0xa);   // row_bcast:15 -> rows 1,3
    v += MXF_DPP_F(v, 0x143, 0xc);   // row_bcast:31 -> rows 2,3
    return v;
}
#define MXF_DPP_D(v, ctrl, rmask)                                                                                  \
    __builtin_bit_cast(double, (((unsigned long long)(unsigned)__builtin_amdgcn_update_dpp(                        \
                                     0, (int)(__builtin_bit_cast(unsigned long long, (v)) >> 32), (ctrl), (rmask), 0xf, false)) << 32) | \
                                (unsigned long long)(unsigned)__builtin_amdgcn_update_dpp(                         \
                                    0, (int)(__builtin_bit_cast(unsigned long long, (v)) & 0xffffffffull), (ctrl), (rmask), 0xf, false))
__device__ __forceinline__ double wave_sum63(double v) {
    v += MXF_DPP_D(v, 0xB1, 0xf);
    v += MXF_DPP_D(v, 0x4E, 0xf);
    v += MXF_DPP_D(v, 0x141, 0xf);
    v += MXF_DPP_D(v, 0x140, 0xf);
    v += MXF_DPP_D(v, 0x142, 0xa);
    v += MXF_DPP_D(v, 0x143, 0xc);
    return v;
}

// ---- row-level reduce-scatter of N per-lane values (N = 2, 4, 8, 16) -------------------------------------------------------------
// Input: every lane holds a[0..N-1].  Output: lane l of each 16-lane row holds  sum over the row's 16 lanes of a[l & (N-1)]
// (all lanes valid; lanes with (l & 15) < N form one complete set per row).  A halving butterfly: at each level a lane keeps one
// half of its values and receives the partner's partial sums of that half, so the cost is (N-1) DPP adds + 2(N-1) selects
// instead of 4N DPP adds for N separate row reductions.  Partners (row_mirror, row_half_mirror, quad reverse, quad xor-1) always hold
// the same half, so every level is ONE symmetric DPP move.
template <int CTRL> __device__ __forceinline__ float mxf_dpp_mov(float v) { return MXF_DPP_F(v, CTRL, 0xf); }
template <int CTRL> __device__ __forceinline__ double mxf_dpp_mov(double v) { return MXF_DPP_D(v, CTRL, 0xf); }

template <typename T, int HALF, int CTRL>
__device__ __forceinline__ void mxf_rs_level(T* a, bool upper) {
#pragma unroll
    for (int i = 0; i < HALF; ++i) {
        const T keep = upper ? a[i + HALF] : a[i];
        const T send = upper ? a[i] : a[i + HALF];
        a[i] = keep + mxf_dpp_mov<CTRL>(send);
    }
}
template <typename T, int N>
__device__ __forceinline__ T row_reduce_scatter(T* a /* N values, clobbered */, int lane) {
    static_assert(N == 1 || N == 2 || N == 4 || N == 8 || N == 16, "row_reduce_scatter: N must be a power of two <= 16");
    if (N >= 16) mxf_rs_level<T, 8, 0x140>(a, (lane & 8) != 0);                 // row_mirror        i <-> 15-i
    if (N >= 8) mxf_rs_level<T, (N >= 8 ? 4 : 1), 0x141>(a, (lane & 4) != 0);   // row_half_mirror   i <-> 7-i (within 8)
    if (N >= 4) mxf_rs_level<T, (N >= 4 ? 2 : 1), 0x1B>(a, (lane & 2) != 0);    // quad_perm [3,2,1,0]
    if (N >= 2) mxf_rs_level<T, 1, 0xB1>(a, (lane & 1) != 0);                   // quad_perm [1,0,3,2]
    T v = a[0];
    // lanes that hold the same index differ in the bits above log2(N): fold them with rotations (index-preserving)
    if (N <= 1) v += mxf_dpp_mov<0xB1>(v);
    if (N <= 2) v += mxf_dpp_mov<0x4E>(v);      // quad_perm [2,3,0,1]  (xor 2)
    if (N <= 4) v += mxf_dpp_mov<0x124>(v);     // row_ror:4
    if (N <= 8) v += mxf_dpp_mov<0x128>(v);     // row_ror:8
    return v;
}

// lane-wise sum over the wave's four 16-lane rows (every lane ends with x[l%16 of row0] + ... + x[l%16 of row3]): the gfx950
// v_permlane16_swap / v_permlane32_swap instructions.  Inline asm: the clang builtin (ROCm 7.2) folds its two results into one
// register and returns 2x (tests/probes/probe_permlane.hip).
__device__ __forceinline__ float wave_rows_sum(float v) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    a = a + b; b = a;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    return a + b;
}

// block-wide sum (blockDim.x multiple of 64, <= 1024); result valid in thread 0
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* smem /* >= 16 */) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if (lane == 0) smem[w] = v;
    __syncthreads();
    T r = 0;
    if (threadIdx.x < 64) {
        r = (threadIdx.x < nw) ? smem[threadIdx.x] : (T)0;
        r = wave_sum(r);
    }
    return r;
}

__device__ __forceinline__ void atomic_add(float* p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void atomic_add(double* p, double v) { unsafeAtomicAdd(p, v); }
// the same into LDS (workgroup scope)
__device__ __forceinline__ void lds_add(float* p, float v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_add(double* p, double v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// C-ABI entry points implemented across translation units share these internal (typed) launchers

// ---- float64 exponentials of the Gram kernels (arguments are never positive) ------------------------------------------------------
// The device library's exp / exp2 carry special-case handling the covariance functions never need; these are the bare forms:
// round-to-nearest split, degree-13 polynomial on |f| <= 1/2 (2^f) resp. |r| <= ln2/2 (e^r), v_ldexp_f64 (which also gives the gradual
// underflow).  Max error 1 ulp against libm over [0, 1100] (checked on the host with the same fma sequence).  RBF Gram float64 at
// N=65536: 7.43 -> 7.06 ms.  (Replacing v_rndne / v_cvt / v_ldexp by the 1.5 * 2^52 trick and an exponent-field add was slower: 7.73 ms.)
__device__ __forceinline__ double mxf_exp2_neg_f64(double x) {     // 2^(-x), x >= 0
    const double y = -x, n = __builtin_rint(y), f = y - n;
    double p = 1.369148885390412888e-12;
    p = fma(p, f, 2.567843599348820514e-11); p = fma(p, f, 4.445538271870811498e-10); p = fma(p, f, 7.054911620801123329e-09);
    p = fma(p, f, 1.017808600923969973e-07); p = fma(p, f, 1.321548679014430949e-06); p = fma(p, f, 1.525273380405984028e-05);
    p = fma(p, f, 0.0001540353039338160995); p = fma(p, f, 0.001333355814642844342); p = fma(p, f, 0.009618129107628477162);
    p = fma(p, f, 0.05550410866482157995); p = fma(p, f, 0.2402265069591007123); p = fma(p, f, 0.6931471805599453094);
    p = fma(p, f, 1.0);
    return ldexp(p, (int)n);
}
__device__ __forceinline__ double mxf_exp_nonpos_f64(double x) {   // e^x, x <= 0
    const double xc = fmax(x, -800.0), n = __builtin_rint(xc * 1.4426950408889634074);
    double r = fma(-n, 0.693147180369123816490, xc);
    r = fma(-n, 1.90821492927058770002e-10, r);
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0); p = fma(p, r, 1.0 / 39916800.0); p = fma(p, r, 1.0 / 3628800.0); p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0); p = fma(p, r, 1.0 / 5040.0); p = fma(p, r, 1.0 / 720.0); p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0); p = fma(p, r, 1.0 / 6.0); p = fma(p, r, 0.5); p = fma(p, r, 1.0); p = fma(p, r, 1.0);
    return ldexp(p, (int)n);
}
// the covariance functions' scalar pieces in both precisions (gram.hip, gram2.hip)
template <typename T> __device__ __forceinline__ T fast_exp2_neg(T x);   // 2^(-x), x >= 0
template <> __device__ __forceinline__ float fast_exp2_neg<float>(float x) { return __builtin_amdgcn_exp2f(-x); }
template <> __device__ __forceinline__ double fast_exp2_neg<double>(double x) { return mxf_exp2_neg_f64(x); }
template <typename T> __device__ __forceinline__ T t_sqrt(T x);
template <> __device__ __forceinline__ float t_sqrt<float>(float x) { return __builtin_sqrtf(x); }
template <> __device__ __forceinline__ double t_sqrt<double>(double x) { return sqrt(x); }
template <typename T> __device__ __forceinline__ T t_exp(T x);           // e^x, only called with x <= 0
template <> __device__ __forceinline__ float t_exp<float>(float x) { return __expf(x); }
template <> __device__ __forceinline__ double t_exp<double>(double x) { return mxf_exp_nonpos_f64(x); }
