// Gram-matrix build for gfx950 (MI355X): one fused pass  X, X2, lengthscale, variance -> K.
//
// Replaces StationaryKernel._compute_R2 (kernels/stationary.py:74-107: syrk/gemm2 + 3 broadcast passes)
// and RBF/Matern._compute_K (rbf.py:71-72, matern.py:84-151: 2-6 more N^2 passes) of the reference.
//
// Roofline: HBM-WRITE bound.  Algorithmic bytes = S*N*N2*sizeof(T) written (+ (N+N2)*Q read).
// Layout / mapping (wave64):
//   * a wave owns a strip of 64*VEC consecutive columns (VEC = 16 B / sizeof(T)): lane l keeps the
//     VEC pre-scaled z-vectors of its columns in VGPRs for the whole row loop;
//   * a workgroup is ONE wave (64 threads) covering 16 rows of its strip; the pre-scaled x row is the same for all lanes and comes
//     through scalar loads (s_load_dwordx8/x16 into SGPRs, used directly as VOP3P sources): no LDS, no barrier;
//   * each lane produces VEC outputs per row and stores them with ONE 16-byte store, so a wave writes
//     1 KiB of one output row per instruction (full-line, fully coalesced), non-temporal (written once,
//     never re-read by this kernel).
#include "common.h"
#include "internal.h"
#include "gram_plan.h"
#include "kmv.h"          // coord_scale, cov_from: shared with the matrix-free product (kmv.hip)
#include <stdlib.h>

namespace {

template <typename T>
struct GramArgs {
    const T* X; const T* X2; const T* ls; const T* var; const T* dadd;
    const T* Xs; const T* Zs; int64_t sXs, sZs;   // pre-scaled, zero-padded coordinates [S|1][pad][QT] (prescale_kernel)
    T* K;
    int64_t N, N2, ldk;
    int64_t sX, sX2, sls, svar, sdadd, sK;
    int Q, ard, square, mode, vecst, tr;
    unsigned ncb;          // column blocks (grid.x = ncb * row blocks, column block fastest)
    T jitter;
};

// 2^(t / 64) for float64 from a 64-entry table of 2^(j / 64) (LDS) and a degree-5 polynomial on |g| <= 1/2 (g in 64ths): 11 VALU
// operations + one ds_read_b64 instead of the 18 of the degree-13 form (truncation (ln2/128)^6 / 6! = 3.5e-17; result within ~1 ulp).
__device__ __forceinline__ double exp2_64ths_tab(double t, const double* __restrict__ tab) {
    const double m = __builtin_rint(t), g = t - m;
    double p = 1.241784370171692541187e-12;
    p = fma(p, g, 5.732851688640402055966e-10); p = fma(p, g, 2.117313715546477506757e-7); p = fma(p, g, 0.00005864904955056169734706);
    p = fma(p, g, 0.01083042469624914545964); p = fma(p, g, 1.0);
    const int mi = (int)m;
    return ldexp(p * tab[mi & 63], mi >> 6);
}

// One-wave workgroups.  The x rows are read through wave-uniform (scalar) loads straight from the pre-scaled copy: no LDS, no
// barrier, and every wave is its own workgroup, dispatched and retired independently (measured on MI355X, f32 RBF N=65536:
// 4-wave blocks with an LDS x tile 5.67 TB/s, 4-wave blocks with scalar x 5.86, single-wave blocks with scalar x 6.52 TB/s --
// tests/probes/gram_variants.hip).
// FAST: plain overwrite (MXF_WRITE), 16-byte-aligned rows and N2 a multiple of VEC -- every store is one full 16-byte store and the
// accumulate / ragged-edge code (and its registers: 86 -> <= 64 VGPRs, i.e. 8 waves per SIMD) is compiled out.
template <typename T, int QT, int KIND, bool FAST>
__global__ __launch_bounds__(64) void gram_kernel(GramArgs<T> a, const T* __restrict__ Xs_all, const T* __restrict__ Zs_all,
                                                  T* __restrict__ K_all) {
    // (the three array pointers are separate __restrict__ kernel arguments: only then may the compiler read the x rows with SCALAR
    //  loads -- a pointer inside the by-value struct could alias the output and would be fetched with per-lane vector loads)
    const int MODE = FAST ? (int)MXF_WRITE : a.mode;
    const bool VECST = FAST ? true : (bool)a.vecst;
    constexpr int VEC = Vec16<T>::n;
    typedef typename Vec16<T>::type V;

    const int lane = threadIdx.x & 63;
    const int s = blockIdx.z;
    const int TRr = a.tr;                       // rows per block
    const int64_t row0 = (int64_t)(blockIdx.x / a.ncb) * TRr;
    const int64_t wcol0 = (int64_t)(blockIdx.x % a.ncb) * (64 * VEC);      // first column of the wave (wave-uniform)
    const int64_t col0 = wcol0 + (int64_t)lane * VEC;
    if (col0 >= a.N2 || row0 >= a.N) return;

    const T variance = (KIND == MXF_K_LINEAR) ? (T)1 : a.var[(int64_t)s * a.svar];
    T* __restrict__ K = K_all + (int64_t)s * a.sK;

    // prologue: unguarded 16-byte copies of the PRE-SCALED, zero-padded coordinates (prescale_kernel): the VEC z-vectors of this
    // lane's columns into VGPRs.
    T z[VEC][QT];
    const T* __restrict__ Xrows = nullptr;
    if (KIND != MXF_K_BIAS && KIND != MXF_K_WHITE) {
        Xrows = Xs_all + (int64_t)s * a.sXs + row0 * QT;       // wave-uniform
        const T* __restrict__ Zs = Zs_all + (int64_t)s * a.sZs + col0 * QT;
#pragma unroll
        for (int i = 0; i < VEC * QT; i += VEC)
            *reinterpret_cast<V*>(&z[0][0] + i) = *reinterpret_cast<const V*>(Zs + i);
    }

    const T dadd = a.square ? ((a.dadd ? a.dadd[(int64_t)s * a.sdadd] : (T)0) + a.jitter) : (T)0;
    const bool full = FAST ? true : (VECST && (col0 + VEC <= a.N2));
    // (an interleaved row assignment -- the NB workgroups that run side by side own every NB-th row of a band, so that the rows being
    //  written at any moment are consecutive -- was measured: 6.4 -> 4.1-5.4 TB/s; rows per workgroup stay consecutive)

    // one row: kv = covariances of (row, col0 .. col0+VEC-1), then the store.  DIAG (the "+ noise / jitter on the diagonal" and the
    // WHITE kernel) is a compile-time flag: only the few waves whose tile touches the diagonal run the variant with the compares.
    // the "+ noise / jitter on the diagonal" and the WHITE kernel touch one element per row: a SCALAR test (is this row inside the
    // wave's column range?) guards the per-lane compares, so the row loop carries no vector compare for them
    const bool diag_possible = __builtin_amdgcn_readfirstlane((int)(a.square && (KIND == MXF_K_WHITE || dadd != (T)0))) != 0;
    auto do_row = [&](int r) {
        const int64_t row = row0 + r;
        const bool DIAG = diag_possible && (uint64_t)(row - wcol0) < (uint64_t)(64 * VEC);
        T kv[VEC];
        if (KIND == MXF_K_BIAS) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) kv[v] = variance;
        } else if (KIND == MXF_K_WHITE) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) kv[v] = (DIAG && (col0 + v == row)) ? variance : (T)0;
        } else {
            T x[QT];
#pragma unroll
            for (int q = 0; q < QT; ++q) x[q] = Xrows[r * QT + q];      // s_load: the address is the same in every lane
            if constexpr (sizeof(T) == 4 && KIND != MXF_K_LINEAR) {
                // float: two outputs per v_pk_add_f32 / v_pk_fma_f32 (halves the VALU issue slots of the distance loop)
                typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int p = 0; p < VEC / 2; ++p) {
                    f32x2 acc2 = {0.f, 0.f};
#pragma unroll
                    for (int q = 0; q < QT; ++q) {
                        const f32x2 xx = {(float)x[q], (float)x[q]};
                        const f32x2 zz = {(float)z[2 * p][q], (float)z[2 * p + 1][q]};
                        const f32x2 d = xx - zz;
                        acc2 = __builtin_elementwise_fma(d, d, acc2);
                    }
                    kv[2 * p] = cov_from<T, KIND>((T)acc2.x, variance);
                    kv[2 * p + 1] = cov_from<T, KIND>((T)acc2.y, variance);
                }
            } else
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                T acc = 0;
                if (KIND == MXF_K_LINEAR) {
#pragma unroll
                    for (int q = 0; q < QT; ++q) acc = fma(x[q], z[v][q], acc);
                } else {
#pragma unroll
                    for (int q = 0; q < QT; ++q) { T d = x[q] - z[v][q]; acc = fma(d, d, acc); }
                }
                kv[v] = cov_from<T, KIND>(acc, variance);
            }
        }
        if (DIAG) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) if (col0 + v == row) kv[v] += dadd;
        }
        T* dst = K + row * a.ldk + col0;
        if (full) {
            V out;
            if (MODE != MXF_WRITE) {
                V old = *reinterpret_cast<const V*>(dst);
                T* o = reinterpret_cast<T*>(&old);
#pragma unroll
                for (int v = 0; v < VEC; ++v) kv[v] = (MODE == MXF_ACC_ADD) ? o[v] + kv[v] : o[v] * kv[v];
            }
            T* po = reinterpret_cast<T*>(&out);
#pragma unroll
            for (int v = 0; v < VEC; ++v) po[v] = kv[v];
            if (MODE == MXF_WRITE) __builtin_nontemporal_store(out, reinterpret_cast<V*>(dst));
            else *reinterpret_cast<V*>(dst) = out;
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                if (col0 + v < a.N2) {
                    T val = kv[v];
                    if (MODE == MXF_ACC_ADD) val = dst[v] + val;
                    if (MODE == MXF_ACC_MUL) val = dst[v] * val;
                    dst[v] = val;
                }
            }
        }
    };
    // number of this workgroup's rows that exist (wave-uniform)
    const int rmax = (a.N - row0) < TRr ? (int)(a.N - row0) : TRr;
#pragma unroll 2
    for (int r = 0; r < rmax; ++r) do_row(r);
}

// The overwrite path (MXF_WRITE, aligned, N2 % VEC == 0) of the coordinate kernels as ONE-WAVE workgroups with a short argument list:
// 5 pointers + 12 scalars instead of the 25-field GramArgs, whose lazily loaded fields put ~6 dependent s_load round trips in front
// of a workgroup that lives for only 16 rows.
// Grid: x = column block (fastest: neighbouring workgroups write neighbouring 1 KiB pieces of the same rows), y = row block, z = sample
// -- no integer division in the prologue.  The diagonal term is branch-free, dadd = dscale * dadd_p[s] + jitter (the host passes
// dscale = 0 and any valid pointer when there is none), so that all scalar loads of the prologue are issued back to back.
template <typename T> struct GramLean {
    int64_t N, N2, ldk, sXs, sZs, sK, svar, sdadd, sXn, sZn;
    int tr, has_diag;
    T dscale, jitter;
};

// XF (float64 RBF only): the squared distance in the reference's own expansion form |x|^2 + |z|^2 - 2 x.z (stationary.py:98-107) --
// 1 + QT fused multiply-adds per element instead of 2 QT operations -- with the row norms from prescale_kernel, and the table-driven
// exp2 above.  In float64 the kernel is bound by its VALU work, not by HBM (~40 issue slots per 8-byte element before, ~27 with XF).
// TRC > 0 (r03): the rows per workgroup as a compile-time constant, and the diagonal term HOISTED -- a wave-uniform test in front of the row
// loop sends only the workgroups the diagonal crosses (and a ragged last row block) through the loop with the per-row check.  Same-box
// (tests/probes/gram_variants.hip "cand"): +2.0 ... 2.5 % over the run-time form at 16 rows; 12 rows measured between equal and +4 %.
template <typename T, int QT, int KIND, int XF, int TRC>
__global__ __launch_bounds__(64) void gram_lean_kernel(const T* __restrict__ Xs_all, const T* __restrict__ Zs_all, T* __restrict__ K_all,
                                                       const T* __restrict__ var, const T* __restrict__ dadd_p,
                                                       const T* __restrict__ Xn_all, const T* __restrict__ Zn_all, GramLean<T> a) {
    constexpr int VEC = Vec16<T>::n;
    typedef typename Vec16<T>::type V;
    const int lane = threadIdx.x;
    const int s = blockIdx.z;
    __shared__ double tab[XF ? 64 : 1];
    // (forcing the whole argument segment into SGPRs up front with an `asm volatile("" :: "s"(...))` makes the compiler fetch the x rows
    //  with per-lane vector loads instead of s_loads: 6.4 -> 5.7 TB/s, tests/probes/gram_variants.hip "force")
    const int tr = TRC > 0 ? TRC : a.tr;
    const int64_t row0 = (int64_t)blockIdx.y * tr;
    const int64_t wcol0 = (int64_t)blockIdx.x * (64 * VEC);       // first column of the wave
    const int64_t col0 = wcol0 + (int64_t)lane * VEC;
    const T variance = (KIND == MXF_K_LINEAR) ? (T)1 : var[(int64_t)s * a.svar];
    const T dadd = a.dscale * dadd_p[(int64_t)s * a.sdadd] + a.jitter;
    if constexpr (XF) {
        tab[lane] = (double)variance * mxf_exp2_neg_f64(-(double)lane * (1.0 / 64.0));       // variance 2^(lane / 64)
        __syncthreads();
    }
    if (col0 >= a.N2) return;
    T z[VEC][QT];
    {
        const T* __restrict__ Zs = Zs_all + (int64_t)s * a.sZs + col0 * QT;
#pragma unroll
        for (int i = 0; i < VEC * QT; i += VEC)
            *reinterpret_cast<V*>(&z[0][0] + i) = *reinterpret_cast<const V*>(Zs + i);
    }
    const T* __restrict__ Xrows = Xs_all + (int64_t)s * a.sXs + row0 * QT;       // wave-uniform: scalar loads
    T* __restrict__ Krow = K_all + (int64_t)s * a.sK + row0 * a.ldk + col0;
    // a diagonal term exists (decided on the host; its value may still be 0) -- TRC form: ... and crosses this workgroup's rows x columns
    const bool diag_possible = a.has_diag != 0 && (TRC == 0 || (row0 < wcol0 + 64 * VEC && row0 + tr > wcol0));
    const int rmax = (a.N - row0) < tr ? (int)(a.N - row0) : tr;
    T zz[VEC];
    const T* __restrict__ Xn = nullptr;
    if constexpr (XF == 1) {     // t = -64 (|x|^2 + |z|^2 - 2 x.z) = fma(|x|^2, -64, -64 |z|^2) + sum_q x_q (128 z_q)
        // Both norms come from prescale_kernel (for a square Gram from the SAME array) and the scalings are powers of two, so
        // K[i][j] and K[j][i] go through identical roundings: the square Gram stays bit-symmetric.
        Xn = Xn_all + (int64_t)s * a.sXn + row0;
        const T* __restrict__ Zn = Zn_all + (int64_t)s * a.sZn + col0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            zz[v] = (T)-64 * Zn[v];
#pragma unroll
            for (int q = 0; q < QT; ++q) z[v][q] *= (T)128;
        }
    }
    auto do_row = [&](int r, auto with_diag) {
        T x[QT];
#pragma unroll
        for (int q = 0; q < QT; ++q) x[q] = Xrows[r * QT + q];
        T kv[VEC];
        if constexpr (XF == 1) {
            const T xn = Xn[r];
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                T acc = fma(xn, (T)-64, zz[v]);
#pragma unroll
                for (int q = 0; q < QT; ++q) acc = fma(x[q], z[v][q], acc);
                kv[v] = (T)exp2_64ths_tab((double)acc, tab);     // the table carries the variance
            }
        } else if constexpr (sizeof(T) == 4 && KIND != MXF_K_LINEAR) {
            typedef float f32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int p = 0; p < VEC / 2; ++p) {
                f32x2 acc2 = {0.f, 0.f};
#pragma unroll
                for (int q = 0; q < QT; ++q) {
                    const f32x2 xx = {(float)x[q], (float)x[q]};
                    const f32x2 zz = {(float)z[2 * p][q], (float)z[2 * p + 1][q]};
                    const f32x2 d = xx - zz;
                    acc2 = __builtin_elementwise_fma(d, d, acc2);
                }
                kv[2 * p] = cov_from<T, KIND>((T)acc2.x, variance);
                kv[2 * p + 1] = cov_from<T, KIND>((T)acc2.y, variance);
            }
        } else {
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                T acc = 0;
                if (KIND == MXF_K_LINEAR) {
#pragma unroll
                    for (int q = 0; q < QT; ++q) acc = fma(x[q], z[v][q], acc);
                } else {
#pragma unroll
                    for (int q = 0; q < QT; ++q) { T d = x[q] - z[v][q]; acc = fma(d, d, acc); }
                }
                kv[v] = cov_from<T, KIND>(acc, variance);
            }
        }
        // "+ noise / jitter on the diagonal": a scalar test (is this row inside the wave's column range?) guards the per-lane compares
        if constexpr (decltype(with_diag)::value) {
            if (diag_possible && (uint64_t)(row0 + r - wcol0) < (uint64_t)(64 * VEC)) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) if (col0 + v == row0 + r) {
                    if (XF == 1 && (a.has_diag & 2)) kv[v] = variance;     // k(x, x) = variance exactly (stationary.py:123-124), as the difference form gives
                    kv[v] += dadd;
                }
            }
        }
        V out;
        T* po = reinterpret_cast<T*>(&out);
#pragma unroll
        for (int v = 0; v < VEC; ++v) po[v] = kv[v];
        __builtin_nontemporal_store(out, reinterpret_cast<V*>(Krow + (int64_t)r * a.ldk));
    };
    if constexpr (TRC > 0) {
        if (rmax == TRC && !diag_possible) {
#pragma unroll 2
            for (int r = 0; r < TRC; ++r) do_row(r, std::false_type{});
        } else {
            for (int r = 0; r < rmax; ++r) do_row(r, std::true_type{});
        }
    } else {
#pragma unroll 2
        for (int r = 0; r < rmax; ++r) do_row(r, std::true_type{});
    }
}

// out[s][row][q] = X[s][row][q] * m_q for row < N, q < Q, else 0  (row < pad, q < QT);  m_q = c/l_q or sqrt(v_q)
// norms (optional): norms[s][row] = sum_q out[s][row][q]^2 (the QT threads of a row are neighbouring lanes)
template <typename T, int QT, int KIND>
__global__ void prescale_kernel(const T* __restrict__ X, int64_t sX, const T* __restrict__ ls, int64_t sls, int ard, int64_t N, int Q,
                                int64_t pad, T* __restrict__ out, T* __restrict__ norms = nullptr, int raw = 0,
                                const T* __restrict__ centre = nullptr, int64_t sC = 0) {
    const int s = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pad * QT) return;
    const int64_t row = i / QT;
    const int q = (int)(i % QT);
    T v = (T)0;
    if (row < N && q < Q) {
        const T l = ls[(int64_t)s * sls + (ard ? q : 0)];
        const T m = raw ? (T)1 : ((KIND == MXF_K_LINEAR) ? t_sqrt<T>(l) : coord_scale<T, KIND>() / l);      // raw: the padded copy only
        // centre (stationary kinds): one point subtracted from BOTH operands before scaling -- x / l rounds proportionally to |x| / l, so inputs
        // at an offset of 1000 units cost 4e-5 on K in float32 where centred inputs cost 1e-7 (tests/probes/offset_gram.py)
        v = (X[(int64_t)s * sX + row * Q + q] - (centre ? centre[(int64_t)s * sC + q] : (T)0)) * m;
    }
    out[(int64_t)s * pad * QT + i] = v;
    if (norms) {
        T n2 = v * v;
#pragma unroll
        for (int o = QT / 2; o > 0; o >>= 1) n2 += __shfl_xor(n2, o, 64);
        if (q == 0) norms[(int64_t)s * pad + row] = n2;
    }
}

// generic fallback for Q > 16: one output per thread, q-loop over global memory
template <typename T, int KIND>
__global__ __launch_bounds__(256) void gram_generic_kernel(GramArgs<T> a) {
    const int MODE = a.mode;
    const int s = blockIdx.z;
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= a.N2) return;
    const T* X2 = a.X2 + (int64_t)s * a.sX2 + col * a.Q;
    const T* ls = a.ls + (int64_t)s * a.sls;
    const T variance = (KIND == MXF_K_LINEAR) ? (T)1 : a.var[(int64_t)s * a.svar];
    for (int64_t row = blockIdx.y; row < a.N; row += gridDim.y) {      // grid.y is capped at 65535 row slots
        const T* X = a.X + (int64_t)s * a.sX + row * a.Q;
        T acc = 0;
        if (KIND == MXF_K_LINEAR) {
            for (int q = 0; q < a.Q; ++q) acc = fma(X[q] * ls[a.ard ? q : 0], X2[q], acc);
        } else if (KIND != MXF_K_BIAS && KIND != MXF_K_WHITE) {
            for (int q = 0; q < a.Q; ++q) { T d = (X[q] - X2[q]) * (coord_scale<T, KIND>() / ls[a.ard ? q : 0]); acc = fma(d, d, acc); }
        }
        T k;
        if (KIND == MXF_K_BIAS) k = variance;
        else if (KIND == MXF_K_WHITE) k = (a.square && row == col) ? variance : (T)0;
        else k = cov_from<T, KIND>(acc, variance);
        if (a.square && row == col) k += (a.dadd ? a.dadd[(int64_t)s * a.sdadd] : (T)0) + a.jitter;
        T* dst = a.K + (int64_t)s * a.sK + row * a.ldk + col;
        if (MODE == MXF_ACC_ADD) k = *dst + k;
        if (MODE == MXF_ACC_MUL) k = *dst * k;
        *dst = k;
    }
}

// one operand's padded copy: S sample copies (grid.y) of pad rows
template <typename T, int QT, int KIND>
void prescale(hipStream_t st, int S, const T* X, int64_t sX, const T* ls, int64_t sls, int ard, int64_t N, int Q, int64_t pad, T* out, T* norms,
              int raw, const T* centre, int64_t sC) {
    hipLaunchKernelGGL((prescale_kernel<T, QT, KIND>), dim3((unsigned)((pad * QT + 255) / 256), (unsigned)S), dim3(256), 0, st, X, sX, ls, sls, ard,
                       N, Q, pad, out, norms, raw, centre, sC);
}

// buf: the scratch the plan laid out (nullptr: the path takes none)
template <typename T>
GramArgs<T> gram_args(const MxfGram& d, const GramPlan& p, const T* buf, bool vec_ok) {
    GramArgs<T> a{};
    a.square = d.X2 == nullptr;
    a.X = (const T*)d.X; a.X2 = a.square ? a.X : (const T*)d.X2; a.sX = d.sX; a.sX2 = a.square ? d.sX : d.sX2;
    a.ls = (const T*)d.ls; a.sls = d.sls; a.ard = d.ard; a.var = (const T*)d.var; a.svar = d.svar;
    a.dadd = (const T*)d.diag_add; a.sdadd = d.sdiag; a.jitter = (T)d.jitter;
    if (buf) { a.Xs = buf + p.xs; a.Zs = buf + p.zs; a.sXs = p.sxs; a.sZs = p.szs; }
    a.K = (T*)d.K.p; a.ldk = d.K.ld; a.sK = d.K.stride;
    a.N = d.N; a.N2 = a.square ? d.N : d.N2; a.Q = d.Q;
    a.mode = d.mode; a.vecst = vec_ok; a.tr = p.tr; a.ncb = p.ncb;
    return a;
}

// the coordinate kernels (Q <= 16): the pre-scaled copies into the handle's Gram scratch, then the plan's path
template <typename T, int KIND, int QT>
int gram_coord(mxf_ctx* h, hipStream_t st, const MxfGram& d, const GramPlan& p, bool vec_ok) {
    using namespace mxf_gram_tiles;
    constexpr bool RBF = KIND == MXF_K_RBF;
    constexpr int XF = (RBF && sizeof(T) == 8) ? 1 : 0, TRC = RBF ? (sizeof(T) == 4 ? TR_RBF_F32 : TR_RBF_F64) : 0;      // gram_lean_kernel's form of this (T, KIND)
    T* buf = nullptr;
    if (p.bytes) {
        buf = (T*)mxf_gram_ws(h, p.bytes);
        if (!buf) MXF_FAIL(h, -4, "mxf_gram: cannot allocate %zu bytes for the pre-scaled coordinates", p.bytes);
    }
    const GramArgs<T> a = gram_args<T>(d, p, buf, vec_ok);
    const bool xf = p.path == MXF_GRAM_LEAN_XF;
    if (buf) {
        const T* cen = p.centre == MXF_GRAM_CENTRE_NONE ? nullptr : (p.centre == MXF_GRAM_CENTRE_X2 ? a.X2 : a.X);
        prescale<T, QT, KIND>(st, p.Sx, a.X, a.sX, a.ls, a.sls, a.ard, a.N, a.Q, p.padx, buf + p.xs, xf ? buf + p.xn : nullptr, 0, cen, p.scen);
        if (!a.square)
            prescale<T, QT, KIND>(st, p.Sz, a.X2, a.sX2, a.ls, a.sls, a.ard, a.N2, a.Q, p.padc, buf + p.zs, xf ? buf + p.zn : nullptr, 0, cen, p.scen);
    }
    const dim3 g(p.grid[0], p.grid[1], p.grid[2]);
    if (p.path == MXF_GRAM_LEAN || xf) {
        const bool hd = a.square && a.dadd != nullptr;
        GramLean<T> l;
        l.N = a.N; l.N2 = a.N2; l.ldk = a.ldk; l.sXs = a.sXs; l.sZs = a.sZs; l.sK = a.sK; l.svar = a.svar; l.sXn = p.sxn; l.sZn = p.szn;
        l.tr = a.tr; l.has_diag = p.has_diag;
        l.sdadd = hd ? a.sdadd : 0; l.dscale = hd ? (T)1 : (T)0; l.jitter = a.square ? a.jitter : (T)0;
        const T* dptr = hd ? a.dadd : (a.var ? a.var : a.Xs);          // any readable word when there is no diagonal term
        hipLaunchKernelGGL((gram_lean_kernel<T, QT, KIND, XF, TRC>), g, dim3(64), 0, st, a.Xs, a.Zs, a.K, a.var, dptr,
                           xf ? (const T*)(buf + p.xn) : nullptr, xf ? (const T*)(buf + p.zn) : nullptr, l);
    } else if (p.path == MXF_GRAM_COORD_FAST) hipLaunchKernelGGL((gram_kernel<T, QT, KIND, true>), g, dim3(64), 0, st, a, a.Xs, a.Zs, a.K);
    else hipLaunchKernelGGL((gram_kernel<T, QT, KIND, false>), g, dim3(64), 0, st, a, a.Xs, a.Zs, a.K);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

template <typename T, int KIND>
int launch_kind(mxf_ctx* h, hipStream_t st, const MxfGram& d) {
    constexpr int VEC = Vec16<T>::n;
    if (d.mode < 0 || d.mode > 2) MXF_FAIL(h, -2, "mxf_gram: bad mode %d", d.mode);
    const bool square = d.X2 == nullptr;
    const bool vec_ok = (d.K.ld % VEC == 0) && (d.K.stride % VEC == 0) && (((uintptr_t)d.K.p) % 16 == 0);
    const GramPlan p = gram_plan(KIND, sizeof(T), d.S, d.N, d.N2, d.Q, square, d.sX, d.sX2, d.sls, vec_ok, d.mode,
                                 square && (d.diag_add != nullptr || (T)d.jitter != (T)0));
    if (p.refusal) MXF_FAIL(h, p.rc, "mxf_gram: %s", p.refusal);
    if (p.path == MXF_GRAM_GENERIC) {
        hipLaunchKernelGGL((gram_generic_kernel<T, KIND>), dim3(p.grid[0], p.grid[1], p.grid[2]), dim3(mxf_gram_tiles::GENERIC_COLS), 0, st,
                           gram_args<T>(d, p, nullptr, vec_ok));
        MXF_LAUNCH_CHECK(h);
        return 0;
    }
    return dispatch<2, 4, 8, 16>(p.QT, [&](auto qt) { return gram_coord<T, KIND, decltype(qt)::value>(h, st, d, p, vec_ok); });
}

template <typename T>
int gram_typed(mxf_ctx* h, hipStream_t st, const MxfGram& d) {
    const int rc = dispatch<MXF_K_RBF, MXF_K_MATERN12, MXF_K_MATERN32, MXF_K_MATERN52, MXF_K_LINEAR, MXF_K_BIAS, MXF_K_WHITE>(
        d.kind, [&](auto kind) { return launch_kind<T, decltype(kind)::value>(h, st, d); });
    if (rc == NO_CASE) MXF_FAIL(h, -2, "mxf_gram: unknown kernel kind %d", d.kind);
    return rc;
}

// ---- Gram matrix written as split planes (the f16x2 operand format of gemm_split.hip: two scaled f16 terms) ---------------------------
// operand element (r, k) = cov(xmin[r], xmaj[k]); plane p element (r, k) at ((k / 16) * R + r) * 16 + k % 16.
// HBM-write bound: 4 bytes per element (8.6 GB at M = 1024 x 2.1 M columns).
typedef unsigned int gp_u32x4 __attribute__((ext_vector_type(4)));
// The planes hold cov / variance * 2^14 as hi + lo (f16 each); the consumer multiplies by variance * 2^-14 (unit-variance covariances
// are <= 1, so the format's power-of-two scale is known without a reduction).
// PT > 0: the same pass also forms  U[p][r] = sum_k w[k][p] cov(xmin[r], xmaj[k])  (the row w^T Kuf of the SVGP step, svgp_regression.py:98:
// Kuf^T Kuu^-1 mu) from the f32 covariances it has in registers -- the separate 8.6 GB read of the planes that product used to cost
// (1.45 ms at the bench size) is gone.  Needs grid.y == 1 (every block walks all k blocks of its rows).
// (r03) ONE-WAVE workgroups, lane <-> minor index r (64 rows per wave), the sixteen major points of a k block wave-uniform
// (scalar loads, no LDS staging, no barrier -- the layout of gram_lean_kernel).  A lane evaluates the 16 covariances of its row, i.e. BOTH
// 16-byte halves of its 32-byte piece; v_permlane32_swap then trades half 1 of the rows of lanes 0..31 for half 0 of the rows of lanes
// 32..63, so each of the two store instructions per plane covers 1 KB CONTIGUOUS (32 rows x 32 bytes).  (Without the swap each store
// covers 16-byte pieces at a 32-byte stride: measured r02, 30 -> 40 ms per step.)  hi + lo come from the packed conversions
// (v_cvt_pk_f16_f32: a plane's dword directly); the fused row U sums its sixteen terms per k block in index order.
// Measured (planes_store.hip): 1.82 / 1.69 ms for the two 8.6 GB passes of the bench step, the same as the r02 staged kernel (LDS, 256
// threads, a thread <-> (row, k half)) -- neither the LDS staging nor the VALU count (16 -> 14 instructions per covariance here) is what bounds them; the store-only twin
// of the same pattern takes 1.45 - 1.65 ms alone, memset 1.36 ms; PLAIN instead of non-temporal stores: 2.1 - 2.4 ms inside the step.
// (r04) The squared distance as sum_q ((x_q - z_q)^2) (c / l_q)^2 from the RAW coordinates -- difference first, scale after -- instead of
// the difference of pre-scaled coordinates: the rounding of x / l (2^-24 |x / l|) no longer enters r^2 of NEAR pairs, the ones that carry the
// covariance.  At length-scale 0.2 on [-2, 2] (a deep GP's hidden layer) the pre-scaled form's Gram error, amplified by |T| ~ sqrt(cond) in
// q_n = k_n . T_n, was 2/3 of the whitened tier's ELBO error (3.9e-5 -> 4e-6 relative; tests/test_gpu_f32_guard.py two-layer case).
// One more packed multiply per two coordinates.
// MXF_PLANES_WAVES (compile time, r05 experiment): at most this many waves of the planes pass per SIMD.  Its one-wave workgroups otherwise take
// every wave slot (and with ~64 registers each the whole register file) of every CU, and the float64 workgroups of the Kuu chain that runs
// next to it (4 waves of ~128 registers, tens of KB of LDS) wait for a CU to drain by chance -- the r05 timelines show a 60 us GEMM of
// that chain taking 1.26 ms next to this pass.
#ifndef MXF_PLANES_WAVES
#define MXF_PLANES_WAVES 0
#endif
#if MXF_PLANES_WAVES > 0
#define MXF_PLANES_OCC __attribute__((amdgpu_waves_per_eu(MXF_PLANES_WAVES, MXF_PLANES_WAVES)))
#else
#define MXF_PLANES_OCC
#endif
template <int QT, int KIND, int PT>
__global__ __launch_bounds__(64) MXF_PLANES_OCC void gram_planes_lean_kernel(int64_t R, int64_t Kn, const float* __restrict__ Xmin_s, const float* __restrict__ Xmaj_s,
                                                              const float* __restrict__ var, unsigned short* __restrict__ P, int64_t pstride,
                                                              int kb_per_block, const float* __restrict__ wk, int Pw, float* __restrict__ U,
                                                              int64_t ldU, const float* __restrict__ ls, int ard, int Q,
                                                              const float* __restrict__ majs, const float* __restrict__ mins, int64_t period) {
    // Xmin_s / Xmaj_s: the RAW coordinates, zero-padded to QT (prescale_kernel raw); ls, ard, Q: the length-scales the differences are scaled by.
    // majs / mins (optional; the streaming heteroscedastic SVGP bound, svgp_regression.py:61-67): every covariance is multiplied by
    // majs[major index % period] (wave-uniform) and / or mins[minor index % period] (per lane) before it is split into planes -- and before
    // it enters the fused row U -- i.e. the planes hold K diag(s) resp. diag(s) K for per-row weights s <= 1
    const int lane = threadIdx.x;
    float s2[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) {
        const float m = q < Q ? coord_scale<float, KIND>() / ls[ard ? q : 0] : 0.f;      // wave-uniform: scalar loads
        s2[q] = m * m;
    }
    const int64_t bxi = blockIdx.x;
    const int byi = blockIdx.y;
    const int64_t r0 = bxi * 64, r = r0 + lane;
    float z[QT];
#pragma unroll
    for (int q = 0; q < QT; q += 4) *reinterpret_cast<f32x4_t*>(&z[q]) = *reinterpret_cast<const f32x4_t*>(Xmin_s + r * QT + q);   // padded
    float mscale = 1.f;
    if (mins) mscale = mins[(r < R ? r : R - 1) % period];
    float uacc[PT > 0 ? PT : 1];
#pragma unroll
    for (int p = 0; p < (PT > 0 ? PT : 1); ++p) uacc[p] = 0.f;
    const int64_t K16 = (Kn + 15) / 16;
    const int64_t kb_begin = (int64_t)byi * kb_per_block;
    const int64_t kb_end = (kb_begin + kb_per_block) < K16 ? (kb_begin + kb_per_block) : K16;
    // store targets after the swap: instruction 1 <-> row r0 + lane % 32, instruction 2 <-> 32 rows further; the half is lane / 32
    const int64_t ra = r0 + (lane & 31), rb = ra + 32;
    const int hsel = lane >> 5;
    auto kb_body = [&](int64_t kb, auto full_c) {
        constexpr bool FULL = decltype(full_c)::value;
        const float* __restrict__ xk = Xmaj_s + kb * 16 * QT;                    // wave-uniform: scalar loads
        unsigned hi[8], lo[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            typedef float f32x2 __attribute__((ext_vector_type(2)));
            typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
            f32x2 kv2;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int nl = 2 * j + e;
                f32x2 acc2 = {0.f, 0.f};
#pragma unroll
                for (int q = 0; q < QT; q += 2) {
                    const f32x2 xx = {xk[nl * QT + q], xk[nl * QT + q + 1]};
                    const f32x2 zz = {z[q], z[q + 1]};
                    const f32x2 d = xx - zz;
                    const f32x2 ss = {s2[q], s2[q + 1]};
                    acc2 = __builtin_elementwise_fma(d * d, ss, acc2);
                }
                const float red = acc2.x + acc2.y;
                float kv = (FULL || kb * 16 + nl < Kn) ? cov_from<float, KIND>(red, 16384.f) : 0.f;
                if (majs) { const int64_t km = FULL ? kb * 16 + nl : ((kb * 16 + nl < Kn) ? kb * 16 + nl : Kn - 1); kv *= majs[km % period]; }
                if (mins) kv *= mscale;
                if (PT > 0) {
                    const int64_t kk = FULL ? kb * 16 + nl : ((kb * 16 + nl < Kn) ? kb * 16 + nl : Kn - 1);     // (kv == 0 beyond Kn)
#pragma unroll
                    for (int p = 0; p < PT; ++p) {
                        const float wv = (PT == 1 || p < Pw) ? wk[kk * Pw + (PT == 1 ? 0 : p)] : 0.f;       // wave-uniform
                        uacc[p] = fmaf(wv, kv, uacc[p]);
                    }
                }
                kv2[e] = kv;
            }
            // hi + lo two values at a time: the packed conversions (v_cvt_pk_f16_f32) deliver the dword of the plane directly
            const f16x2 fh = __builtin_convertvector(kv2, f16x2);
            const f16x2 fl = __builtin_convertvector(kv2 - __builtin_convertvector(fh, f32x2), f16x2);
            const unsigned hh = __builtin_bit_cast(unsigned, fh), ll = __builtin_bit_cast(unsigned, fl);
            hi[j] = hh; lo[j] = ll;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(hi[i]), "+v"(hi[4 + i]));
            asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(lo[i]), "+v"(lo[4 + i]));
        }
        unsigned short* base = P + (kb * R) * 16 + hsel * 8;
        if (ra < R) {
            const gp_u32x4 vh = {hi[0], hi[1], hi[2], hi[3]}, vl = {lo[0], lo[1], lo[2], lo[3]};
            __builtin_nontemporal_store(vh, reinterpret_cast<gp_u32x4*>(base + ra * 16));
            __builtin_nontemporal_store(vl, reinterpret_cast<gp_u32x4*>(base + ra * 16 + pstride));
        }
        if (rb < R) {
            const gp_u32x4 vh = {hi[4], hi[5], hi[6], hi[7]}, vl = {lo[4], lo[5], lo[6], lo[7]};
            __builtin_nontemporal_store(vh, reinterpret_cast<gp_u32x4*>(base + rb * 16));
            __builtin_nontemporal_store(vl, reinterpret_cast<gp_u32x4*>(base + rb * 16 + pstride));
        }
    };
    const int64_t kb_full = Kn / 16 < kb_end ? Kn / 16 : kb_end;           // k blocks whose sixteen major points all exist
    int64_t kb = kb_begin;
    for (; kb < kb_full; ++kb) kb_body(kb, std::true_type{});
    for (; kb < kb_end; ++kb) kb_body(kb, std::false_type{});
    if (PT > 0) {
        const float sc = var[0] * (1.f / 16384.f);
        if (r < R) {
#pragma unroll
            for (int p = 0; p < PT; ++p) if (p < Pw) U[(int64_t)p * ldU + r] = uacc[p] * sc;
        }
    }
}

// the padded RAW coordinates of both operands into the caller's scratch (difference-then-scale distances, above), then the pass
template <int KIND, int QT>
int gram_planes_launch(mxf_ctx* h, hipStream_t st, const MxfGramPlanes& d, const GramPlanesPlan& p) {
    float* bmin = d.scratch;
    float* bmaj = bmin + (size_t)p.padr * QT;
    prescale<float, QT, KIND>(st, 1, d.Xmin, 0, d.ls, 0, d.ard, d.R, d.Q, p.padr, bmin, nullptr, 1, nullptr, 0);
    prescale<float, QT, KIND>(st, 1, d.Xmaj, 0, d.ls, 0, d.ard, d.Kn, d.Q, p.padk, bmaj, nullptr, 1, nullptr, 0);
    dispatch<0, 1, 8>(p.PT, [&](auto pt) {
        hipLaunchKernelGGL((gram_planes_lean_kernel<QT, KIND, decltype(pt)::value>), dim3(p.grid[0], p.grid[1]), dim3(64), 0, st, d.R, d.Kn,
                           (const float*)bmin, (const float*)bmaj, d.var, d.planes, d.pstride, p.kbpb, d.w, d.Pw, d.U, d.ldU, d.ls, d.ard, d.Q,
                           d.majs, d.mins, d.period);
        return 0;
    });
    MXF_LAUNCH_CHECK(h);
    return 0;
}

}  // namespace

int mxf_gram_internal(mxf_ctx* h, hipStream_t st, const MxfGram& d) {
    if (d.S <= 0 || d.N < 0 || d.N2 < 0 || d.Q <= 0)
        MXF_FAIL(h, -2, "mxf_gram: bad shape S=%d N=%lld N2=%lld Q=%d", d.S, (long long)d.N, (long long)d.N2, d.Q);
    const int64_t n2 = d.X2 ? d.N2 : d.N;
    if (d.N == 0 || n2 == 0) return 0;
    if (!d.X || !d.K.p) MXF_FAIL(h, -2, "mxf_gram: null X or K_out");
    if (d.kind != MXF_K_BIAS && d.kind != MXF_K_WHITE && !d.ls) MXF_FAIL(h, -2, "mxf_gram: null lengthscale/variances");
    if (d.kind != MXF_K_LINEAR && !d.var) MXF_FAIL(h, -2, "mxf_gram: null variance");
    if (d.K.ld < n2) MXF_FAIL(h, -2, "mxf_gram: ldk < N2");
    if (d.S > 65535) MXF_FAIL(h, -3, "mxf_gram: S too large");
    if (d.dtype == MXF_F32) return gram_typed<float>(h, st, d);
    if (d.dtype == MXF_F64) return gram_typed<double>(h, st, d);
    MXF_FAIL(h, -2, "mxf_gram: bad dtype %d", d.dtype);
}

extern "C" int mxf_gram(mxf_handle h, int kind, int dtype, int S, int64_t N, int64_t N2, int Q,
                        const void* X, int64_t strideS_X, const void* X2, int64_t strideS_X2,
                        const void* lengthscale, int ard, int64_t strideS_ls,
                        const void* variance, int64_t strideS_var,
                        const void* diag_add, int64_t strideS_diag, double jitter, int mode,
                        void* K_out, int64_t ldk, int64_t strideS_K, void* stream) {
    if (!h) return -1;
    return mxf_gram_internal(h, (hipStream_t)stream,
                             {.kind = kind, .dtype = dtype, .S = S, .N = N, .N2 = N2, .Q = Q, .X = X, .sX = strideS_X, .X2 = X2, .sX2 = strideS_X2,
                              .ls = lengthscale, .ard = ard, .sls = strideS_ls, .var = variance, .svar = strideS_var, .diag_add = diag_add,
                              .sdiag = strideS_diag, .jitter = jitter, .mode = mode, .K = {K_out, ldk, strideS_K}});
}

// Gram matrix cov(xmin[r], xmaj[k]) (r < R, k < Kn) as split planes in the f16x2 format (float32 inputs, stationary kernels); see
// gram_planes_lean_kernel.  planes: 2 * pstride elements, pstride = mxf_split_plane_elems(R, Kn).
size_t mxf_gram_planes_scratch_bytes(int64_t R, int64_t Kn, int Q) { return gram_planes_scratch_bytes(R, Kn, Q); }

int mxf_gram_planes_internal(mxf_ctx* h, hipStream_t st, const MxfGramPlanes& d) {
    if (d.R <= 0 || d.Kn <= 0) return 0;
    if (!d.scratch) MXF_FAIL(h, -2, "gram planes: scratch of mxf_gram_planes_scratch_bytes() bytes required");
    const GramPlanesPlan p = gram_planes_plan(d.R, d.Kn, d.Q, d.U != nullptr, d.w != nullptr, d.Pw, MXF_KNOB("MXF_PLANES_KB", 8));
    if (p.refusal) MXF_FAIL(h, p.rc, "gram planes: %s", p.refusal);
    const int rc = dispatch<MXF_K_RBF, MXF_K_MATERN12, MXF_K_MATERN32, MXF_K_MATERN52>(d.kind, [&](auto kind) {
        return dispatch<8, 16>(p.QT, [&](auto qt) { return gram_planes_launch<decltype(kind)::value, decltype(qt)::value>(h, st, d, p); });
    });
    if (rc == NO_CASE) MXF_FAIL(h, -2, "gram planes: stationary kernels only (kind %d)", d.kind);
    return rc;
}

// C ABI of the planes pass (include/mxf_gp.h): argument checks, the padded raw coordinates in the handle's Gram scratch (where mxf_gram keeps
// its pre-scaled ones), then mxf_gram_planes_internal as the SVGP step calls it
extern "C" int mxf_gram_planes(mxf_handle h, int kind, int64_t R, int64_t Kn, int Q, const void* Xmin, const void* Xmaj,
                               const void* lengthscale, int ard, const void* variance, void* planes, const void* w, int Pw, void* U,
                               int64_t ldU, const void* majs, const void* mins, int64_t period, void* stream) {
    if (!h) return -1;
    if (R <= 0 || Kn <= 0 || Q <= 0) MXF_FAIL(h, -2, "mxf_gram_planes: bad shape R=%lld Kn=%lld Q=%d", (long long)R, (long long)Kn, Q);
    if (Q > 16) MXF_FAIL(h, -3, "mxf_gram_planes: Q = %d > 16 not supported", Q);
    if (kind != MXF_K_RBF && kind != MXF_K_MATERN12 && kind != MXF_K_MATERN32 && kind != MXF_K_MATERN52)
        MXF_FAIL(h, -2, "mxf_gram_planes: stationary kernels only (kind %d)", kind);
    if (!Xmin || !Xmaj || !lengthscale || !variance || !planes) MXF_FAIL(h, -2, "mxf_gram_planes: null Xmin, Xmaj, lengthscale, variance or planes");
    if (((uintptr_t)planes) % 16 != 0) MXF_FAIL(h, -2, "mxf_gram_planes: planes must be 16-byte aligned");
    if ((w != nullptr) != (U != nullptr)) MXF_FAIL(h, -2, "mxf_gram_planes: w and U go together");
    if (w && (Pw < 1 || Pw > 8)) MXF_FAIL(h, -3, "mxf_gram_planes: the fused row needs 1 <= Pw <= 8 (got %d)", Pw);
    if (w && ldU < R) MXF_FAIL(h, -2, "mxf_gram_planes: ldU < R");
    if (period < 1) MXF_FAIL(h, -2, "mxf_gram_planes: period %lld < 1", (long long)period);
    const size_t need = mxf_gram_planes_scratch_bytes(R, Kn, Q);
    float* scratch = (float*)mxf_gram_ws(h, need);
    if (!scratch) MXF_FAIL(h, -4, "mxf_gram_planes: cannot allocate %zu bytes for the padded coordinates", need);
    return mxf_gram_planes_internal(h, (hipStream_t)stream,
                                    {.kind = kind, .R = R, .Kn = Kn, .Q = Q, .Xmin = (const float*)Xmin, .Xmaj = (const float*)Xmaj,
                                     .ls = (const float*)lengthscale, .ard = ard, .var = (const float*)variance, .planes = (unsigned short*)planes,
                                     .pstride = (int64_t)mxf_split_plane_elems(R, Kn), .scratch = scratch, .w = (const float*)w, .Pw = w ? Pw : 0,
                                     .U = (float*)U, .ldU = ldU, .majs = (const float*)majs, .mins = (const float*)mins, .period = period});
}
