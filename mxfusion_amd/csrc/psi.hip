// RBF psi statistics of a Gaussian input x_n ~ N(mu_n, diag(s_n)) and their reverse mode (gfx950); the element math is psi.h.
//   Psi1[m,n] = E[k(z_m, x_n)]   (M, N)          Psi2[m,m'] = sum_n E[k(z_m, x_n) k(x_n, z_m')]   (M, M)
// No reference counterpart: the reference averages its bound over draws of x.
//
// Psi2 is a reduction over N M (M + 1) / 2 terms of 3 Q multiply-adds and one exponential each, so the vector ALU bounds it, and nothing of
// that size is stored.  Two decompositions, both free of LDS traffic in the inner loop:
//   pair-owned (psi2_pairs_kernel: the forward pass, and dZ / the D part of dl / dvar of the reverse pass): a thread owns one (m, m' <= m),
//     a workgroup a 16 x 16 tile of the lower triangle and a chunk of the rows; the row index is uniform over the wavefront, so a row's
//     constants (mu, 1 / (2 s + l^2), prod (1 + 2 s / l^2)^-1/2, written once by psi_prep_kernel) arrive as scalar loads.  The part of the
//     exponent that depends on (m, m') only, and var^2, multiply the finished sum once.
//   row-owned (psi2_bwd_rows_kernel, psi1_*_kernel: dmu, ds and the row part of dl): a thread owns one row n, its constants live in
//     registers, and the pairs (z / 2 padded to QP, and the weight matrix W[m,m'] = (G2 + G2^T) var^2 exp(-D), halved on the diagonal, of
//     psi2_weight_kernel) arrive as scalar loads.  psi2n is recomputed in both passes and never stored.  psi2_quad_rows_kernel is the
//     forward-only sibling: R[n,j] = sum_{m,m'} A_j[m,m'] psi2n[n,m,m'] with PSI_JB weights per pair in one scalar load, no M_q / U_q sums.
// Rows (pair-owned) and m (row-owned) are split over grid.y until about 2048 workgroups exist, so a small M or a small N still fills the
// device.  Every sum that crosses workgroups is a double, for either dtype: a thread sums at most PSI_ROWS rows (or one m's m' <= m) in T,
// adds that to a double register, and ends with one atomic into a double accumulator -- zeroed handle scratch (Psi2, float32 gradients:
// folded into the caller's buffer with one rounding) or the caller's float64 buffer itself.  With one chunk an element has one writer.
// Psi2 is written from its lower triangle to both halves by one kernel: bitwise symmetric.
#include "common.h"
#include "fused_plan.h"      // PSI_*: the tile sizes; psi_fwd_plan, psi_bwd_plan, psi_quad_plan
#include "shared_grad.h"
#define MXF_PSI_EXP(T, x) t_exp<T>(x)
#include "psi.h"

namespace {

template <typename T>
struct PsiOps {
    int S; int64_t N, M; int Q, ard;
    const T* mu; int64_t ss_mu;
    const T* s; int64_t ss_s;
    const T* Z; int64_t ss_Z;
    const T* ls; int64_t ss_ls;
    const T* var; int64_t ss_var;
};

template <int QP> constexpr int psi_rs() { return 2 * QP + 2; }      // a row of psi_prep_kernel: mu[QP], a2[QP], c2, 0

template <typename T, int QP>
__device__ __forceinline__ void psi_l2(const PsiOps<T>& o, int64_t s, T* l2) {
    const T* ls = o.ls + s * o.ss_ls;
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        const T l = q < o.Q ? ls[o.ard ? q : 0] : (T)1;
        l2[q] = l * l;
    }
}

// a thread's own row: mu, s, a = 1 / (k s + l2) and c; the padding is mu = s = 0, l2 = 1
template <typename T, int QP>
__device__ __forceinline__ void psi_own_row(const PsiOps<T>& o, int k, int64_t s, int64_t n, const T* l2, T* mu, T* sv, T* a, T& c) {
    const T *pm = o.mu + s * o.ss_mu + n * o.Q, *ps = o.s + s * o.ss_s + n * o.Q;
    c = 1;
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        mu[q] = q < o.Q ? pm[q] : (T)0;
        sv[q] = q < o.Q ? ps[q] : (T)0;
        T cq;
        psi_row_q<T>(k, sv[q], l2[q], a[q], cq);
        c *= cq;
    }
}

// rows (S, N, 2 QP + 2): the Psi2 constants of every row; zf, zh (S, M, QP): z and z / 2 padded with zeros
template <typename T, int QP>
__global__ __launch_bounds__(256) void psi_prep_kernel(PsiOps<T> o, T* __restrict__ rows, T* __restrict__ zf, T* __restrict__ zh) {
    const int64_t per = o.N + o.M, total = (int64_t)o.S * per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / per, r = i - s * per;
        if (r < o.N) {
            if (!rows) continue;
            T l2[QP], mu[QP], sv[QP], a[QP], c;
            psi_l2<T, QP>(o, s, l2);
            psi_own_row<T, QP>(o, 2, s, r, l2, mu, sv, a, c);
            T* out = rows + (s * o.N + r) * psi_rs<QP>();
#pragma unroll
            for (int q = 0; q < QP; ++q) { out[q] = mu[q]; out[QP + q] = a[q]; }
            out[2 * QP] = c;
            out[2 * QP + 1] = 0;
        } else {
            const int64_t m = r - o.N;
            const T* z = o.Z + s * o.ss_Z + m * o.Q;
#pragma unroll
            for (int q = 0; q < QP; ++q) {
                const T v = q < o.Q ? z[q] : (T)0;
                zf[(s * o.M + m) * QP + q] = v;
                zh[(s * o.M + m) * QP + q] = (T)0.5 * v;
            }
        }
    }
}

template <typename T, int QP>
__global__ __launch_bounds__(PSI_R1) void psi1_fwd_kernel(PsiOps<T> o, const T* __restrict__ zf, T* __restrict__ out) {
    const int64_t s = blockIdx.z, n = (int64_t)blockIdx.x * PSI_R1 + threadIdx.x;
    const bool live = n < o.N;
    T l2[QP], mu[QP], sv[QP], a[QP], c;
    psi_l2<T, QP>(o, s, l2);
    psi_own_row<T, QP>(o, 1, s, live ? n : o.N - 1, l2, mu, sv, a, c);
    c *= o.var[s * o.ss_var];
    const int64_t m0 = (int64_t)blockIdx.y * PSI_MCH, m1 = m0 + PSI_MCH < o.M ? m0 + PSI_MCH : o.M;
    for (int64_t m = m0; m < m1; ++m) {
        T ae[QP];
        const T v = psi1_term<T, QP>(mu, a, c, zf + (s * o.M + m) * QP, ae);
        if (live) out[(s * o.M + m) * o.N + n] = v;
    }
}

// the tile (ti >= tj) of the lower triangle with number p = ti (ti + 1) / 2 + tj
__device__ __forceinline__ void psi_tile_of(int64_t p, int& ti, int& tj) {
    int64_t t = (int64_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (t * (t + 1) / 2 > p) --t;
    while ((t + 1) * (t + 2) / 2 <= p) ++t;
    ti = (int)t;
    tj = (int)(p - t * (t + 1) / 2);
}

// Forward: acc2[s][m][m'] += var^2 exp(-D) sum_n term over the rows of chunk blockIdx.y, m' <= m.
// Reverse (BWD): with W = var^2 exp(-D) (G2[m,m'] + G2[m',m]), G2[m,m] on the diagonal, P = sum_n term and A_q = sum_n term a_q e_q,
//   dZ[m] += W (A - P dz / (2 l2)), dZ[m'] += W (A + P dz / (2 l2)), dl2 += W P dz^2 / (4 l2^2), dvar += 2 W P / var
// summed over the workgroup in LDS, then one atomic per element.
template <typename T, int QP, bool BWD>
__global__ __launch_bounds__(256) void psi2_pairs_kernel(PsiOps<T> o, const T* __restrict__ rows, const T* __restrict__ zh, int rchunks,
                                                         double* __restrict__ acc2, const T* __restrict__ G2, double* __restrict__ dZacc,
                                                         int own_Z, double* __restrict__ dl2acc, double* __restrict__ dvacc) {
    __shared__ double lz[2][PSI_TILE][QP], ll[QP], red[16];
    int ti, tj;
    psi_tile_of(blockIdx.x, ti, tj);
    const int64_t s = blockIdx.z;
    const int tx = threadIdx.x & (PSI_TILE - 1), ty = threadIdx.x / PSI_TILE;
    const int64_t m = (int64_t)ti * PSI_TILE + ty, m2 = (int64_t)tj * PSI_TILE + tx;
    const bool live = m < o.M && m2 <= m;
    const T *pz = zh + (s * o.M + (m < o.M ? m : o.M - 1)) * QP, *pz2 = zh + (s * o.M + (m2 < o.M ? m2 : o.M - 1)) * QP;
    T zbar[QP], dz[QP];
#pragma unroll
    for (int q = 0; q < QP; ++q) {
        zbar[q] = pz[q] + pz2[q];
        dz[q] = (T)2 * (pz[q] - pz2[q]);
    }
    const int64_t ch = (o.N + rchunks - 1) / rchunks, n0 = (int64_t)blockIdx.y * ch, n1 = n0 + ch < o.N ? n0 + ch : o.N;
    double P = 0, A[QP];
#pragma unroll
    for (int q = 0; q < QP; ++q) A[q] = 0;
    for (int64_t nb = n0; nb < n1; nb += PSI_ROWS) {
        const int64_t ne = nb + PSI_ROWS < n1 ? nb + PSI_ROWS : n1;
        T p_ = 0, a_[QP];
#pragma unroll
        for (int q = 0; q < QP; ++q) a_[q] = 0;
        for (int64_t n = nb; n < ne; ++n) {
            const T* r = rows + (s * o.N + n) * psi_rs<QP>();       // uniform over the wavefront: scalar loads
            T ae[QP];
            const T t = psi2_term<T, QP>(r, r + QP, r[2 * QP], zbar, ae);
            p_ += t;
            if constexpr (BWD) {
#pragma unroll
                for (int q = 0; q < QP; ++q) a_[q] += t * ae[q];
            }
        }
        P += (double)p_;
        if constexpr (BWD) {
#pragma unroll
            for (int q = 0; q < QP; ++q) A[q] += (double)a_[q];
        }
    }
    T l2[QP], D = 0;
    psi_l2<T, QP>(o, s, l2);
#pragma unroll
    for (int q = 0; q < QP; ++q) D += psi2_dist_q<T>(dz[q], (T)0, l2[q]);
    const T var = o.var[s * o.ss_var], ex = t_exp<T>(-D);
    if constexpr (!BWD) {
        if (live) atomic_add(acc2 + (s * o.M + m) * o.M + m2, (double)(var * var * ex) * P);
    } else {
        for (int i = threadIdx.x; i < 2 * PSI_TILE * QP; i += 256) (&lz[0][0][0])[i] = 0;
        if (threadIdx.x < QP) ll[threadIdx.x] = 0;
        __syncthreads();
        double dv = 0;
        if (live) {
            const T* g = G2 + s * o.M * o.M;
            const double w = m == m2 ? (double)g[m * o.M + m] : (double)g[m * o.M + m2] + (double)g[m2 * o.M + m];
            const double W = w * (double)(var * var * ex);
            dv = 2.0 * w * (double)(var * ex) * P;
#pragma unroll
            for (int q = 0; q < QP; ++q) {
                const double zq = (double)dz[q], lq = (double)l2[q];
                lds_add(&lz[0][ty][q], W * psi2_dz_pair<double>(A[q], P, zq, 0.0, lq, 0));
                lds_add(&lz[1][tx][q], W * psi2_dz_pair<double>(A[q], P, zq, 0.0, lq, 1));
                lds_add(&ll[q], psi2_dl2_pair<double>(W * P, zq, 0.0, lq));
            }
        }
        dv = block_sum<double>(dv, red);          // (two barriers: the LDS sums above are complete after it)
        if (threadIdx.x == 0 && dvacc) atomic_add(dvacc + s, dv);
        if (dZacc)
            for (int i = threadIdx.x; i < 2 * PSI_TILE * QP; i += 256) {
                const int side = i / (PSI_TILE * QP), row = i / QP % PSI_TILE, q = i % QP;
                const int64_t mm = (int64_t)(side ? tj : ti) * PSI_TILE + row;
                if (mm < o.M && q < o.Q) atomic_add(dZacc + ((own_Z ? s : 0) * o.M + mm) * o.Q + q, lz[side][row][q]);
            }
        if (dl2acc && threadIdx.x < o.Q) atomic_add(dl2acc + s * QP + threadIdx.x, ll[threadIdx.x]);
    }
}

// out[s][m][m'] = out[s][m'][m] = the lower-triangle sum, rounded once
template <typename T>
__global__ __launch_bounds__(256) void psi2_mirror_kernel(int64_t total, int64_t M, const double* __restrict__ acc2, T* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / (M * M), r = i - s * M * M, m = r / M, m2 = r - m * M;
        out[i] = (T)acc2[(s * M + (m > m2 ? m : m2)) * M + (m > m2 ? m2 : m)];
    }
}

// Wt[s][m][m'] = var^2 exp(-D[m,m']) (G2[m,m'] + G2[m',m]) for m' < m, var^2 G2[m,m] on the diagonal, 0 above it
template <typename T, int QP>
__global__ __launch_bounds__(256) void psi2_weight_kernel(PsiOps<T> o, const T* __restrict__ zh, const T* __restrict__ G2, T* __restrict__ Wt) {
    const int64_t MM = o.M * o.M, total = (int64_t)o.S * MM;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / MM, r = i - s * MM, m = r / o.M, m2 = r - m * o.M;
        T w = 0;
        if (m2 <= m) {
            T l2[QP], D = 0;
            psi_l2<T, QP>(o, s, l2);
            const T *pz = zh + (s * o.M + m) * QP, *pz2 = zh + (s * o.M + m2) * QP;
#pragma unroll
            for (int q = 0; q < QP; ++q) D += psi2_dist_q<T>((T)2 * pz[q], (T)2 * pz2[q], l2[q]);
            const T var = o.var[s * o.ss_var], *g = G2 + s * MM;
            w = var * var * t_exp<T>(-D) * (m == m2 ? g[r] : g[r] + g[m2 * o.M + m]);
        }
        Wt[i] = w;
    }
}

// the sums V, M_q, U_q of psi.h of one row over the weighted terms, then the row's gradients
template <typename T, int QP>
struct PsiRowSums {
    double V = 0, Mq[QP], U[QP];
    T v_, m_[QP], u_[QP];
    __device__ __forceinline__ PsiRowSums() {
#pragma unroll
        for (int q = 0; q < QP; ++q) Mq[q] = U[q] = 0;
    }
    __device__ __forceinline__ void open() {
        v_ = 0;
#pragma unroll
        for (int q = 0; q < QP; ++q) m_[q] = u_[q] = 0;
    }
    __device__ __forceinline__ void add(T t, const T* ae) {
        v_ += t;
#pragma unroll
        for (int q = 0; q < QP; ++q) {
            const T x = t * ae[q];
            m_[q] += x;
            u_[q] += x * ae[q];
        }
    }
    __device__ __forceinline__ void close() {
        V += (double)v_;
#pragma unroll
        for (int q = 0; q < QP; ++q) { Mq[q] += (double)m_[q]; U[q] += (double)u_[q]; }
    }
    // scale: what the terms left out (var for Psi1); dead lanes carry zeros and take part in the wavefront sums
    __device__ __forceinline__ void store(int k, const PsiOps<T>& o, bool live, int64_t s, int64_t n, double scale, const T* a, const T* sv, const T* l2,
                                          double* dmuacc, int own_mu, double* dsacc, int own_s, double* dl2acc) const {
#pragma unroll
        for (int q = 0; q < QP; ++q) {
            const double aq = (double)a[q];
            if (q < o.Q && live && dmuacc) atomic_add(dmuacc + ((own_mu ? s : 0) * o.N + n) * o.Q + q, scale * psi_dmu<double>(k, Mq[q]));
            if (q < o.Q && live && dsacc) atomic_add(dsacc + ((own_s ? s : 0) * o.N + n) * o.Q + q, scale * psi_ds<double>(k, aq, U[q], V));
            if (q < o.Q && dl2acc) {        // (uniform over the wavefront)
                const double d = wave_sum(live ? scale * psi_dl2_row<double>(k, aq, (double)sv[q], (double)l2[q], U[q], V) : 0.0);
                if ((threadIdx.x & 63) == 0) atomic_add(dl2acc + s * QP + q, d);
            }
        }
    }
};

template <typename T, int QP>
__global__ __launch_bounds__(PSI_RB) void psi2_bwd_rows_kernel(PsiOps<T> o, const T* __restrict__ zh, const T* __restrict__ Wt,
                                                               double* __restrict__ dmuacc, int own_mu, double* __restrict__ dsacc, int own_s,
                                                               double* __restrict__ dl2acc) {
    const int64_t s = blockIdx.z, n = (int64_t)blockIdx.x * PSI_RB + threadIdx.x;
    const bool live = n < o.N;
    T l2[QP], mu[QP], sv[QP], a[QP], c;
    psi_l2<T, QP>(o, s, l2);
    psi_own_row<T, QP>(o, 2, s, live ? n : o.N - 1, l2, mu, sv, a, c);
    PsiRowSums<T, QP> sums;
    for (int64_t m = blockIdx.y; m < o.M; m += gridDim.y) {      // interleaved: the triangle's rows are of unequal length
        const T *pz = zh + (s * o.M + m) * QP, *w = Wt + (s * o.M + m) * o.M;
        sums.open();
        for (int64_t m2 = 0; m2 <= m; ++m2) {
            const T* pz2 = zh + (s * o.M + m2) * QP;
            T zbar[QP], ae[QP];
#pragma unroll
            for (int q = 0; q < QP; ++q) zbar[q] = pz[q] + pz2[q];
            sums.add(w[m2] * psi2_term<T, QP>(mu, a, c, zbar, ae), ae);
        }
        sums.close();
    }
    sums.store(2, o, live, s, n, 1.0, a, sv, l2, dmuacc, own_mu, dsacc, own_s, dl2acc);
}

// Wq[s][m][m'][j] = var^2 exp(-D[m,m']) (A_{j0+j}[m,m'] + A_{j0+j}[m',m]) for m' < m, var^2 A_{j0+j}[m,m] on the diagonal; 0 above it and for
// j0 + j >= J.  A (S or 1, J, M, M), need not be symmetric.
template <typename T, int QP>
__global__ __launch_bounds__(256) void psi2_quad_weight_kernel(PsiOps<T> o, const T* __restrict__ zh, const T* __restrict__ A, int64_t ss_A, int J, int j0,
                                                               T* __restrict__ Wq) {
    const int64_t MM = o.M * o.M, total = (int64_t)o.S * MM;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = i / MM, r = i - s * MM, m = r / o.M, m2 = r - m * o.M;
        T w[PSI_JB];
#pragma unroll
        for (int j = 0; j < PSI_JB; ++j) w[j] = 0;
        if (m2 <= m) {
            T l2[QP], D = 0;
            psi_l2<T, QP>(o, s, l2);
            const T *pz = zh + (s * o.M + m) * QP, *pz2 = zh + (s * o.M + m2) * QP;
#pragma unroll
            for (int q = 0; q < QP; ++q) D += psi2_dist_q<T>((T)2 * pz[q], (T)2 * pz2[q], l2[q]);
            const T var = o.var[s * o.ss_var], f = var * var * t_exp<T>(-D);
#pragma unroll
            for (int j = 0; j < PSI_JB; ++j) {
                if (j0 + j < J) {
                    const T* g = A + s * ss_A + (int64_t)(j0 + j) * MM;
                    w[j] = f * (m == m2 ? g[r] : g[r] + g[m2 * o.M + m]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < PSI_JB; ++j) Wq[i * PSI_JB + j] = w[j];
    }
}

// R[s][n][j0 + j] = sum_{m, m' <= m} Wq[s][m][m'][j] term(n, m, m'), j < PSI_JB: the term once per pair, into PSI_JB accumulators.  With
// grid.y = 1 a thread writes its row's results (out); otherwise it adds them to the zeroed doubles acc (S, N, J), narrowed by
// mxf_narrow_kernel after the last pass.
template <typename T, int QP>
__global__ __launch_bounds__(PSI_RB) void psi2_quad_rows_kernel(PsiOps<T> o, const T* __restrict__ zh, const T* __restrict__ Wq, int J, int j0,
                                                                double* __restrict__ acc, T* __restrict__ out) {
    const int64_t s = blockIdx.z, n = (int64_t)blockIdx.x * PSI_RB + threadIdx.x;
    const bool live = n < o.N;
    T l2[QP], mu[QP], sv[QP], a[QP], c;
    psi_l2<T, QP>(o, s, l2);
    psi_own_row<T, QP>(o, 2, s, live ? n : o.N - 1, l2, mu, sv, a, c);
    double R[PSI_JB];
#pragma unroll
    for (int j = 0; j < PSI_JB; ++j) R[j] = 0;
    for (int64_t m = blockIdx.y; m < o.M; m += gridDim.y) {      // interleaved: the triangle's rows are of unequal length
        const T *pz = zh + (s * o.M + m) * QP, *w = Wq + (s * o.M + m) * o.M * PSI_JB;
        T r_[PSI_JB], em[QP];       // mu - zbar = (mu - z_m / 2) - z_m' / 2: the first difference once per m
#pragma unroll
        for (int j = 0; j < PSI_JB; ++j) r_[j] = 0;
#pragma unroll
        for (int q = 0; q < QP; ++q) em[q] = mu[q] - pz[q];
        for (int64_t m2 = 0; m2 <= m; ++m2) {
            T ae[QP];
            const T t = psi2_term<T, QP>(em, a, c, zh + (s * o.M + m2) * QP, ae);
#pragma unroll
            for (int j = 0; j < PSI_JB; ++j) r_[j] += w[m2 * PSI_JB + j] * t;
        }
#pragma unroll
        for (int j = 0; j < PSI_JB; ++j) R[j] += (double)r_[j];
    }
    if (!live) return;
    const int64_t at = (s * o.N + n) * J + j0;
#pragma unroll
    for (int j = 0; j < PSI_JB; ++j) {
        if (j0 + j < J) {
            if (acc) atomic_add(acc + at + j, R[j]);
            else out[at + j] = (T)R[j];
        }
    }
}

// Psi1's reverse mode, row-owned, one chunk of PSI_MCH values of m per workgroup: cotangent G1 (S, M, N).  dZ[m] = var sum_n g term a d needs a sum over the rows: one wavefront sum and one
// atomic per (m, q) and wavefront -- N M Q / 64 of them, nothing next to the N M^2 terms of Psi2.
template <typename T, int QP>
__global__ __launch_bounds__(PSI_R1) void psi1_bwd_kernel(PsiOps<T> o, const T* __restrict__ zf, const T* __restrict__ G1, double* __restrict__ dmuacc,
                                                          int own_mu, double* __restrict__ dsacc, int own_s, double* __restrict__ dZacc, int own_Z,
                                                          double* __restrict__ dl2acc, double* __restrict__ dvacc) {
    const int64_t s = blockIdx.z, n = (int64_t)blockIdx.x * PSI_R1 + threadIdx.x;
    const bool live = n < o.N;
    T l2[QP], mu[QP], sv[QP], a[QP], c;
    psi_l2<T, QP>(o, s, l2);
    psi_own_row<T, QP>(o, 1, s, live ? n : o.N - 1, l2, mu, sv, a, c);
    const T var = o.var[s * o.ss_var];
    PsiRowSums<T, QP> sums;
    {
        const int64_t mb = (int64_t)blockIdx.y * PSI_MCH, me = mb + PSI_MCH < o.M ? mb + PSI_MCH : o.M;
        sums.open();
        for (int64_t m = mb; m < me; ++m) {
            T ae[QP];
            const T g = live ? G1[(s * o.M + m) * o.N + n] : (T)0;
            const T t = g * psi1_term<T, QP>(mu, a, c, zf + (s * o.M + m) * QP, ae);
            sums.add(t, ae);
            if (dZacc) {
#pragma unroll
                for (int q = 0; q < QP; ++q) {
                    if (q < o.Q) {          // (uniform over the wavefront)
                        const T d = wave_sum(var * t * ae[q]);
                        if ((threadIdx.x & 63) == 0) atomic_add(dZacc + ((own_Z ? s : 0) * o.M + m) * o.Q + q, (double)d);
                    }
                }
            }
        }
        sums.close();
    }
    sums.store(1, o, live, s, n, (double)var, a, sv, l2, dmuacc, own_mu, dsacc, own_s, dl2acc);
    if (dvacc) {
        const double d = wave_sum(sums.V);
        if ((threadIdx.x & 63) == 0) atomic_add(dvacc + s, d);
    }
}

// dls += 2 l dl2 (summed over q without ARD) and dvar += dvacc, over the samples that share them: one thread, no atomics
template <typename T, int QP>
__global__ void psi_close_kernel(PsiOps<T> o, const double* __restrict__ dl2acc, const double* __restrict__ dvacc, T* dls, int own_l, T* dvar, int own_v) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int nl = o.ard ? o.Q : 1;
    for (int64_t s = 0; s < o.S; ++s) {
        if (dls)
            for (int q = 0; q < o.Q; ++q) {
                T* d = dls + (own_l ? s : 0) * nl + (o.ard ? q : 0);
                *d = (T)((double)*d + 2.0 * (double)o.ls[s * o.ss_ls + (o.ard ? q : 0)] * dl2acc[s * QP + q]);
            }
        if (dvar) {
            T* d = dvar + (own_v ? s : 0);
            *d = (T)((double)*d + dvacc[s]);
        }
    }
}

struct PsiArgs {
    int dtype = MXF_F32, S = 0; int64_t N = 0, M = 0; int Q = 0, ard = 0;
    const void *mu = nullptr, *s = nullptr, *Z = nullptr, *ls = nullptr, *var = nullptr; int64_t ss_mu = 0, ss_s = 0, ss_Z = 0, ss_ls = 0, ss_var = 0;
    void *Psi1 = nullptr, *Psi2 = nullptr;                                                                          // forward
    const void *G1 = nullptr, *G2 = nullptr; void *dmu = nullptr, *ds = nullptr, *dZ = nullptr, *dls = nullptr, *dvar = nullptr;      // reverse
    int J = 0; const void* A = nullptr; int64_t ss_A = 0; void* R = nullptr;                                        // contraction
};

template <typename T>
PsiOps<T> psi_ops(const PsiArgs& a) {
    return {a.S, a.N, a.M, a.Q, a.ard, (const T*)a.mu, a.ss_mu, (const T*)a.s, a.ss_s, (const T*)a.Z, a.ss_Z, (const T*)a.ls, a.ss_ls, (const T*)a.var, a.ss_var};
}
inline dim3 psi_dim3(const unsigned* g) { return dim3(g[0], g[1], g[2]); }

// The three launchers: the plan (fused_plan.h) has every size, grid and scratch offset; carve, launch
template <typename T, int QP>
int psi_fwd(mxf_handle h, const char* name, const PsiArgs& a, const PsiPlan& p, hipStream_t st) {
    const PsiOps<T> o = psi_ops<T>(a);
    char* ws = (char*)mxf_ws(h, p.bytes);
    if (!ws) MXF_FAIL(h, -4, "%s: out of memory for %zu bytes of scratch", name, p.bytes);
    T *zf = (T*)(ws + p.at_z), *zh = (T*)(ws + p.at_zh), *rows = a.Psi2 ? (T*)(ws + p.at_rows) : nullptr;
    hipLaunchKernelGGL((psi_prep_kernel<T, QP>), dim3(grid_for(p.n_prep)), dim3(256), 0, st, o, rows, zf, zh);
    if (a.Psi1) hipLaunchKernelGGL((psi1_fwd_kernel<T, QP>), psi_dim3(p.grid1), dim3(PSI_R1), 0, st, o, zf, (T*)a.Psi1);
    if (a.Psi2) {
        double* acc2 = (double*)(ws + p.at_acc);
        MXF_HIP(h, hipMemsetAsync(acc2, 0, p.zero_bytes, st));
        hipLaunchKernelGGL((psi2_pairs_kernel<T, QP, false>), psi_dim3(p.grid_pairs), dim3(256), 0, st, o, rows, zh, p.rch, acc2, (const T*)nullptr,
                           (double*)nullptr, 0, (double*)nullptr, (double*)nullptr);
        hipLaunchKernelGGL((psi2_mirror_kernel<T>), dim3(grid_for(p.n_mm)), dim3(256), 0, st, p.n_mm, a.M, acc2, (T*)a.Psi2);
    }
    MXF_LAUNCH_CHECK(h);
    return 0;
}

template <typename T, int QP>
int psi_bwd(mxf_handle h, const char* name, const PsiArgs& a, const PsiPlan& p, hipStream_t st) {
    const PsiOps<T> o = psi_ops<T>(a);
    char* ws = (char*)mxf_ws(h, p.bytes);
    if (!ws) MXF_FAIL(h, -4, "%s: out of memory for %zu bytes of scratch", name, p.bytes);
    MXF_HIP(h, hipMemsetAsync(ws + p.at_zero, 0, p.zero_bytes, st));
    T *zf = (T*)(ws + p.at_z), *zh = (T*)(ws + p.at_zh), *rows = p.pairs_pass ? (T*)(ws + p.at_rows) : nullptr;
    double *dl2acc = (double*)(ws + p.at_l2), *dvacc = (double*)(ws + p.at_dv), *big = (double*)(ws + p.at_big);
    double* dmuacc = !a.dmu ? nullptr : (p.wide ? big : (double*)a.dmu);
    double* dsacc = !a.ds ? nullptr : (p.wide ? big + p.end[0] : (double*)a.ds);
    double* dZacc = !a.dZ ? nullptr : (p.wide ? big + p.end[1] : (double*)a.dZ);
    hipLaunchKernelGGL((psi_prep_kernel<T, QP>), dim3(grid_for(p.n_prep)), dim3(256), 0, st, o, rows, zf, zh);
    if (a.G1)
        hipLaunchKernelGGL((psi1_bwd_kernel<T, QP>), psi_dim3(p.grid1), dim3(PSI_R1), 0, st, o, zf, (const T*)a.G1, dmuacc, p.own_mu, dsacc, p.own_s, dZacc,
                           p.own_Z, a.dls ? dl2acc : nullptr, a.dvar ? dvacc : nullptr);
    if (p.pairs_pass)
        hipLaunchKernelGGL((psi2_pairs_kernel<T, QP, true>), psi_dim3(p.grid_pairs), dim3(256), 0, st, o, rows, zh, p.rch, (double*)nullptr, (const T*)a.G2,
                           dZacc, p.own_Z, a.dls ? dl2acc : nullptr, a.dvar ? dvacc : nullptr);
    if (p.rows_pass) {
        T* Wt = (T*)(ws + p.at_wt);
        hipLaunchKernelGGL((psi2_weight_kernel<T, QP>), dim3(grid_for(p.n_mm)), dim3(256), 0, st, o, zh, (const T*)a.G2, Wt);
        hipLaunchKernelGGL((psi2_bwd_rows_kernel<T, QP>), psi_dim3(p.grid_rows), dim3(PSI_RB), 0, st, o, zh, Wt, dmuacc, p.own_mu, dsacc, p.own_s,
                           a.dls ? dl2acc : nullptr);
    }
    if (p.fold) {
        const FoldTable f = {big, {(float*)a.dmu, (float*)a.ds, (float*)a.dZ}, {p.end[0], p.end[1], p.end[2]}};
        hipLaunchKernelGGL(mxf_fold_kernel, dim3(grid_for(f.end[SHARED_SEGS - 1])), dim3(256), 0, st, f);
    }
    if (p.close) hipLaunchKernelGGL((psi_close_kernel<T, QP>), dim3(1), dim3(64), 0, st, o, dl2acc, dvacc, (T*)a.dls, p.own_l, (T*)a.dvar, p.own_v);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

// R (S, N, J) = sum_{m,m'} A_j[m,m'] psi2n[n,m,m'], PSI_JB values of j per pass over the terms; the weights of one pass are reused by the next
// (stream order).  m is split over grid.y as in the reverse pass.
template <typename T, int QP>
int psi_quad(mxf_handle h, const char* name, const PsiArgs& a, const PsiPlan& p, hipStream_t st) {
    const PsiOps<T> o = psi_ops<T>(a);
    char* ws = (char*)mxf_ws(h, p.bytes);
    if (!ws) MXF_FAIL(h, -4, "%s: out of memory for %zu bytes of scratch", name, p.bytes);
    T *zf = (T*)(ws + p.at_z), *zh = (T*)(ws + p.at_zh), *Wq = (T*)(ws + p.at_wt);
    double* acc = p.split ? (double*)(ws + p.at_acc) : nullptr;
    if (acc) MXF_HIP(h, hipMemsetAsync(acc, 0, p.zero_bytes, st));
    hipLaunchKernelGGL((psi_prep_kernel<T, QP>), dim3(grid_for(p.n_prep)), dim3(256), 0, st, o, (T*)nullptr, zf, zh);
    for (int pass = 0; pass < p.npass; ++pass) {
        hipLaunchKernelGGL((psi2_quad_weight_kernel<T, QP>), dim3(grid_for(p.n_mm)), dim3(256), 0, st, o, zh, (const T*)a.A, a.ss_A, a.J, pass * PSI_JB, Wq);
        hipLaunchKernelGGL((psi2_quad_rows_kernel<T, QP>), psi_dim3(p.grid_rows), dim3(PSI_RB), 0, st, o, zh, Wq, a.J, pass * PSI_JB, acc, (T*)a.R);
    }
    if (acc) hipLaunchKernelGGL((mxf_narrow_kernel<T>), dim3(grid_for(p.n_out)), dim3(256), 0, st, p.n_out, acc, (T*)a.R);
    MXF_LAUNCH_CHECK(h);
    return 0;
}

enum PsiCall { PSI_FWD, PSI_BWD, PSI_QUAD };

int run(mxf_handle h, const char* name, PsiCall call, const PsiArgs& a, void* stream) {
    if (!h) return -1;
    if (a.dtype != MXF_F32 && a.dtype != MXF_F64) MXF_FAIL(h, -2, "%s: bad dtype %d", name, a.dtype);
    const PsiRequest r = {.esize = mxf_esize(a.dtype), .S = a.S, .N = a.N, .M = a.M, .Q = a.Q, .ard = a.ard,
                          .ss_mu = a.ss_mu, .ss_s = a.ss_s, .ss_Z = a.ss_Z, .ss_ls = a.ss_ls, .ss_var = a.ss_var,
                          .has_mu = a.mu != nullptr, .has_s = a.s != nullptr, .has_Z = a.Z != nullptr, .has_ls = a.ls != nullptr, .has_var = a.var != nullptr,
                          .has_Psi1 = a.Psi1 != nullptr, .has_Psi2 = a.Psi2 != nullptr, .has_G1 = a.G1 != nullptr, .has_G2 = a.G2 != nullptr,
                          .has_dmu = a.dmu != nullptr, .has_ds = a.ds != nullptr, .has_dZ = a.dZ != nullptr, .has_dls = a.dls != nullptr,
                          .has_dvar = a.dvar != nullptr, .J = a.J, .ss_A = a.ss_A, .has_A = a.A != nullptr, .has_R = a.R != nullptr};
    const PsiPlan p = call == PSI_FWD ? psi_fwd_plan(r) : call == PSI_BWD ? psi_bwd_plan(r) : psi_quad_plan(r);
    if (p.rc) MXF_FAIL(h, p.rc, "%s: %s", name, p.refusal);
    const hipStream_t st = (hipStream_t)stream;
    return dispatch<MXF_F32, MXF_F64>(a.dtype, [&](auto dt) {
        using T = mxf_elem_t<decltype(dt)::value>;
        return dispatch<4, 8, 16>(p.qp, [&](auto qp) {
            constexpr int QP = decltype(qp)::value;
            return call == PSI_FWD ? psi_fwd<T, QP>(h, name, a, p, st) : call == PSI_BWD ? psi_bwd<T, QP>(h, name, a, p, st) : psi_quad<T, QP>(h, name, a, p, st);
        });
    });
}

}  // namespace

extern "C" int mxf_psi_rbf_fwd(mxf_handle h, int dtype, int S, int64_t N, int64_t M, int Q, const void* mu, int64_t strideS_mu, const void* s,
                               int64_t strideS_s, const void* Z, int64_t strideS_Z, const void* lengthscale, int ard, int64_t strideS_ls,
                               const void* variance, int64_t strideS_var, void* Psi1, void* Psi2, void* stream) {
    const PsiArgs a = {.dtype = dtype, .S = S, .N = N, .M = M, .Q = Q, .ard = ard, .mu = mu, .s = s, .Z = Z, .ls = lengthscale, .var = variance,
                       .ss_mu = strideS_mu, .ss_s = strideS_s, .ss_Z = strideS_Z, .ss_ls = strideS_ls, .ss_var = strideS_var, .Psi1 = Psi1, .Psi2 = Psi2};
    return run(h, "mxf_psi_rbf_fwd", PSI_FWD, a, stream);
}

extern "C" int mxf_psi_rbf_bwd(mxf_handle h, int dtype, int S, int64_t N, int64_t M, int Q, const void* mu, int64_t strideS_mu, const void* s,
                               int64_t strideS_s, const void* Z, int64_t strideS_Z, const void* lengthscale, int ard, int64_t strideS_ls,
                               const void* variance, int64_t strideS_var, const void* G1, const void* G2, void* dmu_acc, void* ds_acc, void* dZ_acc,
                               void* dls_acc, void* dvar_acc, void* stream) {
    const PsiArgs a = {.dtype = dtype, .S = S, .N = N, .M = M, .Q = Q, .ard = ard, .mu = mu, .s = s, .Z = Z, .ls = lengthscale, .var = variance,
                       .ss_mu = strideS_mu, .ss_s = strideS_s, .ss_Z = strideS_Z, .ss_ls = strideS_ls, .ss_var = strideS_var, .G1 = G1, .G2 = G2,
                       .dmu = dmu_acc, .ds = ds_acc, .dZ = dZ_acc, .dls = dls_acc, .dvar = dvar_acc};
    return run(h, "mxf_psi_rbf_bwd", PSI_BWD, a, stream);
}

extern "C" int mxf_psi_rbf_quad(mxf_handle h, int dtype, int S, int64_t N, int64_t M, int Q, const void* mu, int64_t strideS_mu, const void* s,
                                int64_t strideS_s, const void* Z, int64_t strideS_Z, const void* lengthscale, int ard, int64_t strideS_ls,
                                const void* variance, int64_t strideS_var, int J, const void* A, int64_t strideS_A, void* R, void* stream) {
    const PsiArgs a = {.dtype = dtype, .S = S, .N = N, .M = M, .Q = Q, .ard = ard, .mu = mu, .s = s, .Z = Z, .ls = lengthscale, .var = variance,
                       .ss_mu = strideS_mu, .ss_s = strideS_s, .ss_Z = strideS_Z, .ss_ls = strideS_ls, .ss_var = strideS_var,
                       .J = J, .A = A, .ss_A = strideS_A, .R = R};
    return run(h, "mxf_psi_rbf_quad", PSI_QUAD, a, stream);
}
