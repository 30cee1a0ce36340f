// Which path one SVGP call takes (composite.hip: SvgpCall), the Psi2 / Phi / V schedule and the scratch layout, as pure functions of the
// request: plain C++, no HIP, checked on the host by tests/host/svgp_plan_check.cpp.  The launcher passes the probe-build knobs in.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "fused_plan.h"     // Carver
#include "gemm_plan.h"
#include "gram_bwd_plan.h"
#include "gram_plan.h"      // ... and include/mxf_gp.h: MXF_K_*, MXF_SVGP_*

// What the launcher gathers.  x_aligned16: X is 16-byte aligned.  The per-row-noise streaming form needs the matrix-pipe reverse pass, whose
// predicate (mxf_svgp_bwd_is_mfma) asks for a 16-byte aligned T; the path is chosen before the scratch that holds T exists, and the launcher
// has always asked about X in its place.  T is carved at 256 bytes, so this bit only sends such a call with an unaligned X down the generic path.
struct SvgpRequest {
    size_t esize = 4; int kind = MXF_K_RBF;
    int S = 1; int64_t B = 0, M = 0; int Q = 0, P = 0;
    int64_t sX = 0, sY = 0;         // sample strides of X and Y in elements, 0 = shared
    int64_t nrows = 1; int ncols = 1;      // noise_var is (1 | B, 1 | P)
    int ard = 0; int want_grad = 0;
    bool use_mat = false;           // the caller passed its own Grams (mxf_svgp_logpdf_mat)
    int form = MXF_SVGP_EXPLICIT;   // the handle's svgp_form
    bool x_aligned16 = true;
};

// Which path the call takes and the sizes every stage uses.  The stages rely on:
//   use_split  => float32, want_grad, !het, SB % 16 == 0        whiten    => use_split
//   bt_path    => use_split, !whiten                             bt_wh     => whiten
//   het_stream => !het, float32                                  het_split => het, float32
//   fused       = want_grad && !het: the streaming reverse pass, its accumulate-into outputs cleared at the start of the call
struct SvgpPlan {
    const char* refusal = nullptr; int rc = 0;     // why the call is refused, and its error code (nothing below is valid then)
    bool use_mat = false, ysamp = false, het_stream = false, het = false, fused = false, use_split = false, whiten = false, bt_path = false, bt_wh = false,
         het_split = false;
    int SS = 1, SYc = 1, lsn = 1;      // samples with columns of their own, Y samples per column, length-scales
    int64_t M = 0, SB = 0, MM = 0, MP = 0;      // M: as requested
    size_t pl_big = 0, pl_h0 = 0, gp_scr = 0;
    int t_blocked = 0;      // T in 16-column blocks (from the shape alone: T is carved 256-byte aligned)
};

static inline SvgpPlan svgp_plan(const SvgpRequest& r) {
    SvgpPlan p;
    p.M = r.M;
    const bool f32 = r.esize == 4, rbf = r.kind == MXF_K_RBF;
    const int64_t B = r.B, M = r.M;
    const int Q = r.Q, P = r.P;
    auto refuse = [&](int rc, const char* why) { p.rc = rc; p.refusal = why; return p; };
    if (P > 8) return refuse(-3, "mxf_svgp_logpdf: P > 8 outputs not supported");
    if ((r.nrows != 1 && r.nrows != B) || (r.ncols != 1 && r.ncols != P)) return refuse(-2, "mxf_svgp_logpdf: noise_var must be (1|B, 1|P)");
    p.use_mat = r.use_mat;
    // sampled Y over shared X (hence shared Kuf, T, U): the S samples share the B columns -- generic path, the data term is quadratic in Y
    p.ysamp = r.S > 1 && r.sX == 0 && r.sY != 0;
    if (p.ysamp && r.sY != B * P) return refuse(-2, "mxf_svgp_logpdf: Y samples must be contiguous");
    p.SS = (r.sX == 0) ? 1 : r.S;
    const int64_t SB = p.SB = (int64_t)p.SS * B;
    // generic path (het): Kuf-side reverse mode through a materialised dKuf (not the streaming fused pass); also for Q > 16 inputs, which the
    // register-tiled fused reverse pass does not cover (gram_bwd.hip: generic kernel).  Per-row noise (B, 1) with one output column on the
    // float32 split path runs the STREAMING form (het_stream: the het_* kernels of composite.hip); every other heteroscedastic shape keeps the generic path.
    p.het_stream = f32 && r.want_grad && r.nrows == B && r.nrows > 1 && r.ncols == 1 && P == 1 && !p.use_mat && !p.ysamp && Q <= 8 && (B % 16 == 0) &&
                   (M % 16 == 0) && M >= 128 && r.form == MXF_SVGP_EXPLICIT && svgp_bwd_mfma_shape(rbf, f32, SB, B, Q, P) && r.x_aligned16;
    p.het = (r.nrows > 1 || r.ncols > 1 || p.use_mat || p.ysamp || Q > 16) && !p.het_stream;
    if (r.sX != 0 && r.sX != B * Q) return refuse(-2, "mxf_svgp_logpdf: X samples must be contiguous");
    if (r.S > 1 && r.sX == 0 && r.sY == 0) return refuse(-3, "mxf_svgp_logpdf: S > 1 with neither X nor Y sampled");
    p.SYc = p.ysamp ? r.S : 1;
    p.MM = M * M; p.MP = M * P;
    p.lsn = r.ard ? Q : 1;
    p.fused = r.want_grad && !p.het;
    // float32 streaming: the two big GEMMs run on the 16-bit matrix pipe from split planes of their operands (gemm_split.hip), in the format
    // of two scaled f16 terms (three products)
    p.use_split = p.fused && f32 && (SB % 16 == 0) && (M % 16 == 0) && M >= 128 && Q <= 16;
    p.pl_big = split_plane_elems(M, SB); p.pl_h0 = split_plane_elems(M, M);     // == split_plane_elems(SB, M)
    p.gp_scr = p.use_split ? gram_planes_scratch_bytes(SB, SB, Q) : 0;      // upper bound for either orientation
    // float32 streaming form (mxf_svgp_configure): the whitened tier runs on the f16x2 split kernels' wide forms only
    p.whiten = f32 && r.want_grad && r.form == MXF_SVGP_WHITENED;
    if (p.whiten && !(p.use_split && (M % 128) == 0 && (SB % 256) == 0))
        return refuse(-3, "mxf_svgp_logpdf: the whitened float32 form needs M % 128 == 0, S B % 256 == 0, Q <= 16, homoscedastic noise (see mxf_svgp_whitened_ok)");
    // ONE set of Kuf planes: T = H0 Kuf reads the planes Psi2 reads (operand (m, k = n)) through gemm_bt.hip's transposing LDS read, and forms
    // the row U = w^T Kuf on the way (a second planes pass wrote 8.6 GB between the two products: 1.8 ms of the 24 ms step with the matrix pipe
    // idle).  Needs the explicit float32 form, one output column, whole 256 x 256 tiles.
    p.bt_path = p.use_split && !p.whiten && !p.het_stream && P == 1 && M <= 2048 && gemm_bt_shape_ok(M, SB, M);
    // the whitened tier likewise: T = Hh V reads the planes of V that Phi = V V^T reads (the V product's planes output IS the K-major layout),
    // and forms U = a^T V on the way -- the V product writes neither the planes of V^T (8.6 GB) nor the partial sums of U
    p.bt_wh = p.whiten && P == 1 && M <= 2048 && gemm_bt_shape_ok(M, SB, M);
    // the generic (materialised-Gram / heteroscedastic) float32 path's two big products on the f16 matrix pipe as well: T = H0 Kuf through the
    // K-major product from the planes of Kuf (split from the float32 Gram: one maxabs + one split pass, 0.17 ms at 512 x 131 072), and
    // G' = Ksc Kuf^T from the planes of Ksc and the same Kuf planes -- f32-equivalent like the streaming path's products (three f16 products, f32
    // accumulation) where the generic kernel ran true-f32 MFMAs at 100 TF: the deep GP's first layer 0.68 + 0.66 ms -> planes 0.35 + products 0.3.
    p.het_split = p.het && f32 && r.want_grad && gemm_bt_shape_ok(M, SB, M) && (int64_t)M * SB >= (int64_t)1 << 24;
    // (training step on the split path whose reverse pass runs on the matrix pipe: T is written in 16-column blocks, so that each 16 x 16
    //  tile that pass reads is one contiguous KB instead of 16 pieces of 64 bytes, 4 SB bytes apart)
    p.t_blocked = (p.use_split && (svgp_bwd_mfma_shape(rbf, f32, SB, B, Q, P) || svgp_bwd_diff_reads_blocked(f32, SB, Q, P))) ? 1 : 0;
    return p;
}

// mxf_svgp_whitened_ok: does a training call of this shape, homoscedastic noise and per-sample Y, run in the whitened form?
static inline bool svgp_whitened_ok(size_t esize, int S, int64_t B, int64_t M, int Q, int P, int64_t sX) {
    if (S <= 0 || B <= 0) return false;
    SvgpRequest r;
    r.esize = esize; r.S = S; r.B = B; r.M = M; r.Q = Q; r.P = P; r.sX = sX; r.sY = B * P; r.want_grad = 1; r.form = MXF_SVGP_WHITENED;
    const SvgpPlan p = svgp_plan(r);
    return p.refusal == nullptr && p.whiten;
}

// ---- the Psi2 / Phi / V schedule ---------------------------------------------------------------------------------------------------------
// probe-build knobs MXF_SVGP_PSI2_KA, MXF_SVGP_PSI2_RA, MXF_SVGP_PSI2_RB and whether the last two were set
struct SvgpKnobs { int64_t psi2_ka = -1; int psi2_ra = 148; bool psi2_ra_set = false; int psi2_rb = 16; bool psi2_rb_set = false; };
struct SvgpSchedule {
    int64_t KA = 0;                  // explicit form: Psi2's first launch covers [0, KA) of the SB columns, its second the rest
    int reserve_a = 0, reserve_b = 0;      // ... and the CUs each leaves to the other streams
    bool few = false;                // whitened tier: few samples per GPU
    int reserve_v = 0, reserve_phi = 0;    // ... and the CUs the V and the Phi product leave
};
// Psi2 = Kuf Kuf^T depends on neither the core nor the T GEMM nor the reverse pass: it starts at once on the side stream, lower blocks only,
// split-K.  Two launches: phase A covers the first KA = 128 M columns (about as long as the core chains run) with ONE workgroup per CU on
// ~216 CUs, so that the core chains' f64 workgroups (a whole CU's LDS / registers each) still find free CUs; phase B (the rest)
// fills the chip.  Same-box A/B at 4 samples per GPU: 13.65 -> 12.95 ms per step; neutral at 32 samples.
// (few samples per GPU: the whole product runs in the reduced-occupancy form -- the core chains are the critical path there and
//  Psi2 is short; same-box at 4 samples: 5.46 -> 5.20 ms per step; at 32 samples a longer first phase costs 0.1-0.4 ms)
static inline SvgpSchedule svgp_psi2_schedule(const SvgpPlan& p, const SvgpKnobs& k) {
    SvgpSchedule s;
    if (!p.fused) return s;      // (no Psi2 stage: the generic path forms its G' in the reverse pass)
    if (p.whiten) {
        // (few samples per GPU: the Kuu chain on the caller's stream is the critical path -- both side-stream products leave it 40 CUs)
        s.few = p.SB <= 2 * 192 * p.M;
        s.reserve_v = s.few ? 40 : 0;
        s.reserve_phi = s.few ? 202 : k.psi2_rb;
        return s;
    }
    const int64_t ka_dflt = (p.use_split ? 192 : 128) * p.M;
    // one set of planes (bt_path): nothing but the core chains runs next to Psi2, so the whole product leaves them 32 CUs and there is no
    // reduced first phase -- the chains finish under Psi2 and T starts when Psi2 ends (same box, 32 samples: 23.5 -> 22.85 ms per step with
    // a second planes pass beside it before; 24 CUs: 23.8; 40: 22.9)
    const int64_t ka_req = k.psi2_ka >= 0 ? k.psi2_ka : (p.use_split && p.SB <= 2 * ka_dflt ? p.SB : (p.bt_path ? 0 : ka_dflt));
    s.KA = (ka_req > 0 && ka_req < p.SB) ? ka_req / 32 * 32 : (ka_req > 0 ? p.SB : 0);
    // split planes: 4 workgroups of the two-term kernel fit a CU: (256 - 202) * 4 = 216 workgroups = one per CU on 216 CUs.  One-planes path:
    // (256 - 214) * 4 = 168 workgroups -- the chains are alone on what Psi2 leaves, and 88 CUs serve the few-sample step better than 40
    // (same box, 4 samples: 4.30 -> 4.21 ms; 210: 4.25-4.32, 218: 4.22-4.26, 224: 4.27; configs[3] at 4 samples 2.41 -> 2.37).
    // Dense fallback (float64, ragged shapes): the knob's default
    s.reserve_a = (p.use_split && !k.psi2_ra_set) ? (p.bt_path ? 214 : 202) : k.psi2_ra;
    s.reserve_b = (p.bt_path && !k.psi2_rb_set) ? 32 : k.psi2_rb;
    return s;
}

// ---- scratch -----------------------------------------------------------------------------------------------------------------------------
// The SVGP call's scratch (what a path does not take stays null) and its layout, one list: run once to count and once to carve
template <typename T>
struct SvgpScratch {
    typedef double D;
    D *Zd, *lsd, *vard, *noised, *mud, *Wd, *sd, *Lm, *Linv, *Ki, *Su, *Lsinv, *Sui, *KiSu, *H0, *tmp, *wd, *sc, *scal, *ad, *hhs, *hbe2;
    D *G, *T1, *AKi, *T2, *dKuu, *dSu, *Gw, *dmud, *dZc, *dlsc, *dvc;
    T *Aext, *wT, *Text, *qbuf, *Kuf, *Kfu, *Psi2, *R, *Eb, *aT;
    unsigned short *plKfu, *plH0, *plKuf, *plLi, *wpl, *plVt, *hsA, *hsK, *hsS;
    float *gscr0, *gscr1, *sigf, *upart, *hcs, *hrs, *hys, *hnz;
    int* info2; unsigned* hsw; int64_t pVt;

    void carve(Carver& cv, const SvgpRequest& r, const SvgpPlan& p) {
        const int64_t B = r.B, M = r.M, SB = p.SB, MM = p.MM, MP = p.MP;
        const int S = r.S, Q = r.Q, P = r.P, lsn = p.lsn;
        const size_t pl_big = p.pl_big, pl_h0 = p.pl_h0;
        Zd = cv.take<D>(M * Q); lsd = cv.take<D>(lsn); vard = cv.take<D>(1); noised = cv.take<D>(1);     // f64 copies of the parameters
        mud = cv.take<D>(MP); Wd = cv.take<D>(MM); sd = cv.take<D>(M);
        Lm = cv.take<D>(MM); Linv = cv.take<D>(MM); Ki = cv.take<D>(MM); Su = cv.take<D>(MM); Lsinv = cv.take<D>(MM);
        Sui = cv.take<D>(MM); KiSu = cv.take<D>(MM); H0 = cv.take<D>(MM); tmp = cv.take<D>(MM);
        wd = cv.take<D>(MP); sc = cv.take<D>(16); scal = cv.take<D>(2 * (size_t)S); info2 = cv.take<int>(8);
        Aext = cv.take<T>((size_t)(M + P) * M); wT = cv.take<T>(MP);
        Text = cv.take<T>((size_t)(M + P) * SB); qbuf = cv.take<T>((size_t)SB);
        if (p.use_split) {
            plKfu = cv.take<unsigned short>(3 * pl_big); plH0 = cv.take<unsigned short>(3 * pl_h0); plKuf = cv.take<unsigned short>(3 * pl_big);
            gscr0 = (float*)cv.take<char>(p.gp_scr); gscr1 = (float*)cv.take<char>(p.gp_scr);
        } else {
            Kuf = cv.take<T>((size_t)M * SB);        // Kuf, Kfu in the streaming dtype
            if (r.want_grad) Kfu = cv.take<T>((size_t)M * SB);
        }
        if (p.whiten) { plLi = cv.take<unsigned short>(2 * pl_h0); ad = cv.take<D>(MP); aT = cv.take<T>(MP); sigf = cv.take<float>(4); upart = cv.take<float>((size_t)(M / 128) * SB); }
        if (p.bt_path || p.bt_wh) wpl = cv.take<unsigned short>(2 * (size_t)M + 8);
        if (p.het_stream) { hcs = cv.take<float>(B); hrs = cv.take<float>(B); hys = cv.take<float>((size_t)(r.sY == 0 ? B : SB)); hhs = cv.take<D>(4); hbe2 = cv.take<D>(S); hnz = cv.take<float>(4); }
        if (p.het_split) { hsA = cv.take<unsigned short>(2 * pl_h0); hsK = cv.take<unsigned short>(2 * pl_big); hsS = cv.take<unsigned short>(2 * pl_big); hsw = cv.take<unsigned>(4); }
        if (r.want_grad) {
            Psi2 = cv.take<T>(MM); R = cv.take<T>(MP); Eb = cv.take<T>((size_t)SB * P);
            G = cv.take<D>(MM); T1 = cv.take<D>(MM); AKi = cv.take<D>(MM); T2 = cv.take<D>(MM); dKuu = cv.take<D>(MM); dSu = cv.take<D>(MM);
            Gw = cv.take<D>(MP); dmud = cv.take<D>(MP); dZc = cv.take<D>(M * Q); dlsc = cv.take<D>(lsn); dvc = cv.take<D>(4);
        }
        // sc: [0]=sumlogdiag L, [1]=sumlogdiag Ls, [2]=tr(Ki Su), [3]=mu.w, [4]=dnoise, [5]=dvar_direct, [6], [7]: whitened tier's q_n total
    }
};
