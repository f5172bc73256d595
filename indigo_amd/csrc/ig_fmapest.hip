// Field-map estimation from E echo images: the regularised multi-echo fit of Funai, Fessler, Yeo, Olafsson and Noll (IEEE TMI
// 27:1484, 2008), one separable-quadratic-surrogate step per launch (Backend.fieldmap_init / fieldmap_step, python -m
// indigo_amd.fmapest).
//
// y is the N x E complex64 panel of the echo images on the F-ordered n0 x n1 x n2 volume (axis 0 fastest), y_l ~ m exp(-2 pi i f
// te_l) as in pics --fmap, f the real field in Hz.  For every pair l < m, in the order (0,1), (0,2), .., (0,E-1), (1,2), ..:
//   p = y_m conj(y_l),   w = |p|,   k = 2 pi (te_m - te_l),   r = p exp(i k f)   so that   s = arg r = pv(arg p + k f),
//   w sin s = Im r,   w cos s = Re r,   w kappa(s) = Im r / s   (kappa = sin s / s, Huber's curvature of 1 - cos; s == 0: Re r)
//   Psi(f) = sum_j sum_pairs (w - Re r)  +  beta / 2 sum_edges (f_j - f_j')^2          (edges: the forward differences of ig_tv.hip)
//   g_j = sum_pairs k Im r + beta sum_{j' ~ j} (f_j - f_j'),   d_j = sum_pairs k^2 Im r / s + 2 beta deg_j,
//   f_new[j] = f_old[j] - g_j / d_j                                                     (d_j == 0: f_new[j] = f_old[j])
// Im r and Im r / s are continuous across the wrap of s at +-pi, so the branch atan2f picks there changes nothing beyond rounding.
//
// The phase: (te_m - te_l) f reaches tens of cycles, so it is formed in double, reduced by rint to [-1/2, 1/2], converted to
// float and handed to sincospif, as ig_fmap_phase_c64 does.  No fast-math intrinsics.  Per pair: one sincospif, one atan2f, one
// divide.  The E samples of a voxel stay in registers: one instantiation per E = 2 .. 8, the pair loops fully unrolled, and one
// more per E that also emits the cost of its INPUT iterate: per thread a double sum, per workgroup one partial (wave shuffles, then
// the four waves through LDS, a fixed order), the caller adds the partials in order -- bitwise repeatable.  With a NULL partials
// buffer the cost arithmetic is not compiled in; f_new is the same bits either way.  With a NULL f_new the pass is the cost alone
// (the driver's last evaluation, and the other half of the composition that tools/fmapest_timing.py times the fusion against).
//
// The lane layout and voxel loop are those of ig_tv.hip / ig_tgv.hip (ig_stencil.h): the neighbours of f_old along x sit in the same
// lines, those along y and z in rows that this or a nearby workgroup streams anyway; nothing is staged in LDS.  Bytes per voxel:
// 8 E for the panel, 4 + 4 for the two fields.
#include "ig_stencil.h"

namespace {

constexpr int FM_MAXE = 8;
constexpr int FM_MAXPAIRS = FM_MAXE * (FM_MAXE - 1) / 2;
constexpr double FM_TWO_PI = 6.283185307179586476925286766559;

// per pair, in the order above: te_m - te_l, k = 2 pi (te_m - te_l) rounded to float, and k * k rounded once more (formed on the
// host: wave-uniform values that the kernel would otherwise compute with the vector unit and keep in vector registers)
struct fm_pairs { double dte[FM_MAXPAIRS]; float k[FM_MAXPAIRS], k2[FM_MAXPAIRS]; };

// f0 = -arg(y_1 conj(y_0)) / (2 pi (te_1 - te_0))
__global__ void __launch_bounds__(TV_BLK)
k_fmapest_init(tv_dims d, const float2* __restrict__ y, int64_t ldy, float inv_k, float* __restrict__ f) {
    for_each_voxel(d, 1, [&](int64_t, int64_t, int64_t, int64_t, int64_t i) {
        const float2 p = cmulc(y[i], y[ldy + i]);
        f[i] = -atan2f(p.y, p.x) * inv_k;
    });
}

// STEP false: the cost alone (f_new is not touched, and what only the step needs is not computed)
template <int E, bool COST, bool STEP>
__global__ void __launch_bounds__(TV_BLK)
k_fmapest_step(tv_dims d, const float2* __restrict__ y, int64_t ldy, const float* __restrict__ fo, fm_pairs pr, float beta,
               float* __restrict__ fn, double* __restrict__ parts) {
    const int64_t stride[3] = {1, d.n0, d.n0 * d.n1};
    double acc = 0.0;
    for_each_voxel(d, 1, [&](int64_t, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        float2 ys[E];
#pragma unroll
        for (int l = 0; l < E; ++l) ys[l] = y[l * ldy + i];
        const float f = fo[i];
        float g = 0.f, dd = 0.f;
        double c = 0.0;
        int q = 0;
#pragma unroll
        for (int l = 0; l < E; ++l)
#pragma unroll
            for (int m = l + 1; m < E; ++m, ++q) {
                const double dte = pr.dte[q];
                const float k = pr.k[q], k2 = pr.k2[q];
                const float2 p = cmulc(ys[l], ys[m]);
                double cyc = dte * (double)f;
                cyc -= rint(cyc);                                              // whole cycles drop out exactly
                float sn, cs;
                sincospif(2.f * (float)cyc, &sn, &cs);
                const float2 r = cmul(p, make_float2(cs, sn));
                const float s = atan2f(r.y, r.x);
                const float h = s != 0.f ? r.y / s : r.x;                      // w kappa(s); s == 0: r is real and not negative
                g = fmaf(k, r.y, g);
                dd = fmaf(k2, h, dd);
                if (COST) c += (double)(sqrtf(fmaf(p.x, p.x, p.y * p.y)) - r.x);
            }
        const bool fwd[3] = {i0 < d.n0 - 1, i1 < d.n1 - 1, i2 < d.n2 - 1}, bwd[3] = {i0 > 0, i1 > 0, i2 > 0};
        float pg = 0.f;
        int deg = 0;
        double pen = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (fwd[a]) {
                const float df = f - fo[i + stride[a]];
                pg += df;
                ++deg;
                if (COST) pen += (double)df * (double)df;
            }
            if (bwd[a]) {
                pg += f - fo[i - stride[a]];
                ++deg;
            }
        }
        g = fmaf(beta, pg, g);
        dd = fmaf(2.f * beta, (float)deg, dd);
        if (STEP) fn[i] = dd > 0.f ? f - g / dd : f;
        if (COST) acc += c + 0.5 * (double)beta * pen;
    });
    if (COST) {
        __shared__ double sh[TV_BLK / 64];
        double v = acc;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = sh[0];
#pragma unroll
            for (int wv = 1; wv < TV_BLK / 64; ++wv) t += sh[wv];
            parts[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
        }
    }
}

bool ranges_overlap(const void* p, size_t pbytes, const void* q, size_t qbytes) {
    return ig_bytes_overlap((uintptr_t)p, (uintptr_t)p + pbytes, (uintptr_t)q, (uintptr_t)q + qbytes);
}

}  // namespace

int64_t ig_fmapest_cost_parts(int64_t n0, int64_t n1, int64_t n2) {
    if (n0 < 1 || n1 < 1 || n2 < 1) return 0;
    const dim3 g = make_grid(make_dims(n0, n1, n2), 1);
    return (int64_t)g.x * g.y;
}

int ig_fmapest_init_r32(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, const void* y, int64_t ldy, double te0, double te1, float* f) {
    const char* fn = "ig_fmapest_init_r32";
    IG_REQUIRE(ctx, ctx != nullptr, "%s: ctx is NULL", fn);
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0, "%s: negative dimension", fn);
    IG_REQUIRE(ctx, te1 > te0, "%s: echo times (%g, %g) are not strictly increasing", fn, te0, te1);
    const tv_dims d = make_dims(n0, n1, n2);
    IG_REQUIRE(ctx, ldy >= d.vol, "%s: leading dimension %lld below N = %lld", fn, (long long)ldy, (long long)d.vol);
    if (d.vol == 0) return IG_OK;
    IG_REQUIRE(ctx, y && f, "%s: NULL pointer", fn);
    IG_REQUIRE(ctx, !ranges_overlap(f, (size_t)d.vol * sizeof(float), y, (size_t)(ldy + d.vol) * sizeof(float2)), "%s: f overlaps y", fn);
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, "fmapest_init", (double)d.vol * 20.0);
    hipLaunchKernelGGL(k_fmapest_init, make_grid(d, 1), dim3(TV_BLK), 0, ctx->stream, d, (const float2*)y, ldy,
                       (float)(1.0 / (FM_TWO_PI * (te1 - te0))), f);
    IG_LAUNCH_CHECK(ctx, "k_fmapest_init");
    return IG_OK;
}

int ig_fmapest_step_r32(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t E, const void* y, int64_t ldy, const double* te,
                        float beta, const float* f_old, float* f_new, double* parts, int64_t nparts) {
    const char* fn = "ig_fmapest_step_r32";
    IG_REQUIRE(ctx, ctx != nullptr, "%s: ctx is NULL", fn);
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0, "%s: negative dimension", fn);
    IG_REQUIRE(ctx, E >= 2 && E <= FM_MAXE, "%s: %lld echoes, between 2 and %d are supported", fn, (long long)E, FM_MAXE);
    IG_REQUIRE(ctx, te != nullptr, "%s: NULL pointer", fn);
    for (int64_t l = 1; l < E; ++l)
        IG_REQUIRE(ctx, te[l] > te[l - 1], "%s: echo times are not strictly increasing (%g after %g)", fn, te[l], te[l - 1]);
    IG_REQUIRE(ctx, beta >= 0.f && beta <= 3.0e38f, "%s: beta %g is negative or not finite", fn, (double)beta);
    const tv_dims d = make_dims(n0, n1, n2);
    IG_REQUIRE(ctx, ldy >= d.vol, "%s: leading dimension %lld below N = %lld", fn, (long long)ldy, (long long)d.vol);
    if (d.vol == 0) return IG_OK;
    IG_REQUIRE(ctx, y && f_old && (f_new || parts), "%s: NULL pointer", fn);
    const size_t fbytes = (size_t)d.vol * sizeof(float), ybytes = (size_t)((E - 1) * ldy + d.vol) * sizeof(float2);
    IG_REQUIRE(ctx, !f_new || (!ranges_overlap(f_new, fbytes, f_old, fbytes) && !ranges_overlap(f_new, fbytes, y, ybytes)),
               "%s: f_new overlaps f_old or y", fn);
    const dim3 grid = make_grid(d, 1);
    const int64_t need = (int64_t)grid.x * grid.y;
    if (parts) {
        IG_REQUIRE(ctx, nparts >= need, "%s: %lld partial sums, %lld are written", fn, (long long)nparts, (long long)need);
        const size_t pbytes = (size_t)need * sizeof(double);
        IG_REQUIRE(ctx, !ranges_overlap(parts, pbytes, f_old, fbytes) && !(f_new && ranges_overlap(parts, pbytes, f_new, fbytes)) &&
                   !ranges_overlap(parts, pbytes, y, ybytes), "%s: the partial sums overlap f_old, f_new or y", fn);
    }
    fm_pairs pr = {};
    int q = 0;
    for (int64_t l = 0; l < E; ++l)
        for (int64_t m = l + 1; m < E; ++m, ++q) {
            pr.dte[q] = te[m] - te[l];
            pr.k[q] = (float)(FM_TWO_PI * pr.dte[q]);
            pr.k2[q] = pr.k[q] * pr.k[q];
        }
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, !f_new ? "fmapest_cost" : parts ? "fmapest_step_cost" : "fmapest_step",
                       (double)d.vol * (8.0 * (double)E + (f_new ? 8.0 : 4.0)));
#define IG_FM_LAUNCH(NE, COST, STEP) \
    hipLaunchKernelGGL((k_fmapest_step<NE, COST, STEP>), grid, dim3(TV_BLK), 0, ctx->stream, d, (const float2*)y, ldy, f_old, pr, beta, f_new, parts)
#define IG_FM_GO(NE) \
    case NE: \
        if (!f_new) IG_FM_LAUNCH(NE, true, false); \
        else if (parts) IG_FM_LAUNCH(NE, true, true); \
        else IG_FM_LAUNCH(NE, false, true); \
        break;
    switch ((int)E) {
        IG_FM_GO(2) IG_FM_GO(3) IG_FM_GO(4) IG_FM_GO(5) IG_FM_GO(6) IG_FM_GO(7) IG_FM_GO(8)
    }
#undef IG_FM_GO
#undef IG_FM_LAUNCH
    IG_LAUNCH_CHECK(ctx, "k_fmapest_step");
    return IG_OK;
}
