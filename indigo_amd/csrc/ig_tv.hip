// Forward-difference gradient of complex64 volumes, its adjoint, and the fused dual step of isotropic total variation
// (operators.Gradient, Backend.grad3 / tv_dual_step, pics --tv), and the same three with a fourth difference
// along the columns of the panel, the time frames (operators.GradientT, Backend.grad4 / tv4_dual_step, pics --tv-time; §3.8).
//
// A column of x is an F-ordered n0 x n1 x n2 volume with N voxels (axis 0 fastest); a column of u holds the three components
// one after the other, component a in rows [aN, (a+1)N).  With e_a the step along axis a:
//   (D_a x)[i] = x[i + e_a] - x[i]   if i_a < n_a - 1, else 0                    (zero at the far face)
//   (D^H u)[i] = sum_a ( (i_a > 0 ? u_a[i - e_a] : 0) - (i_a < n_a - 1 ? u_a[i] : 0) )
//   proj_mu(u) : per voxel r = sqrt(sum_a |u_a[i]|^2);  u_a[i] *= (r <= mu ? 1 : mu / r)
// D^H never reads u_a on the far face of axis a, so it is the exact adjoint whatever stands there.
//
// The three kernels are templates on the component count NC (3, or 4 with the temporal parts under `if constexpr`) and are
// streaming stencils.  A workgroup owns 256 / LX x-contiguous rows, LX = 8 .. 64 lanes along x (the smallest power of two that
// covers n0, so that short rows do not idle most of a wave); consecutive rows are consecutive in memory, so a wave reads and
// writes whole 128-byte lines.  The +-1 neighbours along x are in the same lines, the ones along y and z are the neighbouring
// rows that this or a nearby workgroup streams anyway: the caches serve them, nothing is staged in LDS.  grid.x strides along
// the row, grid.y over groups of rows, grid.z over columns.  Outputs must not overlap inputs: a workgroup reads rows that another
// one writes.
//
// The 4-D entries (NC = 4) take the nt columns of the panel as frames; a column of u then holds four components, the fourth
// in rows [3N, 4N):
//   (D_t x)[i, t] = x[i, t + 1] - x[i, t]   if t < nt - 1, else 0                (zero in the last frame)
//   (D4^H u)[i, t] = (D^H u_{0..2}[:, t])[i] + (t > 0 ? u_3[i, t - 1] : 0) - (t < nt - 1 ? u_3[i, t] : 0)
//   proj(u) : components 0..2 as proj_mu above;  u_3[i, t] *= (|u_3| <= mu_t ? 1 : mu_t / |u_3|)   (a separate disc)
// D4^H never reads u_3 of the last frame.  The temporal neighbour of a voxel is the same voxel one column further, 8 ld bytes
// away: no line that this column streams holds it, so it is read from memory once more.  Bytes per voxel and frame, with
// f = (nt - 1) / nt the share of frames that have a neighbour (the 3-D entries: 32, 32 (+ 8), 64):
//   k_grad<4>  8 + 8 f read, 32 written                          = 40 + 8 f    (+ 32 when beta != 0)
//   k_gradh<4> 24 + 16 f read (u_3 of the last frame not read), 8 written = 32 + 16 f   (+ 8 when beta != 0)
//   k_dual<4>  16 + 16 f (xn, xo) + 32 (u) read, 32 written     = 80 + 16 f
#include "ig_stencil.h"          // tv_dims, for_each_voxel, grad_adjoint_at, make_dims, make_grid: shared with ig_tgv.hip

namespace {

// y[cN + i, j] = beta * y[cN + i, j] + alpha * (D_c x[:, j])[i], c < 3;  NC == 4: y[3N + i, j] likewise with x[i, j + 1] - x[i, j], 0
// in the last column;  READ_Y false: y is not read
template <int NC, bool READ_Y>
__global__ void __launch_bounds__(TV_BLK)
k_grad(tv_dims d, int64_t ncols, const float2* __restrict__ x, int64_t ldx, float2 a, float2 b,
       float2* __restrict__ y, int64_t ldy) {
    const int64_t s1 = d.n0, s2 = d.n0 * d.n1;
    for_each_voxel(d, ncols, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        const float2* xc = x + j * ldx + i;
        float2* yc = y + j * ldy + i;
        const float2 zero = make_float2(0.f, 0.f);
        const float2 v = xc[0];
        float2 g[NC] = {i0 < d.n0 - 1 ? csub(xc[1], v) : zero, i1 < d.n1 - 1 ? csub(xc[s1], v) : zero,
                        i2 < d.n2 - 1 ? csub(xc[s2], v) : zero};
        if constexpr (NC == 4) g[3] = j < ncols - 1 ? csub(xc[ldx], v) : zero;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float2 r = cmul(a, g[c]);
            if (READ_Y) cfma(r, b, yc[c * d.vol]);
            yc[c * d.vol] = r;
        }
    });
}

// y[i, j] = beta * y[i, j] + alpha * (D^H u[:, j])[i];  NC == 4: D4^H, the columns are the frames
template <int NC, bool READ_Y>
__global__ void __launch_bounds__(TV_BLK)
k_gradh(tv_dims d, int64_t ncols, const float2* __restrict__ u, int64_t ldu, float2 a, float2 b,
        float2* __restrict__ y, int64_t ldy) {
    for_each_voxel(d, ncols, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        const float2* uc = u + j * ldu + i;
        [[maybe_unused]] const float2* ut = uc + 3 * d.vol;
        float2 s = grad_adjoint_at(d, uc, i0, i1, i2);
        if constexpr (NC == 4) {
            if (j > 0) s = cadd(s, ut[-ldu]);
            if (j < ncols - 1) s = csub(s, ut[0]);
        }
        float2 r = cmul(a, s);
        float2* yp = y + j * ldy + i;
        if (READ_Y) cfma(r, b, *yp);
        *yp = r;
    });
}

// the radii of the dual step's projections; the temporal one exists in the kernel arguments of NC == 4 only
template <int NC> struct tv_radii;
template <> struct tv_radii<3> { float mu; };
template <> struct tv_radii<4> { float mu, mu_t; };

// u <- proj(u + sigma * D(2 xn - xo)): w = 2 xn - xo at the voxel, at its three forward neighbours and (NC == 4) in the next
// column, the NC components of u read and written once.  Components 0..2 onto the ball r^2 <= mu^2 (compared squared, as
// k_csoft compares its threshold), the fourth onto the disc |u_3|^2 <= mu_t^2.
template <int NC>
__global__ void __launch_bounds__(TV_BLK)
k_dual(tv_dims d, int64_t ncols, const float2* __restrict__ xn, int64_t ldn, const float2* __restrict__ xo, int64_t ldo,
       float sigma, tv_radii<NC> rad, float2* __restrict__ u, int64_t ldu) {
    const int64_t s1 = d.n0, s2 = d.n0 * d.n1;
    const float mu = rad.mu, mu2 = mu * mu;
    [[maybe_unused]] float mu_t = 0.f, mut2 = 0.f;
    if constexpr (NC == 4) { mu_t = rad.mu_t; mut2 = mu_t * mu_t; }
    for_each_voxel(d, ncols, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        const float2* nc = xn + j * ldn + i;
        const float2* oc = xo + j * ldo + i;
        float2* uc = u + j * ldu + i;
        auto w = [&](int64_t on, int64_t oo) {
            const float2 p = nc[on], q = oc[oo];
            return make_float2(fmaf(2.f, p.x, -q.x), fmaf(2.f, p.y, -q.y));
        };
        const float2 zero = make_float2(0.f, 0.f);
        const float2 w0 = w(0, 0);
        float2 g[NC] = {i0 < d.n0 - 1 ? csub(w(1, 1), w0) : zero, i1 < d.n1 - 1 ? csub(w(s1, s1), w0) : zero,
                        i2 < d.n2 - 1 ? csub(w(s2, s2), w0) : zero};
        if constexpr (NC == 4) g[3] = j < ncols - 1 ? csub(w(ldn, ldo), w0) : zero;
        float2 t[NC];
        float r2 = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float2 v = uc[c * d.vol];
            t[c] = make_float2(fmaf(sigma, g[c].x, v.x), fmaf(sigma, g[c].y, v.y));
            if (c < 3) {
                r2 = fmaf(t[c].x, t[c].x, r2);
                r2 = fmaf(t[c].y, t[c].y, r2);
            }
        }
        const float f = r2 <= mu2 ? 1.f : mu / sqrtf(r2);
#pragma unroll
        for (int c = 0; c < 3; ++c) uc[c * d.vol] = make_float2(t[c].x * f, t[c].y * f);
        if constexpr (NC == 4) {
            const float rt2 = fmaf(t[3].y, t[3].y, t[3].x * t[3].x);
            const float ft = rt2 <= mut2 ? 1.f : mu_t / sqrtf(rt2);
            uc[3 * d.vol] = make_float2(t[3].x * ft, t[3].y * ft);
        }
    });
}

// The body of ig_grad{3,4}_c64 (ADJ false: in = x with N rows per column, y with NC N) and of ig_grad{3,4}h_c64 (ADJ true: in = u
// with NC N rows, y with N).  fn is the entry's name for the messages; kname is "k_" and the profile label.
template <int NC, bool ADJ>
int grad_launch(ig_ctx* ctx, const char* fn, const char* kname, int64_t n0, int64_t n1, int64_t n2, int64_t ncols,
                const void* in, int64_t ldin, float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    const char* many = NC == 3 ? "3N" : "4N";
    IG_REQUIRE(ctx, ctx != nullptr, "%s: ctx is NULL", fn);
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && ncols >= 0, "%s: negative dimension", fn);
    const tv_dims d = make_dims(n0, n1, n2);
    const int64_t rows_in = (ADJ ? NC : 1) * d.vol, rows_y = (ADJ ? 1 : NC) * d.vol;
    IG_REQUIRE(ctx, ldin >= rows_in && ldy >= rows_y, "%s: leading dimension (%lld, %lld) below (%s, %s) for N = %lld", fn,
               (long long)ldin, (long long)ldy, ADJ ? many : "N", ADJ ? "N" : many, (long long)d.vol);
    if (d.vol == 0 || ncols == 0) return IG_OK;
    IG_REQUIRE(ctx, in && y, "%s: NULL pointer", fn);
    IG_REQUIRE(ctx, !ig_panels_overlap(in, ldin, rows_in, ncols, y, ldy, rows_y, ncols), "%s: y overlaps %s", fn, ADJ ? "u" : "x");
    if (int rc = ig_set_device(ctx)) return rc;
    const bool b0 = (br == 0.f && bi == 0.f);
    const float2 a = make_float2(ar, ai), b = make_float2(br, bi);
    const dim3 g = make_grid(d, ncols);
    // bytes per voxel (the table at the top): read and written in every column, more where y is read, and the temporal neighbour
    // (u_3 of two frames) in every column but the last
    const double per_col = ADJ ? 24.0 + 8.0 : 8.0 + 8.0 * NC, read_y = ADJ ? 8.0 : 8.0 * NC, per_next = NC == 3 ? 0.0 : ADJ ? 16.0 : 8.0;
    ig_prof_scope prof(ctx, kname + 2, (double)d.vol * (ncols * (per_col + (b0 ? 0.0 : read_y)) + (ncols - 1) * per_next));
#define IG_TV_GO(KERNEL, READ_Y) hipLaunchKernelGGL((KERNEL<NC, READ_Y>), g, dim3(TV_BLK), 0, ctx->stream, d, ncols, (const float2*)in, ldin, a, b, (float2*)y, ldy)
    if (ADJ) { if (b0) IG_TV_GO(k_gradh, false); else IG_TV_GO(k_gradh, true); }
    else     { if (b0) IG_TV_GO(k_grad, false);  else IG_TV_GO(k_grad, true); }
#undef IG_TV_GO
    IG_LAUNCH_CHECK(ctx, kname);
    return IG_OK;
}

// The body of ig_tv_dual_c64 and ig_tv4_dual_c64, names as above.  Bytes per voxel: 16 (1 + NC) for every column and 16 for the
// temporal neighbour.
template <int NC>
int dual_launch(ig_ctx* ctx, const char* fn, const char* kname, int64_t n0, int64_t n1, int64_t n2, int64_t ncols,
                const void* xn, int64_t ldn, const void* xo, int64_t ldo, float sigma, tv_radii<NC> rad, void* u, int64_t ldu) {
    IG_REQUIRE(ctx, ctx != nullptr, "%s: ctx is NULL", fn);
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && ncols >= 0, "%s: negative dimension", fn);
    if constexpr (NC == 4) IG_REQUIRE(ctx, rad.mu >= 0.f && rad.mu_t >= 0.f, "%s: negative radius (%g, %g)", fn, (double)rad.mu, (double)rad.mu_t);
    else IG_REQUIRE(ctx, rad.mu >= 0.f, "%s: negative radius %g", fn, (double)rad.mu);
    const tv_dims d = make_dims(n0, n1, n2);
    IG_REQUIRE(ctx, ldn >= d.vol && ldo >= d.vol && ldu >= NC * d.vol, "%s: leading dimension (%lld, %lld, %lld) below (N, N, %s) for N = %lld",
               fn, (long long)ldn, (long long)ldo, (long long)ldu, NC == 3 ? "3N" : "4N", (long long)d.vol);
    if (d.vol == 0 || ncols == 0) return IG_OK;
    IG_REQUIRE(ctx, xn && xo && u, "%s: NULL pointer", fn);
    IG_REQUIRE(ctx, !ig_panels_overlap(xn, ldn, d.vol, ncols, u, ldu, NC * d.vol, ncols) && !ig_panels_overlap(xo, ldo, d.vol, ncols, u, ldu, NC * d.vol, ncols),
               "%s: u overlaps xn or xo", fn);
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, kname + 2, (double)d.vol * (ncols * 16.0 * (1 + NC) + (ncols - 1) * (NC == 4 ? 16.0 : 0.0)));
    hipLaunchKernelGGL(k_dual<NC>, make_grid(d, ncols), dim3(TV_BLK), 0, ctx->stream, d, ncols, (const float2*)xn, ldn,
                       (const float2*)xo, ldo, sigma, rad, (float2*)u, ldu);
    IG_LAUNCH_CHECK(ctx, kname);
    return IG_OK;
}

}  // namespace

int ig_grad3_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, const void* x, int64_t ldx,
                 float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    return grad_launch<3, false>(ctx, "ig_grad3_c64", "k_grad3", n0, n1, n2, ncols, x, ldx, ar, ai, br, bi, y, ldy);
}

int ig_grad3h_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, const void* u, int64_t ldu,
                  float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    return grad_launch<3, true>(ctx, "ig_grad3h_c64", "k_grad3h", n0, n1, n2, ncols, u, ldu, ar, ai, br, bi, y, ldy);
}

int ig_tv_dual_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, const void* xn, int64_t ldn,
                   const void* xo, int64_t ldo, float sigma, float mu, void* u, int64_t ldu) {
    return dual_launch<3>(ctx, "ig_tv_dual_c64", "k_tv_dual", n0, n1, n2, ncols, xn, ldn, xo, ldo, sigma, {mu}, u, ldu);
}

int ig_grad4_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t nt, const void* x, int64_t ldx,
                 float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    return grad_launch<4, false>(ctx, "ig_grad4_c64", "k_grad4", n0, n1, n2, nt, x, ldx, ar, ai, br, bi, y, ldy);
}

int ig_grad4h_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t nt, const void* u, int64_t ldu,
                  float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    return grad_launch<4, true>(ctx, "ig_grad4h_c64", "k_grad4h", n0, n1, n2, nt, u, ldu, ar, ai, br, bi, y, ldy);
}

int ig_tv4_dual_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t nt, const void* xn, int64_t ldn,
                    const void* xo, int64_t ldo, float sigma, float mu, float mu_t, void* u, int64_t ldu) {
    return dual_launch<4>(ctx, "ig_tv4_dual_c64", "k_tv4_dual", n0, n1, n2, nt, xn, ldn, xo, ldo, sigma, {mu, mu_t}, u, ldu);
}
