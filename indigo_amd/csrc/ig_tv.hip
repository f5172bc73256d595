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
// All three kernels are streaming stencils.  A workgroup owns 256 / LX x-contiguous rows, LX = 8 .. 64 lanes along x (the
// smallest power of two that covers n0, so that short rows do not idle most of a wave); consecutive rows are consecutive in
// memory, so a wave reads and writes whole 128-byte lines.  The +-1 neighbours along x are in the same lines, the ones along y
// and z are the neighbouring rows that this or a nearby workgroup streams anyway: the caches serve them, nothing is staged in
// LDS.  grid.x strides along the row, grid.y over groups of rows, grid.z over columns.  Outputs must not overlap inputs: a
// workgroup reads rows that another one writes.
//
// The 4-D entries take the nt columns of the panel as frames; a column of u then holds four components, the fourth in rows
// [3N, 4N):
//   (D_t x)[i, t] = x[i, t + 1] - x[i, t]   if t < nt - 1, else 0                (zero in the last frame)
//   (D4^H u)[i, t] = (D^H u_{0..2}[:, t])[i] + (t > 0 ? u_3[i, t - 1] : 0) - (t < nt - 1 ? u_3[i, t] : 0)
//   proj(u) : components 0..2 as proj_mu above;  u_3[i, t] *= (|u_3| <= mu_t ? 1 : mu_t / |u_3|)   (a separate disc)
// D4^H never reads u_3 of the last frame.  The temporal neighbour of a voxel is the same voxel one column further, 8 ld bytes
// away: no line that this column streams holds it, so it is read from memory once more.  Bytes per voxel and frame, with
// f = (nt - 1) / nt the share of frames that have a neighbour (the 3-D entries: 32, 32 (+ 8), 64):
//   k_grad4    8 + 8 f read, 32 written                          = 40 + 8 f    (+ 32 when beta != 0)
//   k_grad4h   24 + 16 f read (u_3 of the last frame not read), 8 written = 32 + 16 f   (+ 8 when beta != 0)
//   k_tv4_dual 16 + 16 f (xn, xo) + 32 (u) read, 32 written     = 80 + 16 f
// The same for_each_voxel, grid and workgroup shape: grid.z runs over the frames.
#include "ig_common.h"

namespace {

constexpr int TV_BLK = 256;
constexpr int TV_MAXROWS = 2048;       // grid.y cap: with grid.x that is a few workgroups per CU in flight, the rest strides
constexpr int MAXG = 65535;

struct tv_dims { int64_t n0, n1, n2, vol; int lx_log2; };

// the voxel loop shared by the three kernels: body(column j, i0, i1, i2, voxel index i)
template <class F>
__device__ __forceinline__ void for_each_voxel(const tv_dims d, int64_t ncols, F body) {
    const int lx = 1 << d.lx_log2;
    const int tx = threadIdx.x & (lx - 1), ty = threadIdx.x >> d.lx_log2, rows = TV_BLK >> d.lx_log2;
    const int64_t nrows = d.n1 * d.n2;
    for (int64_t j = blockIdx.z; j < ncols; j += gridDim.z)
        for (int64_t r = (int64_t)blockIdx.y * rows + ty; r < nrows; r += (int64_t)gridDim.y * rows) {
            const int64_t i1 = r % d.n1, i2 = r / d.n1;
            for (int64_t i0 = (int64_t)blockIdx.x * lx + tx; i0 < d.n0; i0 += (int64_t)gridDim.x * lx)
                body(j, i0, i1, i2, r * d.n0 + i0);
        }
}

// y[aN + i, j] = beta * y[aN + i, j] + alpha * (D_a x[:, j])[i];  READ_Y false: y is not read
template <bool READ_Y>
__global__ void __launch_bounds__(TV_BLK)
k_grad3(tv_dims d, int64_t ncols, const float2* __restrict__ x, int64_t ldx, float2 a, float2 b,
        float2* __restrict__ y, int64_t ldy) {
    const int64_t s1 = d.n0, s2 = d.n0 * d.n1;
    for_each_voxel(d, ncols, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        const float2* xc = x + j * ldx + i;
        float2* yc = y + j * ldy + i;
        const float2 zero = make_float2(0.f, 0.f);
        const float2 v = xc[0];
        const float2 g[3] = {i0 < d.n0 - 1 ? csub(xc[1], v) : zero, i1 < d.n1 - 1 ? csub(xc[s1], v) : zero,
                             i2 < d.n2 - 1 ? csub(xc[s2], v) : zero};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float2 r = cmul(a, g[c]);
            if (READ_Y) cfma(r, b, yc[c * d.vol]);
            yc[c * d.vol] = r;
        }
    });
}

// (D^H u[:, j])[i]
__device__ __forceinline__ float2 grad_adjoint_at(const tv_dims& d, const float2* uc, int64_t i0, int64_t i1, int64_t i2) {
    const int64_t s1 = d.n0, s2 = d.n0 * d.n1;
    const float2* u0 = uc;
    const float2* u1 = uc + d.vol;
    const float2* u2 = uc + 2 * d.vol;
    float2 s = make_float2(0.f, 0.f);
    if (i0 > 0) s = cadd(s, u0[-1]);
    if (i0 < d.n0 - 1) s = csub(s, u0[0]);
    if (i1 > 0) s = cadd(s, u1[-s1]);
    if (i1 < d.n1 - 1) s = csub(s, u1[0]);
    if (i2 > 0) s = cadd(s, u2[-s2]);
    if (i2 < d.n2 - 1) s = csub(s, u2[0]);
    return s;
}

// y[i, j] = beta * y[i, j] + alpha * (D^H u[:, j])[i]
template <bool READ_Y>
__global__ void __launch_bounds__(TV_BLK)
k_grad3h(tv_dims d, int64_t ncols, const float2* __restrict__ u, int64_t ldu, float2 a, float2 b,
         float2* __restrict__ y, int64_t ldy) {
    for_each_voxel(d, ncols, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        float2 r = cmul(a, grad_adjoint_at(d, u + j * ldu + i, i0, i1, i2));
        float2* yp = y + j * ldy + i;
        if (READ_Y) cfma(r, b, *yp);
        *yp = r;
    });
}

// u <- proj_mu(u + sigma * D(2 xn - xo)): w = 2 xn - xo at the voxel and at its three forward neighbours, the three
// components of u read and written once.  Compared as r^2 <= mu^2, as k_csoft compares its threshold.
__global__ void __launch_bounds__(TV_BLK)
k_tv_dual(tv_dims d, int64_t ncols, const float2* __restrict__ xn, int64_t ldn, const float2* __restrict__ xo, int64_t ldo,
          float sigma, float mu, float2* __restrict__ u, int64_t ldu) {
    const int64_t s1 = d.n0, s2 = d.n0 * d.n1;
    const float mu2 = mu * mu;
    for_each_voxel(d, ncols, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        const float2* nc = xn + j * ldn + i;
        const float2* oc = xo + j * ldo + i;
        float2* uc = u + j * ldu + i;
        auto w = [&](int64_t off) {
            const float2 p = nc[off], q = oc[off];
            return make_float2(fmaf(2.f, p.x, -q.x), fmaf(2.f, p.y, -q.y));
        };
        const float2 zero = make_float2(0.f, 0.f);
        const float2 w0 = w(0);
        const float2 g[3] = {i0 < d.n0 - 1 ? csub(w(1), w0) : zero, i1 < d.n1 - 1 ? csub(w(s1), w0) : zero,
                             i2 < d.n2 - 1 ? csub(w(s2), w0) : zero};
        float2 t[3];
        float r2 = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float2 v = uc[c * d.vol];
            t[c] = make_float2(fmaf(sigma, g[c].x, v.x), fmaf(sigma, g[c].y, v.y));
            r2 = fmaf(t[c].x, t[c].x, r2);
            r2 = fmaf(t[c].y, t[c].y, r2);
        }
        const float f = r2 <= mu2 ? 1.f : mu / sqrtf(r2);
#pragma unroll
        for (int c = 0; c < 3; ++c) uc[c * d.vol] = make_float2(t[c].x * f, t[c].y * f);
    });
}

// y[aN + i, t] = beta * y[aN + i, t] + alpha * (D_a x[:, t])[i], a = 0..2;  y[3N + i, t] likewise with x[i, t + 1] - x[i, t], 0 in
// the last frame;  READ_Y false: y is not read
template <bool READ_Y>
__global__ void __launch_bounds__(TV_BLK)
k_grad4(tv_dims d, int64_t nt, const float2* __restrict__ x, int64_t ldx, float2 a, float2 b,
        float2* __restrict__ y, int64_t ldy) {
    const int64_t s1 = d.n0, s2 = d.n0 * d.n1;
    for_each_voxel(d, nt, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        const float2* xc = x + j * ldx + i;
        float2* yc = y + j * ldy + i;
        const float2 zero = make_float2(0.f, 0.f);
        const float2 v = xc[0];
        const float2 g[4] = {i0 < d.n0 - 1 ? csub(xc[1], v) : zero, i1 < d.n1 - 1 ? csub(xc[s1], v) : zero,
                             i2 < d.n2 - 1 ? csub(xc[s2], v) : zero, j < nt - 1 ? csub(xc[ldx], v) : zero};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float2 r = cmul(a, g[c]);
            if (READ_Y) cfma(r, b, yc[c * d.vol]);
            yc[c * d.vol] = r;
        }
    });
}

// y[i, t] = beta * y[i, t] + alpha * (D4^H u)[i, t]
template <bool READ_Y>
__global__ void __launch_bounds__(TV_BLK)
k_grad4h(tv_dims d, int64_t nt, const float2* __restrict__ u, int64_t ldu, float2 a, float2 b,
         float2* __restrict__ y, int64_t ldy) {
    for_each_voxel(d, nt, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        const float2* uc = u + j * ldu + i;
        const float2* u3 = uc + 3 * d.vol;
        float2 s = grad_adjoint_at(d, uc, i0, i1, i2);
        if (j > 0) s = cadd(s, u3[-ldu]);
        if (j < nt - 1) s = csub(s, u3[0]);
        float2 r = cmul(a, s);
        float2* yp = y + j * ldy + i;
        if (READ_Y) cfma(r, b, *yp);
        *yp = r;
    });
}

// u <- proj(u + sigma * D4(2 xn - xo)): w = 2 xn - xo at the voxel, at its three forward neighbours and in the next frame, the
// four components of u read and written once.  Components 0..2 onto the ball r^2 <= mu^2 exactly as k_tv_dual does it, the
// fourth onto the disc |u_3|^2 <= mu_t^2.
__global__ void __launch_bounds__(TV_BLK)
k_tv4_dual(tv_dims d, int64_t nt, const float2* __restrict__ xn, int64_t ldn, const float2* __restrict__ xo, int64_t ldo,
           float sigma, float mu, float mu_t, float2* __restrict__ u, int64_t ldu) {
    const int64_t s1 = d.n0, s2 = d.n0 * d.n1;
    const float mu2 = mu * mu, mut2 = mu_t * mu_t;
    for_each_voxel(d, nt, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        const float2* nc = xn + j * ldn + i;
        const float2* oc = xo + j * ldo + i;
        float2* uc = u + j * ldu + i;
        auto w = [&](int64_t on, int64_t oo) {
            const float2 p = nc[on], q = oc[oo];
            return make_float2(fmaf(2.f, p.x, -q.x), fmaf(2.f, p.y, -q.y));
        };
        const float2 zero = make_float2(0.f, 0.f);
        const float2 w0 = w(0, 0);
        const float2 g[4] = {i0 < d.n0 - 1 ? csub(w(1, 1), w0) : zero, i1 < d.n1 - 1 ? csub(w(s1, s1), w0) : zero,
                             i2 < d.n2 - 1 ? csub(w(s2, s2), w0) : zero, j < nt - 1 ? csub(w(ldn, ldo), w0) : zero};
        float2 t[4];
        float r2 = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
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
        const float rt2 = fmaf(t[3].y, t[3].y, t[3].x * t[3].x);
        const float ft = rt2 <= mut2 ? 1.f : mu_t / sqrtf(rt2);
        uc[3 * d.vol] = make_float2(t[3].x * ft, t[3].y * ft);
    });
}

inline int64_t capg(int64_t v, int64_t hi) { return v < 1 ? 1 : (v > hi ? hi : v); }

tv_dims make_dims(int64_t n0, int64_t n1, int64_t n2) {
    int l = 3;
    while (l < 6 && (int64_t(1) << l) < n0) ++l;
    return tv_dims{n0, n1, n2, n0 * n1 * n2, l};
}

dim3 make_grid(const tv_dims& d, int64_t ncols) {
    const int64_t lx = int64_t(1) << d.lx_log2, rows = TV_BLK / lx;
    return dim3((unsigned)capg((d.n0 + lx - 1) / lx, 64), (unsigned)capg((d.n1 * d.n2 + rows - 1) / rows, TV_MAXROWS),
                (unsigned)capg(ncols, MAXG));
}

// whether the panels [p, p + ((ncols - 1) * ldp + rows_p) elements) and [q, ...) share a byte
bool overlap(const void* p, int64_t ldp, int64_t rows_p, const void* q, int64_t ldq, int64_t rows_q, int64_t ncols) {
    const uintptr_t p0 = (uintptr_t)p, p1 = p0 + (uintptr_t)((ncols - 1) * ldp + rows_p) * sizeof(float2);
    const uintptr_t q0 = (uintptr_t)q, q1 = q0 + (uintptr_t)((ncols - 1) * ldq + rows_q) * sizeof(float2);
    return p0 < q1 && q0 < p1;
}

}  // namespace

int ig_grad3_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, const void* x, int64_t ldx,
                 float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_grad3_c64: ctx is NULL");
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && ncols >= 0, "ig_grad3_c64: negative dimension");
    const tv_dims d = make_dims(n0, n1, n2);
    IG_REQUIRE(ctx, ldx >= d.vol && ldy >= 3 * d.vol, "ig_grad3_c64: leading dimension (%lld, %lld) below (N, 3N) for N = %lld",
               (long long)ldx, (long long)ldy, (long long)d.vol);
    if (d.vol == 0 || ncols == 0) return IG_OK;
    IG_REQUIRE(ctx, x && y, "ig_grad3_c64: NULL pointer");
    IG_REQUIRE(ctx, !overlap(x, ldx, d.vol, y, ldy, 3 * d.vol, ncols), "ig_grad3_c64: y overlaps x");
    if (int rc = ig_set_device(ctx)) return rc;
    const bool b0 = (br == 0.f && bi == 0.f);
    const float2 a = make_float2(ar, ai), b = make_float2(br, bi);
    const dim3 g = make_grid(d, ncols);
    ig_prof_scope prof(ctx, "grad3", (double)d.vol * ncols * (b0 ? 32.0 : 56.0));
    if (b0) hipLaunchKernelGGL(k_grad3<false>, g, dim3(TV_BLK), 0, ctx->stream, d, ncols, (const float2*)x, ldx, a, b, (float2*)y, ldy);
    else    hipLaunchKernelGGL(k_grad3<true>, g, dim3(TV_BLK), 0, ctx->stream, d, ncols, (const float2*)x, ldx, a, b, (float2*)y, ldy);
    IG_LAUNCH_CHECK(ctx, "k_grad3");
    return IG_OK;
}

int ig_grad3h_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, const void* u, int64_t ldu,
                  float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_grad3h_c64: ctx is NULL");
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && ncols >= 0, "ig_grad3h_c64: negative dimension");
    const tv_dims d = make_dims(n0, n1, n2);
    IG_REQUIRE(ctx, ldu >= 3 * d.vol && ldy >= d.vol, "ig_grad3h_c64: leading dimension (%lld, %lld) below (3N, N) for N = %lld",
               (long long)ldu, (long long)ldy, (long long)d.vol);
    if (d.vol == 0 || ncols == 0) return IG_OK;
    IG_REQUIRE(ctx, u && y, "ig_grad3h_c64: NULL pointer");
    IG_REQUIRE(ctx, !overlap(u, ldu, 3 * d.vol, y, ldy, d.vol, ncols), "ig_grad3h_c64: y overlaps u");
    if (int rc = ig_set_device(ctx)) return rc;
    const bool b0 = (br == 0.f && bi == 0.f);
    const float2 a = make_float2(ar, ai), b = make_float2(br, bi);
    const dim3 g = make_grid(d, ncols);
    ig_prof_scope prof(ctx, "grad3h", (double)d.vol * ncols * (b0 ? 32.0 : 40.0));
    if (b0) hipLaunchKernelGGL(k_grad3h<false>, g, dim3(TV_BLK), 0, ctx->stream, d, ncols, (const float2*)u, ldu, a, b, (float2*)y, ldy);
    else    hipLaunchKernelGGL(k_grad3h<true>, g, dim3(TV_BLK), 0, ctx->stream, d, ncols, (const float2*)u, ldu, a, b, (float2*)y, ldy);
    IG_LAUNCH_CHECK(ctx, "k_grad3h");
    return IG_OK;
}

int ig_tv_dual_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, const void* xn, int64_t ldn,
                   const void* xo, int64_t ldo, float sigma, float mu, void* u, int64_t ldu) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_tv_dual_c64: ctx is NULL");
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && ncols >= 0, "ig_tv_dual_c64: negative dimension");
    IG_REQUIRE(ctx, mu >= 0.f, "ig_tv_dual_c64: negative radius %g", (double)mu);
    const tv_dims d = make_dims(n0, n1, n2);
    IG_REQUIRE(ctx, ldn >= d.vol && ldo >= d.vol && ldu >= 3 * d.vol,
               "ig_tv_dual_c64: leading dimension (%lld, %lld, %lld) below (N, N, 3N) for N = %lld",
               (long long)ldn, (long long)ldo, (long long)ldu, (long long)d.vol);
    if (d.vol == 0 || ncols == 0) return IG_OK;
    IG_REQUIRE(ctx, xn && xo && u, "ig_tv_dual_c64: NULL pointer");
    IG_REQUIRE(ctx, !overlap(xn, ldn, d.vol, u, ldu, 3 * d.vol, ncols) && !overlap(xo, ldo, d.vol, u, ldu, 3 * d.vol, ncols),
               "ig_tv_dual_c64: u overlaps xn or xo");
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, "tv_dual", (double)d.vol * ncols * 64.0);
    hipLaunchKernelGGL(k_tv_dual, make_grid(d, ncols), dim3(TV_BLK), 0, ctx->stream, d, ncols, (const float2*)xn, ldn,
                       (const float2*)xo, ldo, sigma, mu, (float2*)u, ldu);
    IG_LAUNCH_CHECK(ctx, "k_tv_dual");
    return IG_OK;
}

int ig_grad4_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t nt, const void* x, int64_t ldx,
                 float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_grad4_c64: ctx is NULL");
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && nt >= 0, "ig_grad4_c64: negative dimension");
    const tv_dims d = make_dims(n0, n1, n2);
    IG_REQUIRE(ctx, ldx >= d.vol && ldy >= 4 * d.vol, "ig_grad4_c64: leading dimension (%lld, %lld) below (N, 4N) for N = %lld",
               (long long)ldx, (long long)ldy, (long long)d.vol);
    if (d.vol == 0 || nt == 0) return IG_OK;
    IG_REQUIRE(ctx, x && y, "ig_grad4_c64: NULL pointer");
    IG_REQUIRE(ctx, !overlap(x, ldx, d.vol, y, ldy, 4 * d.vol, nt), "ig_grad4_c64: y overlaps x");
    if (int rc = ig_set_device(ctx)) return rc;
    const bool b0 = (br == 0.f && bi == 0.f);
    const float2 a = make_float2(ar, ai), b = make_float2(br, bi);
    const dim3 g = make_grid(d, nt);
    ig_prof_scope prof(ctx, "grad4", (double)d.vol * (nt * (b0 ? 40.0 : 72.0) + (nt - 1) * 8.0));
    if (b0) hipLaunchKernelGGL(k_grad4<false>, g, dim3(TV_BLK), 0, ctx->stream, d, nt, (const float2*)x, ldx, a, b, (float2*)y, ldy);
    else    hipLaunchKernelGGL(k_grad4<true>, g, dim3(TV_BLK), 0, ctx->stream, d, nt, (const float2*)x, ldx, a, b, (float2*)y, ldy);
    IG_LAUNCH_CHECK(ctx, "k_grad4");
    return IG_OK;
}

int ig_grad4h_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t nt, const void* u, int64_t ldu,
                  float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_grad4h_c64: ctx is NULL");
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && nt >= 0, "ig_grad4h_c64: negative dimension");
    const tv_dims d = make_dims(n0, n1, n2);
    IG_REQUIRE(ctx, ldu >= 4 * d.vol && ldy >= d.vol, "ig_grad4h_c64: leading dimension (%lld, %lld) below (4N, N) for N = %lld",
               (long long)ldu, (long long)ldy, (long long)d.vol);
    if (d.vol == 0 || nt == 0) return IG_OK;
    IG_REQUIRE(ctx, u && y, "ig_grad4h_c64: NULL pointer");
    IG_REQUIRE(ctx, !overlap(u, ldu, 4 * d.vol, y, ldy, d.vol, nt), "ig_grad4h_c64: y overlaps u");
    if (int rc = ig_set_device(ctx)) return rc;
    const bool b0 = (br == 0.f && bi == 0.f);
    const float2 a = make_float2(ar, ai), b = make_float2(br, bi);
    const dim3 g = make_grid(d, nt);
    ig_prof_scope prof(ctx, "grad4h", (double)d.vol * (nt * (b0 ? 32.0 : 40.0) + (nt - 1) * 16.0));
    if (b0) hipLaunchKernelGGL(k_grad4h<false>, g, dim3(TV_BLK), 0, ctx->stream, d, nt, (const float2*)u, ldu, a, b, (float2*)y, ldy);
    else    hipLaunchKernelGGL(k_grad4h<true>, g, dim3(TV_BLK), 0, ctx->stream, d, nt, (const float2*)u, ldu, a, b, (float2*)y, ldy);
    IG_LAUNCH_CHECK(ctx, "k_grad4h");
    return IG_OK;
}

int ig_tv4_dual_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t nt, const void* xn, int64_t ldn,
                    const void* xo, int64_t ldo, float sigma, float mu, float mu_t, void* u, int64_t ldu) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_tv4_dual_c64: ctx is NULL");
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && nt >= 0, "ig_tv4_dual_c64: negative dimension");
    IG_REQUIRE(ctx, mu >= 0.f && mu_t >= 0.f, "ig_tv4_dual_c64: negative radius (%g, %g)", (double)mu, (double)mu_t);
    const tv_dims d = make_dims(n0, n1, n2);
    IG_REQUIRE(ctx, ldn >= d.vol && ldo >= d.vol && ldu >= 4 * d.vol,
               "ig_tv4_dual_c64: leading dimension (%lld, %lld, %lld) below (N, N, 4N) for N = %lld",
               (long long)ldn, (long long)ldo, (long long)ldu, (long long)d.vol);
    if (d.vol == 0 || nt == 0) return IG_OK;
    IG_REQUIRE(ctx, xn && xo && u, "ig_tv4_dual_c64: NULL pointer");
    IG_REQUIRE(ctx, !overlap(xn, ldn, d.vol, u, ldu, 4 * d.vol, nt) && !overlap(xo, ldo, d.vol, u, ldu, 4 * d.vol, nt),
               "ig_tv4_dual_c64: u overlaps xn or xo");
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, "tv4_dual", (double)d.vol * (nt * 80.0 + (nt - 1) * 16.0));
    hipLaunchKernelGGL(k_tv4_dual, make_grid(d, nt), dim3(TV_BLK), 0, ctx->stream, d, nt, (const float2*)xn, ldn,
                       (const float2*)xo, ldo, sigma, mu, mu_t, (float2*)u, ldu);
    IG_LAUNCH_CHECK(ctx, "k_tv4_dual");
    return IG_OK;
}
