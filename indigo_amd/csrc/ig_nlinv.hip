// The model kernels of NLINV, the joint estimation of the image and the coil sensitivities (indigo_amd.nlinv, Backend.nlinv_product,
// Backend.sobolev_weight, operators.NlinvProduct, operators.SobolevCoils).
//
// ig_nlinv_product_c64: the derivative of the bilinear coil product rho * c_c at the point (rho, c) and its adjoint
//
//   forward : y[i, c]     = beta*y[i, c]     + alpha * ( x[i, 0] * coils[i, c] + rho[i] * x[i, 1 + c] )      x: n x (1 + nc), y: n x nc
//   adjoint : y[i, 0]     = beta*y[i, 0]     + alpha * sum_c conj(coils[i, c]) * x[i, c]                      x: n x nc, y: n x (1 + nc)
//             y[i, 1 + c] = beta*y[i, 1 + c] + alpha * conj(rho[i]) * x[i, c]
//
// All panels are coil-major (column-major with a leading dimension), as KronI(C, NUFFT) takes and leaves its coil images.  Both
// directions are one pass of 8 n (3 nc + 2) bytes: ig_maps.hip's coil-major pattern, one thread per voxel -- or per pair of
// neighbouring voxels with 16-byte accesses when n, the leading dimensions and the pointers allow --, the voxel's rho and x[i, 0]
// (forward) or its accumulator of the sum over the coils (adjoint) in registers across the coil loop, every x element read once.
// Every element is formed by the same sequence of fused multiply-adds in both forms: the same bits.  No atomics, 64-bit offsets.
//
// ig_sobolev_weight_c64: y[k, j] = scale * w(k) * x[k, j] with the k-space smoothness weight of the coil penalty
//
//   w(k) = (1 + a |kappa|^2)^(-b/2),   kappa_a = k'_a / n_a,   k'_a = k_a if 2 k_a <= n_a else k_a - n_a
//
// on the points of an uncentred n0 x n1 x n2 transform.  One thread per k-space point forms w in double from its integer
// coordinates, rounds it to float32 once and loops over the columns: no weight array, 16 bytes per element and nothing else.
// k' enters only through its square, so w(k) and w(-k) are the same bits.
#include "ig_common.h"

namespace {

constexpr int NLINV_BLK = 256;
constexpr int64_t NLINV_MAXGRID = 1 << 20;   // workgroups; the item loop strides beyond that

// nv work items of V voxels each (n = nv * V)
template <int V, bool BETA>
__global__ void __launch_bounds__(NLINV_BLK)
k_nlinv_fwd(int64_t nv, int64_t nc, const float2* __restrict__ rho, const float2* __restrict__ coils, int64_t ldc,
            const float2* __restrict__ x, int64_t ldx, float2 a, float2 b, float2* __restrict__ y, int64_t ldy) {
    for (int64_t it = (int64_t)blockIdx.x * NLINV_BLK + threadIdx.x; it < nv; it += (int64_t)gridDim.x * NLINV_BLK) {
        const int64_t i = it * V;
        float2 r[V], d[V];
        ldv<V>(r, rho + i);
        ldv<V>(d, x + i);
        const float2* cp = coils + i;
        const float2* xp = x + i + ldx;
        float2* yp = y + i;
#pragma unroll 2
        for (int64_t c = 0; c < nc; ++c, cp += ldc, xp += ldx, yp += ldy) {
            float2 s[V], xv[V], out[V];
            ldv<V>(s, cp);
            ldv<V>(xv, xp);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float2 t = cmul(d[v], s[v]);
                cfma(t, r[v], xv[v]);
                out[v] = cmul(a, t);
            }
            if (BETA) {
                float2 o[V];
                ldv<V>(o, yp);
#pragma unroll
                for (int v = 0; v < V; ++v) cfma(out[v], b, o[v]);
            }
            stv<V>(yp, out);
        }
    }
}

template <int V, bool BETA>
__global__ void __launch_bounds__(NLINV_BLK)
k_nlinv_adj(int64_t nv, int64_t nc, const float2* __restrict__ rho, const float2* __restrict__ coils, int64_t ldc,
            const float2* __restrict__ x, int64_t ldx, float2 a, float2 b, float2* __restrict__ y, int64_t ldy) {
    for (int64_t it = (int64_t)blockIdx.x * NLINV_BLK + threadIdx.x; it < nv; it += (int64_t)gridDim.x * NLINV_BLK) {
        const int64_t i = it * V;
        float2 r[V], acc[V];
        ldv<V>(r, rho + i);
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = make_float2(0.f, 0.f);
        const float2* cp = coils + i;
        const float2* xp = x + i;
        float2* yp = y + i + ldy;
#pragma unroll 2
        for (int64_t c = 0; c < nc; ++c, cp += ldc, xp += ldx, yp += ldy) {
            float2 s[V], xv[V], out[V];
            ldv<V>(s, cp);
            ldv<V>(xv, xp);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                cfmac(acc[v], s[v], xv[v]);
                out[v] = cmul(a, cmulc(r[v], xv[v]));
            }
            if (BETA) {
                float2 o[V];
                ldv<V>(o, yp);
#pragma unroll
                for (int v = 0; v < V; ++v) cfma(out[v], b, o[v]);
            }
            stv<V>(yp, out);
        }
        float2 out[V];
#pragma unroll
        for (int v = 0; v < V; ++v) out[v] = cmul(a, acc[v]);
        if (BETA) {
            float2 o[V];
            ldv<V>(o, y + i);
#pragma unroll
            for (int v = 0; v < V; ++v) cfma(out[v], b, o[v]);
        }
        stv<V>(y + i, out);
    }
}

template <int V>
void nlinv_launch(ig_ctx* ctx, bool adjoint, bool beta, int64_t n, int64_t nc, const float2* rho, const float2* coils, int64_t ldc,
                  const float2* x, int64_t ldx, float2 a, float2 b, float2* y, int64_t ldy) {
    const int64_t nv = n / V;
    const dim3 grid = ig_grid_1d(nv, NLINV_BLK, NLINV_MAXGRID), block(NLINV_BLK);
    if (adjoint) {
        if (beta) hipLaunchKernelGGL((k_nlinv_adj<V, true>), grid, block, 0, ctx->stream, nv, nc, rho, coils, ldc, x, ldx, a, b, y, ldy);
        else      hipLaunchKernelGGL((k_nlinv_adj<V, false>), grid, block, 0, ctx->stream, nv, nc, rho, coils, ldc, x, ldx, a, b, y, ldy);
    } else {
        if (beta) hipLaunchKernelGGL((k_nlinv_fwd<V, true>), grid, block, 0, ctx->stream, nv, nc, rho, coils, ldc, x, ldx, a, b, y, ldy);
        else      hipLaunchKernelGGL((k_nlinv_fwd<V, false>), grid, block, 0, ctx->stream, nv, nc, rho, coils, ldc, x, ldx, a, b, y, ldy);
    }
}

// x and y may be the same panel: no __restrict__; a thread reads an element before it writes the same one
__global__ void __launch_bounds__(NLINV_BLK)
k_sobolev(int64_t n, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, double a, double e /* -b/2 */, double scale,
          const float2* x, int64_t ldx, float2* y, int64_t ldy) {
    for (int64_t k = (int64_t)blockIdx.x * NLINV_BLK + threadIdx.x; k < n; k += (int64_t)gridDim.x * NLINV_BLK) {
        const int64_t k0 = k % n0, q = k / n0, k1 = q % n1, k2 = q / n1;
        const int64_t s0 = 2 * k0 <= n0 ? k0 : k0 - n0, s1 = 2 * k1 <= n1 ? k1 : k1 - n1, s2 = 2 * k2 <= n2 ? k2 : k2 - n2;
        const double f0 = (double)s0 / (double)n0, f1 = (double)s1 / (double)n1, f2 = (double)s2 / (double)n2;
        const double r2 = __dadd_rn(__dadd_rn(__dmul_rn(f0, f0), __dmul_rn(f1, f1)), __dmul_rn(f2, f2));
        const float w = (float)pow(__dadd_rn(1.0, __dmul_rn(a, r2)), e);    // the one rounding of w
        const float sw = (float)((double)w * scale);                       // (float x double is exact to 53 bits: one rounding)
        const float2* xp = x + k;
        float2* yp = y + k;
        for (int64_t j = 0; j < ncols; ++j, xp += ldx, yp += ldy) {
            const float2 v = *xp;
            *yp = make_float2(sw * v.x, sw * v.y);
        }
    }
}

}  // namespace

int ig_nlinv_product_c64(ig_ctx* ctx, int64_t n, int64_t nc, const void* rho, const void* coils, int64_t ldc, int adjoint,
                         const void* x, int64_t ldx, float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_nlinv_product_c64: ctx is NULL");
    if (n < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_nlinv_product_c64: %lld voxels, at least 1 is supported", (long long)n);
    if (nc < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_nlinv_product_c64: %lld coils, at least 1 is supported", (long long)nc);
    IG_REQUIRE(ctx, ldc >= n, "ig_nlinv_product_c64: leading dimension %lld of the coils below n = %lld", (long long)ldc, (long long)n);
    IG_REQUIRE(ctx, ldx >= n, "ig_nlinv_product_c64: leading dimension %lld of x below n = %lld", (long long)ldx, (long long)n);
    IG_REQUIRE(ctx, ldy >= n, "ig_nlinv_product_c64: leading dimension %lld of y below n = %lld", (long long)ldy, (long long)n);
    IG_REQUIRE(ctx, rho && coils && x && y, "ig_nlinv_product_c64: NULL pointer");
    const int64_t cols_x = adjoint ? nc : nc + 1, cols_y = adjoint ? nc + 1 : nc;
    IG_REQUIRE(ctx, !ig_panels_overlap(y, ldy, n, cols_y, x, ldx, n, cols_x), "ig_nlinv_product_c64: y overlaps x");
    IG_REQUIRE(ctx, !ig_panels_overlap(y, ldy, n, cols_y, rho, n, n, 1), "ig_nlinv_product_c64: y overlaps rho");
    IG_REQUIRE(ctx, !ig_panels_overlap(y, ldy, n, cols_y, coils, ldc, n, nc), "ig_nlinv_product_c64: y overlaps the coils");
    if (int rc = ig_set_device(ctx)) return rc;
    const bool beta = !(br == 0.f && bi == 0.f), adj = adjoint != 0;
    const float2 a = make_float2(ar, ai), b = make_float2(br, bi);
    ig_prof_scope prof(ctx, adj ? "nlinv_product_adj" : "nlinv_product_fwd",
                       8.0 * (double)n * ((double)(3 * nc + 2) + (beta ? (double)cols_y : 0.0)));
    // pairs of voxels: every column of every panel starts on a 16-byte boundary and holds whole pairs
    const bool wide = n % 2 == 0 && ldc % 2 == 0 && ldx % 2 == 0 && ldy % 2 == 0 && (uintptr_t)rho % 16 == 0 && (uintptr_t)coils % 16 == 0 &&
                      (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0;
    if (wide) nlinv_launch<2>(ctx, adj, beta, n, nc, (const float2*)rho, (const float2*)coils, ldc, (const float2*)x, ldx, a, b, (float2*)y, ldy);
    else      nlinv_launch<1>(ctx, adj, beta, n, nc, (const float2*)rho, (const float2*)coils, ldc, (const float2*)x, ldx, a, b, (float2*)y, ldy);
    IG_LAUNCH_CHECK(ctx, adj ? "k_nlinv_adj" : "k_nlinv_fwd");
    return IG_OK;
}

int ig_sobolev_weight_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, double a, double b, double scale,
                          const void* x, int64_t ldx, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_sobolev_weight_c64: ctx is NULL");
    if (n0 < 1 || n1 < 1 || n2 < 1 || ncols < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_sobolev_weight_c64: a %lld x %lld x %lld volume and %lld columns, at least 1 each is supported",
                       (long long)n0, (long long)n1, (long long)n2, (long long)ncols);
    if (!(a >= 0.0))
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_sobolev_weight_c64: a = %g, a non-negative value is supported", a);
    const int64_t n = n0 * n1 * n2;
    IG_REQUIRE(ctx, ldx >= n && ldy >= n, "ig_sobolev_weight_c64: leading dimensions (%lld, %lld) below n = %lld", (long long)ldx, (long long)ldy, (long long)n);
    IG_REQUIRE(ctx, x && y, "ig_sobolev_weight_c64: NULL pointer");
    const bool in_place = x == y && ldx == ldy;
    IG_REQUIRE(ctx, in_place || !ig_panels_overlap(y, ldy, n, ncols, x, ldx, n, ncols), "ig_sobolev_weight_c64: y overlaps x (only y == x with ldy == ldx is in place)");
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, "sobolev_weight", 16.0 * (double)n * (double)ncols);
    const dim3 grid = ig_grid_1d(n, NLINV_BLK, NLINV_MAXGRID), block(NLINV_BLK);
    hipLaunchKernelGGL(k_sobolev, grid, block, 0, ctx->stream, n, n0, n1, n2, ncols, a, -0.5 * b, scale, (const float2*)x, ldx, (float2*)y, ldy);
    IG_LAUNCH_CHECK(ctx, "k_sobolev");
    return IG_OK;
}
