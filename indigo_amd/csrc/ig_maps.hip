// The per-voxel C x M coil-map product of soft-SENSE and its adjoint (Backend.coil_maps, operators.CoilMaps, operators.ZpadFFTMaps,
// pics on a scan with several sets of maps).
//
//   forward : y[i, c] = beta*y[i, c] + alpha * sum_m      S[i, c, m]  * x[i, m]      x: n x nm images, y: the nc coil images
//   adjoint : y[i, m] = beta*y[i, m] + alpha * sum_c conj(S[i, c, m]) * x[i, c]      x: the nc coil images, y: n x nm images
//
// The image side is a column-major panel (ldi >= n).  The coil side is coil-major (element (i, c) at i + sc*c, sc >= n) or
// coil-interleaved (element (i, c) at i*width + c, width in {2, 4, 8, 16}, nc <= width: the layout-2 form of ZpadFFT's weights and
// of the cropped transform's result; slots c >= nc are the zero-weight padding coils).  S is nm dense planes in the form of the
// coil side (n*nc or n*width elements each).  Both directions are single-pass streams of 8 n (nc nm + nc + nm) bytes: the
// voxel's nm values (forward, alpha already applied) or nm accumulators (adjoint) stay in registers, so nm has the compile-time
// bound 4.  No atomics, no second pass over y.  All element offsets are 64-bit.
//
// Coil-major: ig_basis's pattern.  One thread per voxel -- or per pair of neighbouring voxels with 16-byte accesses when n, the
// leading dimensions and the pointers allow --, a loop over the coils that reads or writes one fully coalesced column element
// per lane.
// Coil-interleaved: a voxel's row of `width` slots is width / CV neighbouring lanes with CV = 2 slots (16 bytes) each, or CV = 1
// (8 bytes) when a pointer is not 16-byte aligned: consecutive lanes cover consecutive memory of the coil side and of S, and the
// lanes of a row read the same image elements (one address per row).  The adjoint's sum over the row is a butterfly over those
// lanes (width / CV <= 16 divides the wave, a row never straddles two waves); a thread that owned the whole 16- to 128-byte row
// would need no cross-lane step, but its wave would touch 64 rows at a stride of up to 128 bytes with every access.  A lane sums
// its two slots from separately rounded products, so both CV give the same tree and the same bits.  On forward the padding
// slots are written as zero; on adjoint they are not loaded at all (x or S: a pair that straddles nc loads its first slot alone).
#include "ig_common.h"

namespace {

constexpr int MAPS_MAXM = 4;
constexpr int MAPS_BLK = 256;
constexpr int64_t MAPS_MAXGRID = 1 << 20;   // workgroups; the item loop strides beyond that

// ---- coil-major -------------------------------------------------------------------------------------------------------------
// nv work items of V voxels each (n = nv * V); plane = n * nc elements of S per set of maps
template <int NM, int V, bool BETA>
__global__ void __launch_bounds__(MAPS_BLK)
k_maps_fwd(int64_t nv, int64_t n, int64_t nc, const float2* __restrict__ S, const float2* __restrict__ x, int64_t ldi,
           float2 a, float2 b, float2* __restrict__ y, int64_t sc) {
    const int64_t plane = n * nc;
    for (int64_t it = (int64_t)blockIdx.x * MAPS_BLK + threadIdx.x; it < nv; it += (int64_t)gridDim.x * MAPS_BLK) {
        const int64_t i = it * V;
        float2 xr[NM][V];
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            ldv<V>(xr[m], x + i + (int64_t)m * ldi);
#pragma unroll
            for (int v = 0; v < V; ++v) xr[m][v] = cmul(a, xr[m][v]);
        }
        const float2* sp = S + i;
        float2* yp = y + i;
#pragma unroll 2
        for (int64_t c = 0; c < nc; ++c, sp += n, yp += sc) {
            float2 acc[V];
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = make_float2(0.f, 0.f);
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                float2 s[V];
                ldv<V>(s, sp + (int64_t)m * plane);
#pragma unroll
                for (int v = 0; v < V; ++v) cfma(acc[v], s[v], xr[m][v]);
            }
            if (BETA) {
                float2 o[V];
                ldv<V>(o, yp);
#pragma unroll
                for (int v = 0; v < V; ++v) cfma(acc[v], b, o[v]);
            }
            stv<V>(yp, acc);
        }
    }
}

template <int NM, int V, bool BETA>
__global__ void __launch_bounds__(MAPS_BLK)
k_maps_adj(int64_t nv, int64_t n, int64_t nc, const float2* __restrict__ S, const float2* __restrict__ x, int64_t sc,
           float2 a, float2 b, float2* __restrict__ y, int64_t ldi) {
    const int64_t plane = n * nc;
    for (int64_t it = (int64_t)blockIdx.x * MAPS_BLK + threadIdx.x; it < nv; it += (int64_t)gridDim.x * MAPS_BLK) {
        const int64_t i = it * V;
        float2 acc[NM][V];
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[m][v] = make_float2(0.f, 0.f);
        const float2* sp = S + i;
        const float2* xp = x + i;
#pragma unroll 2
        for (int64_t c = 0; c < nc; ++c, sp += n, xp += sc) {
            float2 xv[V];
            ldv<V>(xv, xp);
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                float2 s[V];
                ldv<V>(s, sp + (int64_t)m * plane);
#pragma unroll
                for (int v = 0; v < V; ++v) cfmac(acc[m][v], s[v], xv[v]);
            }
        }
        float2* yp = y + i;
#pragma unroll
        for (int m = 0; m < NM; ++m, yp += ldi) {
            float2 r[V];
#pragma unroll
            for (int v = 0; v < V; ++v) r[v] = cmul(a, acc[m][v]);
            if (BETA) {
                float2 o[V];
                ldv<V>(o, yp);
#pragma unroll
                for (int v = 0; v < V; ++v) cfma(r[v], b, o[v]);
            }
            stv<V>(yp, r);
        }
    }
}

// ---- coil-interleaved -------------------------------------------------------------------------------------------------------
// nitems = n * G work items, G = width / CV lanes per voxel (a power of two <= 16); plane = n * width elements of S per set.
template <int NM, int CV, bool BETA>
__global__ void __launch_bounds__(MAPS_BLK)
k_maps_il_fwd(int64_t nitems, int64_t n, int nc, int width, int lg /* log2 G */, const float2* __restrict__ S,
              const float2* __restrict__ x, int64_t ldi, float2 a, float2 b, float2* __restrict__ y) {
    const int64_t plane = n * (int64_t)width;
    for (int64_t it = (int64_t)blockIdx.x * MAPS_BLK + threadIdx.x; it < nitems; it += (int64_t)gridDim.x * MAPS_BLK) {
        const int64_t i = it >> lg;
        const int c0 = (int)(it - (i << lg)) * CV;
        const int64_t e = i * width + c0;                                   // = it * CV: consecutive lanes, consecutive memory
        float2 acc[CV];
#pragma unroll
        for (int v = 0; v < CV; ++v) acc[v] = make_float2(0.f, 0.f);
        if (c0 < nc) {
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const float2 xm = cmul(a, x[i + (int64_t)m * ldi]);
                float2 s[CV];
                ldv<CV>(s, S + e + (int64_t)m * plane);
#pragma unroll
                for (int v = 0; v < CV; ++v) cfma(acc[v], s[v], xm);
            }
            if (BETA) {
                float2 o[CV];
                ldv<CV>(o, y + e);
#pragma unroll
                for (int v = 0; v < CV; ++v) cfma(acc[v], b, o[v]);
            }
        }
#pragma unroll
        for (int v = 0; v < CV; ++v)
            if (c0 + v >= nc) acc[v] = make_float2(0.f, 0.f);               // the padding coils: exact zeros
        stv<CV>(y + e, acc);
    }
}

// Every lane of a wave runs the butterfly (a lane past the end carries zeros): the item loop has the same trip count in all
// lanes of a workgroup.
template <int NM, int CV, bool BETA>
__global__ void __launch_bounds__(MAPS_BLK)
k_maps_il_adj(int64_t nitems, int64_t n, int nc, int width, int lg, const float2* __restrict__ S, const float2* __restrict__ x,
              float2 a, float2 b, float2* __restrict__ y, int64_t ldi) {
    const int64_t plane = n * (int64_t)width;
    const int G = 1 << lg;
    for (int64_t base = (int64_t)blockIdx.x * MAPS_BLK; base < nitems; base += (int64_t)gridDim.x * MAPS_BLK) {
        const int64_t it = base + threadIdx.x;
        const bool active = it < nitems;
        const int64_t i = it >> lg;
        const int p = (int)(it - (i << lg)), c0 = p * CV;
        const int64_t e = i * width + c0;
        float2 acc[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) acc[m] = make_float2(0.f, 0.f);
        if (active && c0 < nc) {
            if (CV == 2 && c0 + 1 < nc) {
                float2 xv[2];
                ldv<2>(xv, x + e);
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    float2 s[2];
                    ldv<2>(s, S + e + (int64_t)m * plane);
                    const float2 p0 = cmulc(s[0], xv[0]), p1 = cmulc(s[1], xv[1]);
                    acc[m] = cadd(p0, p1);
                }
            } else {                                                        // one slot: CV = 1, or the last real coil of an odd nc
                const float2 xv = x[e];
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    acc[m] = cmulc(S[e + (int64_t)m * plane], xv);
                    if (CV == 2) acc[m] = cadd(acc[m], make_float2(0.f, 0.f));      // (the sum CV = 1 forms with the padding lane)
                }
            }
        }
        for (int d = 1; d < G; d <<= 1) {
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                acc[m].x += __shfl_xor(acc[m].x, d);
                acc[m].y += __shfl_xor(acc[m].y, d);
            }
        }
        if (active && p == 0) {
            float2* yp = y + i;
#pragma unroll
            for (int m = 0; m < NM; ++m, yp += ldi) {
                float2 r = cmul(a, acc[m]);
                if (BETA) cfma(r, b, *yp);
                *yp = r;
            }
        }
    }
}

template <int NM, int V>
void maps_launch_cm(ig_ctx* ctx, bool adjoint, bool beta, int64_t n, int64_t nc, const float2* S, const float2* x, float2 a, float2 b,
                    float2* y, int64_t ldi, int64_t sc) {
    const int64_t nv = n / V;
    const dim3 grid = ig_grid_1d(nv, MAPS_BLK, MAPS_MAXGRID), block(MAPS_BLK);
    if (adjoint) {
        if (beta) hipLaunchKernelGGL((k_maps_adj<NM, V, true>), grid, block, 0, ctx->stream, nv, n, nc, S, x, sc, a, b, y, ldi);
        else      hipLaunchKernelGGL((k_maps_adj<NM, V, false>), grid, block, 0, ctx->stream, nv, n, nc, S, x, sc, a, b, y, ldi);
    } else {
        if (beta) hipLaunchKernelGGL((k_maps_fwd<NM, V, true>), grid, block, 0, ctx->stream, nv, n, nc, S, x, ldi, a, b, y, sc);
        else      hipLaunchKernelGGL((k_maps_fwd<NM, V, false>), grid, block, 0, ctx->stream, nv, n, nc, S, x, ldi, a, b, y, sc);
    }
}

template <int NM, int CV>
void maps_launch_il(ig_ctx* ctx, bool adjoint, bool beta, int64_t n, int nc, int width, const float2* S, const float2* x, float2 a, float2 b,
                    float2* y, int64_t ldi) {
    int lg = 0;
    while ((CV << lg) < width) ++lg;
    const int64_t nitems = n << lg;
    const dim3 grid = ig_grid_1d(nitems, MAPS_BLK, MAPS_MAXGRID), block(MAPS_BLK);
    if (adjoint) {
        if (beta) hipLaunchKernelGGL((k_maps_il_adj<NM, CV, true>), grid, block, 0, ctx->stream, nitems, n, nc, width, lg, S, x, a, b, y, ldi);
        else      hipLaunchKernelGGL((k_maps_il_adj<NM, CV, false>), grid, block, 0, ctx->stream, nitems, n, nc, width, lg, S, x, a, b, y, ldi);
    } else {
        if (beta) hipLaunchKernelGGL((k_maps_il_fwd<NM, CV, true>), grid, block, 0, ctx->stream, nitems, n, nc, width, lg, S, x, ldi, a, b, y);
        else      hipLaunchKernelGGL((k_maps_il_fwd<NM, CV, false>), grid, block, 0, ctx->stream, nitems, n, nc, width, lg, S, x, ldi, a, b, y);
    }
}

}  // namespace

int ig_coil_maps_c64(ig_ctx* ctx, int64_t n, int64_t nc, int64_t nm, const void* maps, int adjoint, const void* x,
                     float ar, float ai, float br, float bi, void* y, int64_t ldi, int64_t sg, int64_t sc) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_coil_maps_c64: ctx is NULL");
    if (nm < 1 || nm > MAPS_MAXM)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_coil_maps_c64: %lld sets of maps, between 1 and %d are supported", (long long)nm, MAPS_MAXM);
    if (n < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_coil_maps_c64: %lld voxels, at least 1 is supported", (long long)n);
    if (nc < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_coil_maps_c64: %lld coils, at least 1 is supported", (long long)nc);
    const bool il = sg != 1;
    if (il) {
        if (!(sc == 1 && (sg == 2 || sg == 4 || sg == 8 || sg == 16)))
            return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_coil_maps_c64: strides (%lld, %lld): coil-major (sg = 1, sc >= n) or coil-interleaved "
                           "(sc = 1, sg = width 2, 4, 8 or 16) coil images", (long long)sg, (long long)sc);
        if (nc > sg)
            return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_coil_maps_c64: %lld coils in rows of width %lld", (long long)nc, (long long)sg);
    } else {
        IG_REQUIRE(ctx, sc >= n, "ig_coil_maps_c64: coil stride %lld below n = %lld", (long long)sc, (long long)n);
    }
    IG_REQUIRE(ctx, ldi >= n, "ig_coil_maps_c64: leading dimension %lld of the images below n = %lld", (long long)ldi, (long long)n);
    IG_REQUIRE(ctx, maps && x && y, "ig_coil_maps_c64: NULL pointer");
    const int64_t ext_i = (nm - 1) * ldi + n;                               // elements of the image side, of the coil side, of S
    const int64_t ext_c = il ? n * sg : (nc - 1) * sc + n;
    const int64_t ext_s = nm * n * (il ? sg : nc);
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (uintptr_t)(adjoint ? ext_c : ext_i) * sizeof(float2);
    const uintptr_t y0 = (uintptr_t)y, y1 = y0 + (uintptr_t)(adjoint ? ext_i : ext_c) * sizeof(float2);
    const uintptr_t s0 = (uintptr_t)maps, s1 = s0 + (uintptr_t)ext_s * sizeof(float2);
    IG_REQUIRE(ctx, !ig_bytes_overlap(x0, x1, y0, y1), "ig_coil_maps_c64: y overlaps x");
    IG_REQUIRE(ctx, !ig_bytes_overlap(s0, s1, y0, y1), "ig_coil_maps_c64: y overlaps the maps");
    if (int rc = ig_set_device(ctx)) return rc;
    const bool beta = !(br == 0.f && bi == 0.f);
    const float2 a = make_float2(ar, ai), b = make_float2(br, bi);
    const float2* S = (const float2*)maps;
    const float2* xp = (const float2*)x;
    float2* yp = (float2*)y;
    const double rows_y = adjoint ? (double)nm : (double)nc;
    ig_prof_scope prof(ctx, adjoint ? "coil_maps_adj" : "coil_maps_fwd", 8.0 * (double)n * ((double)(nc * nm + nc + nm) + (beta ? rows_y : 0.0)));
    const bool adj = adjoint != 0;
    if (il) {
        // pairs of slots: every row of the coil side and of S starts on a 16-byte boundary (the width is even)
        const uintptr_t cside = adj ? x0 : y0;
        const bool wide = cside % 16 == 0 && s0 % 16 == 0;
#define IG_MAPS_IL(NM)                                                                                        \
        do {                                                                                                  \
            if (wide) maps_launch_il<NM, 2>(ctx, adj, beta, n, (int)nc, (int)sg, S, xp, a, b, yp, ldi);       \
            else maps_launch_il<NM, 1>(ctx, adj, beta, n, (int)nc, (int)sg, S, xp, a, b, yp, ldi);            \
        } while (0)
        if (nm == 1) IG_MAPS_IL(1); else if (nm == 2) IG_MAPS_IL(2); else if (nm == 3) IG_MAPS_IL(3); else IG_MAPS_IL(4);
#undef IG_MAPS_IL
    } else {
        // pairs of voxels: every column of the images, every coil image and every plane of S starts on a 16-byte boundary and
        // holds whole pairs
        const bool wide = n % 2 == 0 && ldi % 2 == 0 && sc % 2 == 0 && x0 % 16 == 0 && y0 % 16 == 0 && s0 % 16 == 0;
#define IG_MAPS_CM(NM)                                                                                        \
        do {                                                                                                  \
            if (wide) maps_launch_cm<NM, 2>(ctx, adj, beta, n, nc, S, xp, a, b, yp, ldi, sc);                 \
            else maps_launch_cm<NM, 1>(ctx, adj, beta, n, nc, S, xp, a, b, yp, ldi, sc);                      \
        } while (0)
        if (nm == 1) IG_MAPS_CM(1); else if (nm == 2) IG_MAPS_CM(2); else if (nm == 3) IG_MAPS_CM(3); else IG_MAPS_CM(4);
#undef IG_MAPS_CM
    }
    IG_LAUNCH_CHECK(ctx, adjoint ? "k_maps_adj" : "k_maps_fwd");
    return IG_OK;
}
