// The two streaming passes of the time-segmented off-resonance model (Backend.segment_phase, Backend.segment_combine,
// operators.SegmentPhase, operators.SegmentCombine, pics --fmap).
//
//   exp(-2 pi i f(r) t_j)  ~  sum_{l < L} b_l(t_j) exp(-2 pi i f(r) tau_l),      tau_l = tau0 + l dtau
//
// ig_fmap_phase_c64, f the n float32 values of the field map in Hz, x and y column-major panels of n-voxel images:
//   forward : y[i, l] = beta*y[i, l] + alpha * exp(-2 pi i f[i] tau_l) * x[i]               x: n x 1, y: n x L
//   adjoint : y[i]    = beta*y[i]    + alpha * sum_l exp(+2 pi i f[i] tau_l) * x[i, l]      x: n x L, y: n x 1
// ig_fmap_combine_c64, b the P x L interpolator table (column-major, ldb >= P), row r of the panels uses b[r mod P, .]:
//   forward : y[r]    = beta*y[r]    + alpha * sum_l      b[r mod P, l]  * x[r, l]          x: n x L, y: n x 1
//   adjoint : y[r, l] = beta*y[r, l] + alpha *       conj(b[r mod P, l]) * x[r]             x: n x 1, y: n x L
//
// All four are single-pass streams: 8 n (L + 1) bytes, 4 n more for f, and 8 n (columns of y) more when beta != 0; the table is
// P L elements that the n / P periods share, so it is served by the caches whenever the panels are large.  One thread per row,
// or per pair of neighbouring rows with 16-byte accesses when n, the leading dimensions and the pointers allow.  L is a run-time
// loop bound (1..16): the forward phase and the adjoint combine keep one input value per row, the other two one accumulator.
// The phase: f tau reaches tens of cycles, where a float32 product is already 1e-5 rad off, so p = f tau_l is formed in double,
// reduced by rint(p) to [-1/2, 1/2], converted to float (2e-7 rad) and handed to sincospif, which works in half revolutions: no
// recurrence over l, every segment's phase is as accurate as the first.  No atomics, no second pass over y.  All element offsets
// are 64-bit.
#include "ig_common.h"

namespace {

constexpr int FMAP_MAXL = 16;          // time segments
constexpr int FMAP_BLK = 256;
constexpr int64_t FMAP_MAXGRID = 1 << 20;   // workgroups; the row loop strides beyond that

// exp(-2 pi i f tau), or its conjugate
template <bool CONJ>
__device__ __forceinline__ float2 seg_phase(float f, double tau) {
    double p = (double)f * tau;
    p -= rint(p);                                                           // whole cycles drop out exactly
    float s, c;
    sincospif(2.f * (float)p, &s, &c);
    return make_float2(c, CONJ ? s : -s);
}

// nv work items of V voxels each (n = nv * V)
template <int V, bool BETA>
__global__ void __launch_bounds__(FMAP_BLK)
k_fmap_phase_fwd(int64_t nv, int L, const float* __restrict__ f, double tau0, double dtau, const float2* __restrict__ x,
                 float2 a, float2 b, float2* __restrict__ y, int64_t ldy) {
    for (int64_t w = (int64_t)blockIdx.x * FMAP_BLK + threadIdx.x; w < nv; w += (int64_t)gridDim.x * FMAP_BLK) {
        const int64_t i = w * V;
        float fr[V];
        float2 xr[V];
        ldv<V>(xr, x + i);
#pragma unroll
        for (int v = 0; v < V; ++v) { fr[v] = f[i + v]; xr[v] = cmul(a, xr[v]); }
        float2* yp = y + i;
#pragma unroll 2
        for (int l = 0; l < L; ++l, yp += ldy) {
            const double tau = tau0 + (double)l * dtau;
            float2 r[V];
#pragma unroll
            for (int v = 0; v < V; ++v) r[v] = cmul(seg_phase<false>(fr[v], tau), xr[v]);
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

template <int V, bool BETA>
__global__ void __launch_bounds__(FMAP_BLK)
k_fmap_phase_adj(int64_t nv, int L, const float* __restrict__ f, double tau0, double dtau, const float2* __restrict__ x, int64_t ldx,
                 float2 a, float2 b, float2* __restrict__ y) {
    for (int64_t w = (int64_t)blockIdx.x * FMAP_BLK + threadIdx.x; w < nv; w += (int64_t)gridDim.x * FMAP_BLK) {
        const int64_t i = w * V;
        float fr[V];
        float2 acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) { fr[v] = f[i + v]; acc[v] = make_float2(0.f, 0.f); }
        const float2* xp = x + i;
#pragma unroll 4
        for (int l = 0; l < L; ++l, xp += ldx) {
            const double tau = tau0 + (double)l * dtau;
            float2 xv[V];
            ldv<V>(xv, xp);
#pragma unroll
            for (int v = 0; v < V; ++v) cfma(acc[v], seg_phase<true>(fr[v], tau), xv[v]);
        }
        float2 r[V];
#pragma unroll
        for (int v = 0; v < V; ++v) r[v] = cmul(a, acc[v]);
        if (BETA) {
            float2 o[V];
            ldv<V>(o, y + i);
#pragma unroll
            for (int v = 0; v < V; ++v) cfma(r[v], b, o[v]);
        }
        stv<V>(y + i, r);
    }
}

// rows of the table for the V rows from r on: r mod P and its successors (32-bit arithmetic when the row count allows)
template <int V>
__device__ __forceinline__ void table_rows(int64_t (&rp)[V], int64_t r, int64_t P, bool small) {
    rp[0] = small ? (int64_t)((uint32_t)r % (uint32_t)P) : r % P;
#pragma unroll
    for (int v = 1; v < V; ++v) rp[v] = rp[v - 1] + 1 == P ? 0 : rp[v - 1] + 1;
}

template <int V, bool BETA>
__global__ void __launch_bounds__(FMAP_BLK)
k_fmap_combine_fwd(int64_t nv, int L, int64_t P, bool small, const float2* __restrict__ tab, int64_t ldb, const float2* __restrict__ x, int64_t ldx,
                   float2 a, float2 b, float2* __restrict__ y) {
    for (int64_t w = (int64_t)blockIdx.x * FMAP_BLK + threadIdx.x; w < nv; w += (int64_t)gridDim.x * FMAP_BLK) {
        const int64_t i = w * V;
        int64_t rp[V];
        table_rows<V>(rp, i, P, small);
        float2 acc[V];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = make_float2(0.f, 0.f);
        const float2* xp = x + i;
        const float2* tp = tab;
#pragma unroll 4
        for (int l = 0; l < L; ++l, xp += ldx, tp += ldb) {
            float2 xv[V];
            ldv<V>(xv, xp);
#pragma unroll
            for (int v = 0; v < V; ++v) cfma(acc[v], tp[rp[v]], xv[v]);
        }
        float2 r[V];
#pragma unroll
        for (int v = 0; v < V; ++v) r[v] = cmul(a, acc[v]);
        if (BETA) {
            float2 o[V];
            ldv<V>(o, y + i);
#pragma unroll
            for (int v = 0; v < V; ++v) cfma(r[v], b, o[v]);
        }
        stv<V>(y + i, r);
    }
}

template <int V, bool BETA>
__global__ void __launch_bounds__(FMAP_BLK)
k_fmap_combine_adj(int64_t nv, int L, int64_t P, bool small, const float2* __restrict__ tab, int64_t ldb, const float2* __restrict__ x,
                   float2 a, float2 b, float2* __restrict__ y, int64_t ldy) {
    for (int64_t w = (int64_t)blockIdx.x * FMAP_BLK + threadIdx.x; w < nv; w += (int64_t)gridDim.x * FMAP_BLK) {
        const int64_t i = w * V;
        int64_t rp[V];
        table_rows<V>(rp, i, P, small);
        float2 xr[V];
        ldv<V>(xr, x + i);
#pragma unroll
        for (int v = 0; v < V; ++v) xr[v] = cmul(a, xr[v]);
        float2* yp = y + i;
        const float2* tp = tab;
#pragma unroll 4
        for (int l = 0; l < L; ++l, yp += ldy, tp += ldb) {
            float2 r[V];
#pragma unroll
            for (int v = 0; v < V; ++v) r[v] = cmulc(tp[rp[v]], xr[v]);
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

// the checks that both entries share; cols_x / cols_y: 1 and L, or L and 1
int fmap_check(ig_ctx* ctx, const char* who, int64_t n, int64_t L, const void* x, int64_t ldx, const void* y, int64_t ldy) {
    if (L < 1 || L > FMAP_MAXL)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "%s: %lld segments, between 1 and %d are supported", who, (long long)L, FMAP_MAXL);
    if (n < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "%s: %lld rows, at least 1 is supported", who, (long long)n);
    IG_REQUIRE(ctx, ldx >= n && ldy >= n, "%s: leading dimension (%lld, %lld) below n = %lld", who, (long long)ldx, (long long)ldy, (long long)n);
    IG_REQUIRE(ctx, x && y, "%s: NULL pointer", who);
    return IG_OK;
}

// pairs of rows: every column of both panels then starts on a 16-byte boundary and holds whole pairs
bool fmap_wide(int64_t n, const void* x, int64_t ldx, const void* y, int64_t ldy) {
    return n % 2 == 0 && ldx % 2 == 0 && ldy % 2 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0;
}

}  // namespace

int ig_fmap_phase_c64(ig_ctx* ctx, int64_t n, int64_t L, const float* f, double tau0, double dtau, int adjoint,
                      const void* x, int64_t ldx, float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_fmap_phase_c64: ctx is NULL");
    if (int rc = fmap_check(ctx, "ig_fmap_phase_c64", n, L, x, ldx, y, ldy)) return rc;
    IG_REQUIRE(ctx, f != nullptr, "ig_fmap_phase_c64: NULL pointer");
    const int64_t cols_x = adjoint ? L : 1, cols_y = adjoint ? 1 : L;
    IG_REQUIRE(ctx, !ig_panels_overlap(x, ldx, n, cols_x, y, ldy, n, cols_y), "ig_fmap_phase_c64: y overlaps x");
    const uintptr_t y0 = (uintptr_t)y, f0 = (uintptr_t)f;
    IG_REQUIRE(ctx, !ig_bytes_overlap(f0, f0 + (uintptr_t)n * sizeof(float), y0, y0 + (uintptr_t)((cols_y - 1) * ldy + n) * sizeof(float2)),
               "ig_fmap_phase_c64: y overlaps f");
    if (int rc = ig_set_device(ctx)) return rc;
    const bool beta = !(br == 0.f && bi == 0.f);
    const float2 a = make_float2(ar, ai), b = make_float2(br, bi);
    const bool wide = fmap_wide(n, x, ldx, y, ldy);
    ig_prof_scope prof(ctx, adjoint ? "fmap_phase_adj" : "fmap_phase_fwd", 8.0 * (double)n * (double)(L + 1 + (beta ? cols_y : 0)) + 4.0 * (double)n);
    const int V = wide ? 2 : 1;
    const dim3 grid = ig_grid_1d(n / V, FMAP_BLK, FMAP_MAXGRID), block(FMAP_BLK);
#define IG_PHASE_FWD(V, BETA) hipLaunchKernelGGL((k_fmap_phase_fwd<V, BETA>), grid, block, 0, ctx->stream, n / V, (int)L, f, tau0, dtau, (const float2*)x, a, b, (float2*)y, ldy)
#define IG_PHASE_ADJ(V, BETA) hipLaunchKernelGGL((k_fmap_phase_adj<V, BETA>), grid, block, 0, ctx->stream, n / V, (int)L, f, tau0, dtau, (const float2*)x, ldx, a, b, (float2*)y)
    if (adjoint) {
        if (wide) { if (beta) IG_PHASE_ADJ(2, true); else IG_PHASE_ADJ(2, false); }
        else      { if (beta) IG_PHASE_ADJ(1, true); else IG_PHASE_ADJ(1, false); }
    } else {
        if (wide) { if (beta) IG_PHASE_FWD(2, true); else IG_PHASE_FWD(2, false); }
        else      { if (beta) IG_PHASE_FWD(1, true); else IG_PHASE_FWD(1, false); }
    }
#undef IG_PHASE_FWD
#undef IG_PHASE_ADJ
    IG_LAUNCH_CHECK(ctx, adjoint ? "k_fmap_phase_adj" : "k_fmap_phase_fwd");
    return IG_OK;
}

int ig_fmap_combine_c64(ig_ctx* ctx, int64_t n, int64_t L, int64_t P, const void* b, int64_t ldb, int adjoint,
                        const void* x, int64_t ldx, float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_fmap_combine_c64: ctx is NULL");
    if (int rc = fmap_check(ctx, "ig_fmap_combine_c64", n, L, x, ldx, y, ldy)) return rc;
    IG_REQUIRE(ctx, b != nullptr, "ig_fmap_combine_c64: NULL pointer");
    IG_REQUIRE(ctx, P >= 1 && n % P == 0, "ig_fmap_combine_c64: %lld rows are no multiple of the table's period %lld", (long long)n, (long long)P);
    IG_REQUIRE(ctx, ldb >= P, "ig_fmap_combine_c64: leading dimension %lld of b below P = %lld", (long long)ldb, (long long)P);
    const int64_t cols_x = adjoint ? 1 : L, cols_y = adjoint ? L : 1;
    IG_REQUIRE(ctx, !ig_panels_overlap(x, ldx, n, cols_x, y, ldy, n, cols_y), "ig_fmap_combine_c64: y overlaps x");
    IG_REQUIRE(ctx, !ig_panels_overlap(b, ldb, P, L, y, ldy, n, cols_y), "ig_fmap_combine_c64: y overlaps b");
    if (int rc = ig_set_device(ctx)) return rc;
    const bool beta = !(br == 0.f && bi == 0.f);
    const float2 a = make_float2(ar, ai), bb = make_float2(br, bi);
    const bool wide = fmap_wide(n, x, ldx, y, ldy), small = n <= (int64_t)UINT32_MAX;
    ig_prof_scope prof(ctx, adjoint ? "fmap_combine_adj" : "fmap_combine_fwd", 8.0 * (double)n * (double)(L + 1 + (beta ? cols_y : 0)) + 8.0 * (double)P * (double)L);
    const int V = wide ? 2 : 1;
    const dim3 grid = ig_grid_1d(n / V, FMAP_BLK, FMAP_MAXGRID), block(FMAP_BLK);
#define IG_COMBINE_FWD(V, BETA) hipLaunchKernelGGL((k_fmap_combine_fwd<V, BETA>), grid, block, 0, ctx->stream, n / V, (int)L, P, small, (const float2*)b, ldb, (const float2*)x, ldx, a, bb, (float2*)y)
#define IG_COMBINE_ADJ(V, BETA) hipLaunchKernelGGL((k_fmap_combine_adj<V, BETA>), grid, block, 0, ctx->stream, n / V, (int)L, P, small, (const float2*)b, ldb, (const float2*)x, a, bb, (float2*)y, ldy)
    if (adjoint) {
        if (wide) { if (beta) IG_COMBINE_ADJ(2, true); else IG_COMBINE_ADJ(2, false); }
        else      { if (beta) IG_COMBINE_ADJ(1, true); else IG_COMBINE_ADJ(1, false); }
    } else {
        if (wide) { if (beta) IG_COMBINE_FWD(2, true); else IG_COMBINE_FWD(2, false); }
        else      { if (beta) IG_COMBINE_FWD(1, true); else IG_COMBINE_FWD(1, false); }
    }
#undef IG_COMBINE_FWD
#undef IG_COMBINE_ADJ
    IG_LAUNCH_CHECK(ctx, adjoint ? "k_fmap_combine_adj" : "k_fmap_combine_fwd");
    return IG_OK;
}
