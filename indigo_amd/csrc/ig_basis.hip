// The temporal-subspace operator Phi (x) I_n and its adjoint on frame panels (Backend.frame_basis, operators.FrameBasis,
// pics --basis).
//
// phi is the nt x nk basis (column-major, ldphi >= nt), x and y are column-major panels of n-voxel images:
//   forward : y[i, t] = beta*y[i, t] + alpha * sum_k      phi[t, k]  * x[i, k]      x: n x nk coefficient images, y: n x nt frames
//   adjoint : y[i, k] = beta*y[i, k] + alpha * sum_t conj(phi[t, k]) * x[i, t]      x: n x nt frames, y: n x nk coefficient images
//
// Both are single-pass streams: 8 n (nk + nt) bytes, and 8 n (rows of y) more when beta != 0.  One thread per voxel, or per
// pair of neighbouring voxels with 16-byte accesses when n, the leading dimensions and the pointers allow; the voxel's nk
// values (forward, alpha already applied) or nk accumulators (adjoint) stay in registers, so nk has a compile-time bound NK:
// the kernels exist for NK = 4, 8, 16 and 32 and mask the tail (the image of a k >= nk is zero and never loaded or stored).
// The loop over t reads or writes one fully coalesced column element per lane.  Row t of phi is the same for every lane: the
// workgroup copies phi once into LDS, transposed (row t contiguous, the tail k >= nk zero) -- BASIS_LDS bytes of it at a time
// when nt is large -- and every lane reads row t from the same LDS address (a broadcast, 16 bytes = two coefficients per
// read): phi costs no vector memory traffic per voxel.  No atomics, no second pass over y.  All element offsets are 64-bit.
#include "ig_common.h"

namespace {

constexpr int BASIS_MAXK = 32;         // coefficient images
constexpr int BASIS_BLK = 256;
constexpr int BASIS_LDS = 8192;          // bytes of phi in LDS at a time: 256 rows at NK = 4, 32 rows at NK = 32
constexpr int64_t BASIS_MAXGRID = 1 << 20;   // workgroups; the voxel loop strides beyond that

// rows [t0, t0 + tt) of phi into LDS as ph[t][k], zero for the masked tail k >= nk; the caller puts barriers around it
template <int NK>
__device__ __forceinline__ void stage_phi(float2 (*ph)[NK], const float2* __restrict__ phi, int64_t ldphi, int64_t t0, int tt, int nk) {
    for (int e = threadIdx.x; e < tt * NK; e += BASIS_BLK) {
        const int k = e / tt, t = e - k * tt;                               // consecutive threads read consecutive t of a column
        ph[t][k] = k < nk ? phi[t0 + t + (int64_t)k * ldphi] : make_float2(0.f, 0.f);
    }
}

// nv work items of V voxels each (n = nv * V).  The loops over the workgroup's chunks of voxels and over the staged rows of phi
// have the same trip counts in every thread (barriers inside); a thread past the end takes part in the staging only.
template <int NK, int V, bool BETA>
__global__ void __launch_bounds__(BASIS_BLK)
k_basis_fwd(int64_t nv, int nk, int64_t nt, const float2* __restrict__ phi, int64_t ldphi, const float2* __restrict__ x, int64_t ldx,
            float2 a, float2 b, float2* __restrict__ y, int64_t ldy) {
    constexpr int TT = BASIS_LDS / (NK * 8);
    constexpr int UT = NK <= 8 ? 2 : 1;                                     // rows of phi in registers at a time: 2 NK VGPRs each
    __shared__ __align__(16) float2 ph[TT][NK];
    for (int64_t base = (int64_t)blockIdx.x * BASIS_BLK; base < nv; base += (int64_t)gridDim.x * BASIS_BLK) {
        const bool active = base + threadIdx.x < nv;
        const int64_t i = (base + threadIdx.x) * V;
        float2 xr[NK][V];
        const float2* xp = x + i;
#pragma unroll
        for (int k = 0; k < NK; ++k, xp += ldx) {
            if (active && k < nk) {
                ldv<V>(xr[k], xp);
#pragma unroll
                for (int v = 0; v < V; ++v) xr[k][v] = cmul(a, xr[k][v]);
            } else {
#pragma unroll
                for (int v = 0; v < V; ++v) xr[k][v] = make_float2(0.f, 0.f);
            }
        }
        for (int64_t t0 = 0; t0 < nt; t0 += TT) {
            const int tt = (int)(nt - t0 < TT ? nt - t0 : TT);
            __syncthreads();                                                // the previous rows have been used
            stage_phi<NK>(ph, phi, ldphi, t0, tt, nk);
            __syncthreads();
            if (!active) continue;
            float2* yp = y + i + t0 * ldy;
#pragma unroll UT
            for (int t = 0; t < tt; ++t, yp += ldy) {
                float2 acc[V];
#pragma unroll
                for (int v = 0; v < V; ++v) acc[v] = make_float2(0.f, 0.f);
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const float2 p = ph[t][k];
#pragma unroll
                    for (int v = 0; v < V; ++v) cfma(acc[v], xr[k][v], p);
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
}

template <int NK, int V, bool BETA>
__global__ void __launch_bounds__(BASIS_BLK)
k_basis_adj(int64_t nv, int nk, int64_t nt, const float2* __restrict__ phi, int64_t ldphi, const float2* __restrict__ x, int64_t ldx,
            float2 a, float2 b, float2* __restrict__ y, int64_t ldy) {
    constexpr int TT = BASIS_LDS / (NK * 8);
    constexpr int UT = NK <= 8 ? 4 : NK <= 16 ? 2 : 1;                      // loads of x in flight, and rows of phi in registers
    __shared__ __align__(16) float2 ph[TT][NK];
    for (int64_t base = (int64_t)blockIdx.x * BASIS_BLK; base < nv; base += (int64_t)gridDim.x * BASIS_BLK) {
        const bool active = base + threadIdx.x < nv;
        const int64_t i = (base + threadIdx.x) * V;
        float2 acc[NK][V];
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int v = 0; v < V; ++v) acc[k][v] = make_float2(0.f, 0.f);
        for (int64_t t0 = 0; t0 < nt; t0 += TT) {
            const int tt = (int)(nt - t0 < TT ? nt - t0 : TT);
            __syncthreads();                                                // the previous rows have been used
            stage_phi<NK>(ph, phi, ldphi, t0, tt, nk);
            __syncthreads();
            if (!active) continue;
            const float2* xp = x + i + t0 * ldx;
#pragma unroll UT
            for (int t = 0; t < tt; ++t, xp += ldx) {
                float2 xv[V];
                ldv<V>(xv, xp);
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const float2 p = ph[t][k];
#pragma unroll
                    for (int v = 0; v < V; ++v) cfmac(acc[k][v], p, xv[v]);
                }
            }
        }
        if (!active) continue;
        float2* yp = y + i;
#pragma unroll
        for (int k = 0; k < NK; ++k, yp += ldy) {
            if (k < nk) {
                float2 r[V];
#pragma unroll
                for (int v = 0; v < V; ++v) r[v] = cmul(a, acc[k][v]);
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
}

template <int NK, int V>
void basis_launch(ig_ctx* ctx, bool adjoint, bool beta, int64_t n, int nk, int64_t nt, const float2* phi, int64_t ldphi,
                  const float2* x, int64_t ldx, float2 a, float2 b, float2* y, int64_t ldy) {
    const int64_t nv = n / V;
    const dim3 grid = ig_grid_1d(nv, BASIS_BLK, BASIS_MAXGRID), block(BASIS_BLK);
#define IG_BASIS_GO(KERNEL, BETA) hipLaunchKernelGGL((KERNEL<NK, V, BETA>), grid, block, 0, ctx->stream, nv, nk, nt, phi, ldphi, x, ldx, a, b, y, ldy)
    if (adjoint) { if (beta) IG_BASIS_GO(k_basis_adj, true); else IG_BASIS_GO(k_basis_adj, false); }
    else         { if (beta) IG_BASIS_GO(k_basis_fwd, true); else IG_BASIS_GO(k_basis_fwd, false); }
#undef IG_BASIS_GO
}

}  // namespace

int ig_basis_c64(ig_ctx* ctx, int64_t n, int64_t nk, int64_t nt, const void* phi, int64_t ldphi, int adjoint,
                 const void* x, int64_t ldx, float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_basis_c64: ctx is NULL");
    if (nk < 1 || nk > BASIS_MAXK)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_basis_c64: %lld coefficients, between 1 and %d are supported", (long long)nk, BASIS_MAXK);
    if (nt < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_basis_c64: %lld frames, at least 1 is supported", (long long)nt);
    if (n < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_basis_c64: %lld voxels, at least 1 is supported", (long long)n);
    IG_REQUIRE(ctx, ldphi >= nt, "ig_basis_c64: leading dimension %lld of phi below nt = %lld", (long long)ldphi, (long long)nt);
    IG_REQUIRE(ctx, ldx >= n && ldy >= n, "ig_basis_c64: leading dimension (%lld, %lld) below n = %lld", (long long)ldx, (long long)ldy, (long long)n);
    IG_REQUIRE(ctx, phi && x && y, "ig_basis_c64: NULL pointer");
    const int64_t cols_x = adjoint ? nt : nk, cols_y = adjoint ? nk : nt;
    IG_REQUIRE(ctx, !ig_panels_overlap(x, ldx, n, cols_x, y, ldy, n, cols_y), "ig_basis_c64: y overlaps x");
    IG_REQUIRE(ctx, !ig_panels_overlap(phi, ldphi, nt, nk, y, ldy, n, cols_y), "ig_basis_c64: y overlaps phi");
    if (int rc = ig_set_device(ctx)) return rc;
    const bool beta = !(br == 0.f && bi == 0.f);
    const float2 a = make_float2(ar, ai), b = make_float2(br, bi);
    // pairs of voxels: every column of both panels then starts on a 16-byte boundary and holds whole pairs
    const bool wide = n % 2 == 0 && ldx % 2 == 0 && ldy % 2 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0;
    ig_prof_scope prof(ctx, adjoint ? "basis_adj" : "basis_fwd", 8.0 * (double)n * (double)(nk + nt + (beta ? cols_y : 0)));
#define IG_BASIS_CASE(NK, V) basis_launch<NK, V>(ctx, adjoint != 0, beta, n, (int)nk, nt, (const float2*)phi, ldphi, (const float2*)x, ldx, a, b, (float2*)y, ldy)
    if (nk <= 4)       { if (wide) IG_BASIS_CASE(4, 2);  else IG_BASIS_CASE(4, 1); }
    else if (nk <= 8)  { if (wide) IG_BASIS_CASE(8, 2);  else IG_BASIS_CASE(8, 1); }
    else if (nk <= 16) IG_BASIS_CASE(16, 1);      // (pairs would take 64 and 128 registers for the images alone)
    else               IG_BASIS_CASE(32, 1);
#undef IG_BASIS_CASE
    IG_LAUNCH_CHECK(ctx, adjoint ? "k_basis_adj" : "k_basis_fwd");
    return IG_OK;
}
