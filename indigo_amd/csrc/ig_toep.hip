// The K x K point-spread mixing pass of the Toeplitz normal operator (Backend.psf_mix, operators.ToeplitzNormal,
// pics --toeplitz).
//
//   y[g, c, k] = sum_k' P[g][k, k'] * x[g, c, k']        g < n grid points, c < nc coils, k < nk
//
// x and y are panels of nk columns (ldx, ldy in elements); inside a column element (g, c) sits at g*sg + c*sc: coil-major
// grids (sg = 1, sc >= n) or coil-interleaved ones (sc = 1, sg >= nc).  P is Hermitian at every grid point and arrives as nk^2
// planes of n floats: the nk real diagonals, then re and im of every pair (k < k'), pairs in row-major order of the upper triangle;
// the lower triangle is the conjugate.  One thread per grid point (two neighbouring points with 16-byte accesses on coil-major
// grids up to NK = 4; one point and two neighbouring coils per 16-byte access on coil-interleaved grids): the point's nk^2 floats
// go to registers once and serve every coil, so nk has a compile-time bound NK in {1, 2, 4, 8} with a masked tail (a k >= nk is
// never loaded or stored, its entries of P are zero registers).  The loop over the coils loads the next coil's nk values before
// it stores the current one's (up to NK = 4); y may be x: a thread reads and writes its own elements only.  A single pass:
// 16 n nc nk + 4 nk^2 n bytes.  All element offsets are 64-bit.
#include "ig_common.h"

namespace {

constexpr int TOEP_MAXK = 8;
constexpr int TOEP_BLK = 256;
constexpr int64_t TOEP_MAXGRID = 0x7fffffff;   // workgroups of one launch

// GV grid points per thread (neighbours in memory: sg == 1), CV coils per access (neighbours in memory: sc == 1); one of the two
// is 1.  Coil-major: one work item per GV grid points (cpg = 1), which loops over the nloop = nc coils.  Coil-interleaved: a
// grid point's coils lie side by side, so its cpg = nc / CV groups of coils are cpg neighbouring work items that read the same
// entries of P (one address per cpg lanes) and nloop = 1: the wave's accesses to x and y are contiguous.  nitems work items.
// x and y may be the same panel: no __restrict__ on them.
template <int NK, int GV, int CV>
__global__ void __launch_bounds__(TOEP_BLK)
k_psf_mix(int64_t nitems, int64_t n, int64_t cpg, int64_t nloop, int nk, const float* __restrict__ kern, const float2* x, int64_t ldx,
          float2* y, int64_t ldy, int64_t sg, int64_t sc) {
    constexpr int V = GV * CV;
    constexpr int NP = NK * (NK - 1) / 2;
    constexpr bool PRE = NK <= 4;          // the next coil's values are loaded before this coil's are stored; NK = 8 has no registers for that
    const int64_t it = (int64_t)blockIdx.x * TOEP_BLK + threadIdx.x;
    if (it < nitems) {
        const int64_t pt = cpg > 1 ? it / cpg : it;
        const int64_t g = pt * GV, c0 = (it - pt * cpg) * CV;
        // the point's Hermitian matrix: NK real diagonals and NP complex entries above them, per grid point of the thread
        float pd[NK][GV];
        float2 po[NP > 0 ? NP : 1][GV];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            if (k < nk) {
                const float* p = kern + (int64_t)k * n + g;
                if constexpr (GV == 2) { const float2 q = *reinterpret_cast<const float2*>(p); pd[k][0] = q.x; pd[k][1] = q.y; }
                else pd[k][0] = *p;
            } else {
#pragma unroll
                for (int v = 0; v < GV; ++v) pd[k][v] = 0.f;
            }
        }
#pragma unroll
        for (int a = 0, q = 0; a < NK; ++a) {
#pragma unroll
            for (int b = a + 1; b < NK; ++b, ++q) {
                if (b < nk) {
                    const int pair = a * nk - a * (a + 1) / 2 + (b - a - 1);          // its number among the pairs of an nk x nk matrix
                    const float* pr = kern + (int64_t)(nk + 2 * pair) * n + g;
                    if constexpr (GV == 2) {
                        const float2 re = *reinterpret_cast<const float2*>(pr), im = *reinterpret_cast<const float2*>(pr + n);
                        po[q][0] = make_float2(re.x, im.x); po[q][1] = make_float2(re.y, im.y);
                    } else {
                        po[q][0] = make_float2(pr[0], pr[n]);
                    }
                } else {
#pragma unroll
                    for (int v = 0; v < GV; ++v) po[q][v] = make_float2(0.f, 0.f);
                }
            }
        }
        const float2* xp = x + g * sg + c0 * sc;
        float2* yp = y + g * sg + c0 * sc;
        const int64_t cstep = sc;
        float2 cur[NK][V];
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (k < nk) ldv<V>(cur[k], xp + (int64_t)k * ldx);
        for (int64_t c = 0; c < nloop; ++c, xp += cstep, yp += cstep) {
            float2 nxt[PRE ? NK : 1][V];
            if (PRE && c + 1 < nloop) {
#pragma unroll
                for (int k = 0; k < NK; ++k)
                    if (k < nk) ldv<V>(nxt[PRE ? k : 0], xp + cstep + (int64_t)k * ldx);
            }
            float2 acc[NK][V];
#pragma unroll
            for (int k = 0; k < NK; ++k)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const float d = pd[k][GV == 2 ? v : 0];
                    acc[k][v] = k < nk ? make_float2(d * cur[k][v].x, d * cur[k][v].y) : make_float2(0.f, 0.f);
                }
#pragma unroll
            for (int a = 0, q = 0; a < NK; ++a) {
#pragma unroll
                for (int b = a + 1; b < NK; ++b, ++q) {
                    if (b < nk) {
#pragma unroll
                        for (int v = 0; v < V; ++v) {
                            const float2 p = po[q][GV == 2 ? v : 0];
                            cfma(acc[a][v], p, cur[b][v]);                           // P[a, b] x[b]
                            const float2 r = cmulc(p, cur[a][v]);                    // P[b, a] x[a] = conj(P[a, b]) x[a]
                            acc[b][v].x += r.x; acc[b][v].y += r.y;
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < NK; ++k)
                if (k < nk) stv<V>(yp + (int64_t)k * ldy, acc[k]);
            if (c + 1 < nloop) {
#pragma unroll
                for (int k = 0; k < NK; ++k)
                    if (k < nk) {
                        if constexpr (PRE) {
#pragma unroll
                            for (int v = 0; v < V; ++v) cur[k][v] = nxt[k][v];
                        } else {
                            ldv<V>(cur[k], xp + cstep + (int64_t)k * ldx);            // (after this coil's stores: y may be x)
                        }
                    }
            }
        }
    }
}

template <int NK, int GV, int CV>
void toep_launch(ig_ctx* ctx, int64_t n, int64_t nc, int nk, const float* kern, const float2* x, int64_t ldx, float2* y, int64_t ldy,
                 int64_t sg, int64_t sc) {
    const int64_t cpg = sc == 1 ? nc / CV : 1, nloop = sc == 1 ? 1 : nc;
    const int64_t nitems = n / GV * cpg, blocks = (nitems + TOEP_BLK - 1) / TOEP_BLK;
    hipLaunchKernelGGL((k_psf_mix<NK, GV, CV>), dim3((unsigned)blocks), dim3(TOEP_BLK), 0, ctx->stream, nitems, n, cpg, nloop, nk, kern, x, ldx, y, ldy, sg, sc);
}

}  // namespace

int ig_psf_mix_c64(ig_ctx* ctx, int64_t n, int64_t nc, int64_t nk, const float* kern, const void* x, int64_t ldx,
                   void* y, int64_t ldy, int64_t sg, int64_t sc) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_psf_mix_c64: ctx is NULL");
    if (nk < 1 || nk > TOEP_MAXK)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_psf_mix_c64: %lld coefficients, between 1 and %d are supported (the kernel array holds "
                       "4 nk^2 bytes per grid point)", (long long)nk, TOEP_MAXK);
    if (n < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_psf_mix_c64: %lld grid points, at least 1 is supported", (long long)n);
    if (nc < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_psf_mix_c64: %lld coils, at least 1 is supported", (long long)nc);
    IG_REQUIRE(ctx, kern && x && y, "ig_psf_mix_c64: NULL pointer");
    IG_REQUIRE(ctx, (sg == 1 && sc >= n) || (sc == 1 && sg >= nc),
               "ig_psf_mix_c64: strides (%lld, %lld): coil-major (sg = 1, sc >= n) or coil-interleaved (sc = 1, sg >= nc) grids",
               (long long)sg, (long long)sc);
    const int64_t ext = (n - 1) * sg + (nc - 1) * sc + 1;                           // elements of one column
    IG_REQUIRE(ctx, ldx >= ext && ldy >= ext, "ig_psf_mix_c64: leading dimension (%lld, %lld) below the %lld elements of a column",
               (long long)ldx, (long long)ldy, (long long)ext);
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (uintptr_t)((nk - 1) * ldx + ext) * sizeof(float2);
    const uintptr_t y0 = (uintptr_t)y, y1 = y0 + (uintptr_t)((nk - 1) * ldy + ext) * sizeof(float2);
    const uintptr_t k0 = (uintptr_t)kern, k1 = k0 + (uintptr_t)(nk * nk * n) * sizeof(float);
    IG_REQUIRE(ctx, (x == y && ldx == ldy) || !ig_bytes_overlap(x0, x1, y0, y1), "ig_psf_mix_c64: y overlaps x (y == x with ldy == ldx is the in-place form)");
    IG_REQUIRE(ctx, !ig_bytes_overlap(k0, k1, y0, y1), "ig_psf_mix_c64: y overlaps the kernel array");
    if ((n * nc + TOEP_BLK - 1) / TOEP_BLK > TOEP_MAXGRID)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_psf_mix_c64: %lld x %lld elements per column exceed one launch", (long long)n, (long long)nc);
    if (int rc = ig_set_device(ctx)) return rc;
    const float2* xp = (const float2*)x;
    float2* yp = (float2*)y;
    const bool al16 = x0 % 16 == 0 && y0 % 16 == 0 && ldx % 2 == 0 && ldy % 2 == 0;
    // pairs of grid points (coil-major): every column and every coil's grid starts on a 16-byte boundary and holds whole pairs,
    // and so does every plane of the kernel array (8-byte accesses there)
    const bool gwide = sg == 1 && al16 && n % 2 == 0 && sc % 2 == 0 && k0 % 8 == 0 && nk <= 4;
    // pairs of coils (coil-interleaved): every grid point's coils start on a 16-byte boundary and hold whole pairs
    const bool cwide = sc == 1 && al16 && nc % 2 == 0 && sg % 2 == 0;
    ig_prof_scope prof(ctx, "psf_mix", 16.0 * (double)n * (double)nc * (double)nk + 4.0 * (double)(nk * nk) * (double)n);
    const int ik = (int)nk;
#define IG_TOEP_CASE(NK)                                                                                  \
    do {                                                                                                  \
        if (cwide) toep_launch<NK, 1, 2>(ctx, n, nc, ik, kern, xp, ldx, yp, ldy, sg, sc);                  \
        else toep_launch<NK, 1, 1>(ctx, n, nc, ik, kern, xp, ldx, yp, ldy, sg, sc);                        \
    } while (0)
#define IG_TOEP_CASE_G(NK)                                                                                \
    do {                                                                                                  \
        if (gwide) toep_launch<NK, 2, 1>(ctx, n, nc, ik, kern, xp, ldx, yp, ldy, sg, sc);                  \
        else IG_TOEP_CASE(NK);                                                                            \
    } while (0)
    if (nk == 1)      IG_TOEP_CASE_G(1);
    else if (nk == 2) IG_TOEP_CASE_G(2);
    else if (nk <= 4) IG_TOEP_CASE_G(4);
    else              IG_TOEP_CASE(8);
#undef IG_TOEP_CASE_G
#undef IG_TOEP_CASE
    IG_LAUNCH_CHECK(ctx, "k_psf_mix");
    return IG_OK;
}
