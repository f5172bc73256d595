// ESPIRiT calibration at image resolution (indigo_amd.ecalib, Backend.place_wrapped, Backend.espirit_eig).
//
// ig_place_wrapped_c64: ncols small boxes (the correlation boxes R_cc'[delta] of the calibration's projector) into ncols zeroed
// volumes, each box with its centre element at index 0 and its negative half wrapped to the top of every axis: the input of the
// unnormalised inverse transforms that evaluate G(x).  One thread per volume element, every element written once (the box value
// or zero), 8 N ncols bytes.
//
// ig_espirit_eig_c64: the nm leading eigenpairs of the Hermitian nc x nc matrix G at every voxel, from the panel of the row-wise
// upper triangle of G, with the map conventions of ESPIRiT: descending eigenvalues, unit vectors, coil 0 real and >= 0, exact zeros
// where the eigenvalue is below `crop`.  Two kernels; in both neighbouring lanes work on neighbouring voxels, so every column of the
// three panels is read and written in contiguous runs, and everything between the loads and the stores is float32 in registers.
//
//   nc <= 8   k_esp_jacobi<NC>: one lane per voxel, cyclic Jacobi on the whole matrix.  The strict upper triangle, the real
//             diagonal and the nc x nc rotation product stay in registers: every loop over rows, columns and pairs is unrolled over
//             the compile-time NC, so no register array is indexed dynamically.  A rotation is skipped where
//             |a_pq|^2 <= (4 eps)^2 |a_pp a_qq|, and the sweeps end when no lane of the wave rotated (or after `iters` sweeps): about
//             seven sweeps at nc = 8.  Jacobi does not depend on the gaps between the eigenvalues: a voxel whose two leading
//             eigenvalues nearly coincide still gets both to float32 accuracy, where 30 power iterations leave an error of up to
//             0.6 % in the leading one.  The nm leading pairs are picked afterwards by unrolled compare-and-select chains.
//   nc <= 32  k_esp_orth<R, L, NM>: orthogonal iteration (what bart ecalib runs), `iters` rounds of V <- orth(G V) by modified
//             Gram-Schmidt, eigenvalue m = the norm of column m after the projections.  L lanes share a voxel, each with R rows of G
//             (zero rows beyond nc) and of V: (R, L) = (4, 4) up to 16 coils, (2, 16) up to 32.  A wave holds 64 / L neighbouring
//             voxels, lane = voxel + (64 / L) * member, so the lanes of one member read and write runs of 64 / L voxels.  The product
//             takes the rows of V from the other members by __shfl, the inner products are xor butterflies over the members
//             (every member ends with the same bits).  Its accuracy depends on the gaps: the error of pair m after k rounds is of
//             the order (lambda_{nm+1} / lambda_m)^k.
#include "ig_common.h"

namespace {

constexpr int ESP_MAXM = 4;
constexpr int ESP_MAXC = 32;
constexpr int ESP_JBLK = 64;                    // k_esp_jacobi: one wave per workgroup (about 250 registers per lane at NC = 8)
constexpr int ESP_OBLK = 256;
constexpr int64_t ESP_MAXGRID = 1 << 20;        // workgroups; the voxel loops stride beyond that
constexpr float ESP_ROT2 = 5.7e-14f;            // (4 eps)^2: a rotation below it changes nothing that float32 resolves
constexpr float ESP_MINPHASE = 1e-6f;           // a vector whose coil-0 magnitude is below this is left unrotated

__device__ __forceinline__ float2 cconj(float2 a) { return make_float2(a.x, -a.y); }
__device__ __forceinline__ float2 cscale(float s, float2 a) { return make_float2(s * a.x, s * a.y); }

// ---- place_wrapped ------------------------------------------------------------------------------------------------------------
// index of volume coordinate i inside a box of b elements whose element cb = b / 2 sits at 0, or -1
__device__ __forceinline__ int64_t wrapped_src(int64_t i, int64_t n, int64_t b, int64_t cb) {
    if (i + cb < b) return i + cb;
    if (i >= n - cb) return i - (n - cb);
    return -1;
}

__global__ void __launch_bounds__(256)
k_place_wrapped(int64_t n0, int64_t n1, int64_t n2, int64_t ncols, int64_t b0, int64_t b1, int64_t b2,
                const float2* __restrict__ box, float2* __restrict__ vol, int64_t ld) {
    const int64_t N = n0 * n1 * n2, nb = b0 * b1 * b2, total = N * ncols;
    for (int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x; it < total; it += (int64_t)gridDim.x * 256) {
        const int64_t col = it / N, e = it - col * N;
        const int64_t i2 = e / (n0 * n1), r = e - i2 * (n0 * n1), i1 = r / n0, i0 = r - i1 * n0;
        const int64_t j0 = wrapped_src(i0, n0, b0, b0 / 2), j1 = wrapped_src(i1, n1, b1, b1 / 2), j2 = wrapped_src(i2, n2, b2, b2 / 2);
        float2 v = make_float2(0.f, 0.f);
        if (j0 >= 0 && j1 >= 0 && j2 >= 0) v = box[col * nb + j0 + b0 * (j1 + b1 * j2)];
        vol[col * ld + e] = v;
    }
}

// ---- nc <= 8: Jacobi, one lane per voxel -----------------------------------------------------------------------------------------
// a Hermitian NC x NC matrix as its real diagonal and its strict upper triangle (row-wise); all indices are compile-time after unrolling
template <int NC>
struct esp_herm {
    float  d[NC];
    float2 u[NC > 1 ? NC * (NC - 1) / 2 : 1];
    static __device__ __forceinline__ constexpr int at(int p, int q) { return p * (2 * NC - p - 1) / 2 + (q - p - 1); }
    __device__ __forceinline__ float2 get(int k, int p) const { return k < p ? u[at(k, p)] : cconj(u[at(p, k)]); }
    __device__ __forceinline__ void set(int k, int p, float2 v) { if (k < p) u[at(k, p)] = v; else u[at(p, k)] = cconj(v); }
};

template <int NC>
__global__ void __launch_bounds__(ESP_JBLK)
k_esp_jacobi(int64_t n, int nm, int iters, float crop, const float2* __restrict__ gram, int64_t ldg,
             float2* __restrict__ maps, int64_t ldm, float* __restrict__ evals, int64_t lde) {
    for (int64_t base = (int64_t)blockIdx.x * ESP_JBLK; base < n; base += (int64_t)gridDim.x * ESP_JBLK) {
        const int64_t i = base + threadIdx.x;
        const bool active = i < n;
        const int64_t ii = active ? i : n - 1;              // a lane past the end works on the last voxel and stores nothing
        esp_herm<NC> A;
        {
            const float2* gp = gram + ii;
#pragma unroll
            for (int p = 0; p < NC; ++p) {
#pragma unroll
                for (int q = p; q < NC; ++q, gp += ldg) {
                    const float2 v = *gp;
                    if (q == p) A.d[p] = v.x; else A.u[esp_herm<NC>::at(p, q)] = v;
                }
            }
        }
        float2 V[NC][NC];
#pragma unroll
        for (int r = 0; r < NC; ++r)
#pragma unroll
            for (int c = 0; c < NC; ++c) V[r][c] = make_float2(r == c ? 1.f : 0.f, 0.f);

        for (int sweep = 0; sweep < iters; ++sweep) {
            bool rotated = false;
#pragma unroll
            for (int p = 0; p < NC - 1; ++p) {
#pragma unroll
                for (int q = p + 1; q < NC; ++q) {
                    const float2 b = A.u[esp_herm<NC>::at(p, q)];
                    const float b2 = b.x * b.x + b.y * b.y;
                    const float app = A.d[p], aqq = A.d[q];
                    if (b2 > ESP_ROT2 * fabsf(app * aqq) + 1e-37f) {
                        rotated = true;
                        const float ab = sqrtf(b2);
                        const float tau = (aqq - app) / (2.f * ab);
                        const float t = copysignf(1.f, tau) / (fabsf(tau) + sqrtf(1.f + tau * tau));
                        const float c = 1.f / sqrtf(1.f + t * t), s = t * c;
                        const float2 w = cscale(s / ab, b);                     // s e^{i phi}, a_pq = |a_pq| e^{i phi}
                        const float2 mwc = make_float2(-w.x, w.y);              // -conj(w)
                        A.d[p] = app - t * ab;
                        A.d[q] = aqq + t * ab;
                        A.u[esp_herm<NC>::at(p, q)] = make_float2(0.f, 0.f);
#pragma unroll
                        for (int k = 0; k < NC; ++k) {
                            if (k == p || k == q) continue;
                            const float2 akp = A.get(k, p), akq = A.get(k, q);
                            float2 np_ = cscale(c, akp), nq_ = cscale(c, akq);
                            cfma(np_, mwc, akq);
                            cfma(nq_, w, akp);
                            A.set(k, p, np_);
                            A.set(k, q, nq_);
                        }
#pragma unroll
                        for (int k = 0; k < NC; ++k) {
                            const float2 vkp = V[k][p], vkq = V[k][q];
                            float2 np_ = cscale(c, vkp), nq_ = cscale(c, vkq);
                            cfma(np_, mwc, vkq);
                            cfma(nq_, w, vkp);
                            V[k][p] = np_;
                            V[k][q] = nq_;
                        }
                    }
                }
            }
            if (!__any(rotated ? 1 : 0)) break;
        }

        // the nm leading pairs, in descending order
        unsigned used = 0;
        for (int m = 0; m < nm; ++m) {
            float best = 0.f;
            int jb = -1;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const bool take = !((used >> j) & 1u) && (jb < 0 || A.d[j] > best);
                best = take ? A.d[j] : best;
                jb = take ? j : jb;
            }
            used |= 1u << jb;
            float2 v[NC];
            float nrm2 = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                v[c] = make_float2(0.f, 0.f);
#pragma unroll
                for (int j = 0; j < NC; ++j) v[c] = (jb == j) ? V[c][j] : v[c];
                nrm2 = fmaf(v[c].x, v[c].x, fmaf(v[c].y, v[c].y, nrm2));
            }
            const float inv = 1.f / sqrtf(nrm2);
#pragma unroll
            for (int c = 0; c < NC; ++c) v[c] = cscale(inv, v[c]);
            const float a0 = sqrtf(v[0].x * v[0].x + v[0].y * v[0].y);
            if (a0 >= ESP_MINPHASE) {
                const float2 ph = make_float2(v[0].x / a0, -v[0].y / a0);
#pragma unroll
                for (int c = 1; c < NC; ++c) v[c] = cmul(v[c], ph);
                v[0] = make_float2(a0, 0.f);
            }
            const bool keep = !(best < crop);
            if (active) {
                float2* mp = maps + i + ldm * (int64_t)(NC * m);
#pragma unroll
                for (int c = 0; c < NC; ++c, mp += ldm) *mp = keep ? v[c] : make_float2(0.f, 0.f);
                evals[i + lde * (int64_t)m] = best;
            }
        }
    }
}

// ---- nc <= 32: orthogonal iteration, L lanes per voxel --------------------------------------------------------------------------
template <int VPW>
__device__ __forceinline__ float esp_gsum(float x) {            // the sum over the members of a voxel: lanes at distance VPW, 2 VPW, ...
#pragma unroll
    for (int d = VPW; d < 64; d <<= 1) x += __shfl_xor(x, d);
    return x;
}

template <int R, int L, int NM>
__global__ void __launch_bounds__(ESP_OBLK)
k_esp_orth(int64_t n, int nc, int iters, float crop, const float2* __restrict__ gram, int64_t ldg,
           float2* __restrict__ maps, int64_t ldm, float* __restrict__ evals, int64_t lde) {
    constexpr int VPW = 64 / L, VPB = VPW * (ESP_OBLK / 64), NCP = R * L;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & (VPW - 1), l = lane / VPW;
    // (one group of VPB voxels per workgroup, no loop over groups: the R NCP lane-dependent column offsets would be hoisted out of
    // it and held in 2 R NCP registers for the whole kernel)
    {
        const int64_t i = (int64_t)blockIdx.x * VPB + wave * VPW + j;
        const bool active = i < n;
        const int64_t ii = active ? i : n - 1;
        float2 g[R][NCP];
#pragma unroll
        for (int rr = 0; rr < R; ++rr) {
            const int r = l * R + rr;
#pragma unroll
            for (int c = 0; c < NCP; ++c) {
                float2 v = make_float2(0.f, 0.f);
                if (r < nc && c < nc) {
                    const int a = r < c ? r : c, b = r < c ? c : r;
                    v = gram[ii + ldg * (int64_t)(a * nc - a * (a - 1) / 2 + (b - a))];
                    if (r > c) v.y = -v.y;
                    if (r == c) v.y = 0.f;
                }
                g[rr][c] = v;
            }
        }
        float2 v[R][NM], w[R][NM];
        float lam[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            lam[m] = 0.f;
#pragma unroll
            for (int rr = 0; rr < R; ++rr) {
                const int r = l * R + rr;
                const float ang = 2.399963f * (float)(r + 1) + 1.7f * (float)(m * (r + 3));
                v[rr][m] = r < nc ? make_float2(__cosf(ang), __sinf(ang)) : make_float2(0.f, 0.f);
            }
        }
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int m = 0; m < NM; ++m)
#pragma unroll
                for (int rr = 0; rr < R; ++rr) w[rr][m] = make_float2(0.f, 0.f);
#pragma unroll
            for (int ls = 0; ls < L; ++ls) {
#pragma unroll
                for (int s = 0; s < R; ++s) {
#pragma unroll
                    for (int m = 0; m < NM; ++m) {
                        const float2 x = make_float2(__shfl(v[s][m].x, j + VPW * ls), __shfl(v[s][m].y, j + VPW * ls));
#pragma unroll
                        for (int rr = 0; rr < R; ++rr) cfma(w[rr][m], g[rr][ls * R + s], x);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < NM; ++m) {
#pragma unroll
                for (int k = 0; k < m; ++k) {                   // v[.][k] already holds the new column k
                    float2 p = make_float2(0.f, 0.f);
#pragma unroll
                    for (int rr = 0; rr < R; ++rr) {
                        const float2 t = cmulc(v[rr][k], w[rr][m]);
                        p.x += t.x; p.y += t.y;
                    }
                    p.x = esp_gsum<VPW>(p.x);
                    p.y = esp_gsum<VPW>(p.y);
                    const float2 mp = make_float2(-p.x, -p.y);
#pragma unroll
                    for (int rr = 0; rr < R; ++rr) cfma(w[rr][m], mp, v[rr][k]);
                }
                float nrm2 = 0.f;
#pragma unroll
                for (int rr = 0; rr < R; ++rr) nrm2 = fmaf(w[rr][m].x, w[rr][m].x, fmaf(w[rr][m].y, w[rr][m].y, nrm2));
                const float nrm = sqrtf(esp_gsum<VPW>(nrm2));
                lam[m] = nrm;
                const float inv = nrm > 1e-30f ? 1.f / nrm : 0.f;
#pragma unroll
                for (int rr = 0; rr < R; ++rr) v[rr][m] = cscale(inv, w[rr][m]);
            }
        }
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const float2 v0 = make_float2(__shfl(v[0][m].x, j), __shfl(v[0][m].y, j));       // coil 0: member 0, its first row
            const float a0 = sqrtf(v0.x * v0.x + v0.y * v0.y);
            if (a0 >= ESP_MINPHASE) {
                const float2 ph = make_float2(v0.x / a0, -v0.y / a0);
#pragma unroll
                for (int rr = 0; rr < R; ++rr) v[rr][m] = cmul(v[rr][m], ph);
                if (l == 0) v[0][m] = make_float2(a0, 0.f);
            }
            const bool keep = !(lam[m] < crop);
            if (active) {
#pragma unroll
                for (int rr = 0; rr < R; ++rr) {
                    const int r = l * R + rr;
                    if (r < nc) maps[i + ldm * (int64_t)(r + nc * m)] = keep ? v[rr][m] : make_float2(0.f, 0.f);
                }
                if (l == 0) evals[i + lde * (int64_t)m] = lam[m];
            }
        }
    }
}

template <int R, int L>
void esp_launch_orth(ig_ctx* ctx, int64_t n, int nc, int nm, int iters, float crop, const float2* gram, int64_t ldg,
                     float2* maps, int64_t ldm, float* evals, int64_t lde) {
    const int vpb = (64 / L) * (ESP_OBLK / 64);
    const dim3 grid((unsigned)((n + vpb - 1) / vpb)), block(ESP_OBLK);
#define IG_ESP_ORTH(NM) hipLaunchKernelGGL((k_esp_orth<R, L, NM>), grid, block, 0, ctx->stream, n, nc, iters, crop, gram, ldg, maps, ldm, evals, lde)
    if (nm == 1) IG_ESP_ORTH(1); else if (nm == 2) IG_ESP_ORTH(2); else if (nm == 3) IG_ESP_ORTH(3); else IG_ESP_ORTH(4);
#undef IG_ESP_ORTH
}

}  // namespace

int ig_place_wrapped_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, int64_t b0, int64_t b1, int64_t b2,
                         const void* box, void* vol, int64_t ld) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_place_wrapped_c64: ctx is NULL");
    if (n0 < 1 || n1 < 1 || n2 < 1 || ncols < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_place_wrapped_c64: %lld volumes of %lld x %lld x %lld, at least one element each",
                       (long long)ncols, (long long)n0, (long long)n1, (long long)n2);
    if (b0 < 1 || b1 < 1 || b2 < 1 || b0 > n0 || b1 > n1 || b2 > n2)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_place_wrapped_c64: a box of %lld x %lld x %lld in a volume of %lld x %lld x %lld: every side "
                       "between 1 and the volume's", (long long)b0, (long long)b1, (long long)b2, (long long)n0, (long long)n1, (long long)n2);
    const int64_t N = n0 * n1 * n2, nb = b0 * b1 * b2;
    IG_REQUIRE(ctx, ld >= N, "ig_place_wrapped_c64: leading dimension %lld below N = %lld", (long long)ld, (long long)N);
    IG_REQUIRE(ctx, box && vol, "ig_place_wrapped_c64: NULL pointer");
    const uintptr_t s0 = (uintptr_t)box, s1 = s0 + (uintptr_t)(nb * ncols) * sizeof(float2);
    const uintptr_t v0 = (uintptr_t)vol, v1 = v0 + (uintptr_t)((ncols - 1) * ld + N) * sizeof(float2);
    IG_REQUIRE(ctx, !ig_bytes_overlap(s0, s1, v0, v1), "ig_place_wrapped_c64: the volumes overlap the boxes");
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, "place_wrapped", 8.0 * (double)ncols * (double)(N + nb));
    hipLaunchKernelGGL(k_place_wrapped, ig_grid_1d(N * ncols, 256, ESP_MAXGRID), dim3(256), 0, ctx->stream, n0, n1, n2, ncols, b0, b1, b2,
                       (const float2*)box, (float2*)vol, ld);
    IG_LAUNCH_CHECK(ctx, "k_place_wrapped");
    return IG_OK;
}

int ig_espirit_eig_c64(ig_ctx* ctx, int64_t n, int64_t nc, int64_t nm, int64_t iters, float crop, const void* gram, int64_t ldg,
                       void* maps, int64_t ldm, float* evals, int64_t lde) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_espirit_eig_c64: ctx is NULL");
    if (nc < 1 || nc > ESP_MAXC)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_espirit_eig_c64: %lld coils, between 1 and %d are supported", (long long)nc, ESP_MAXC);
    if (nm < 1 || nm > ESP_MAXM || nm > nc)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_espirit_eig_c64: %lld sets of maps from %lld coils, between 1 and min(%d, coils) are supported",
                       (long long)nm, (long long)nc, ESP_MAXM);
    if (n < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_espirit_eig_c64: %lld voxels, at least 1 is supported", (long long)n);
    if (iters < 0 || iters > 100000)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_espirit_eig_c64: %lld iterations, between 0 and 100000 are supported", (long long)iters);
    IG_REQUIRE(ctx, ldg >= n && ldm >= n && lde >= n, "ig_espirit_eig_c64: leading dimensions (%lld, %lld, %lld) below n = %lld",
               (long long)ldg, (long long)ldm, (long long)lde, (long long)n);
    IG_REQUIRE(ctx, gram && maps && evals, "ig_espirit_eig_c64: NULL pointer");
    if (nc > 8 && n > ((int64_t)1 << 33))
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_espirit_eig_c64: %lld voxels with %lld coils, at most 2^33 are supported beyond 8 coils", (long long)n, (long long)nc);
    const int64_t ntri = nc * (nc + 1) / 2;
    const uintptr_t g0 = (uintptr_t)gram, g1 = g0 + (uintptr_t)((ntri - 1) * ldg + n) * sizeof(float2);
    const uintptr_t m0 = (uintptr_t)maps, m1 = m0 + (uintptr_t)((nc * nm - 1) * ldm + n) * sizeof(float2);
    const uintptr_t e0 = (uintptr_t)evals, e1 = e0 + (uintptr_t)((nm - 1) * lde + n) * sizeof(float);
    IG_REQUIRE(ctx, !ig_bytes_overlap(g0, g1, m0, m1), "ig_espirit_eig_c64: maps overlaps gram");
    IG_REQUIRE(ctx, !ig_bytes_overlap(g0, g1, e0, e1), "ig_espirit_eig_c64: evals overlaps gram");
    IG_REQUIRE(ctx, !ig_bytes_overlap(m0, m1, e0, e1), "ig_espirit_eig_c64: evals overlaps maps");
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, nc <= 8 ? "espirit_eig_jacobi" : "espirit_eig_orth", (double)n * (8.0 * (double)(ntri + nc * nm) + 4.0 * (double)nm));
    const float2* G = (const float2*)gram;
    float2* M = (float2*)maps;
    const int c = (int)nc, m = (int)nm, it = (int)iters;
    if (nc <= 8) {
        const dim3 grid = ig_grid_1d(n, ESP_JBLK, ESP_MAXGRID), block(ESP_JBLK);
#define IG_ESP_JAC(NC) hipLaunchKernelGGL((k_esp_jacobi<NC>), grid, block, 0, ctx->stream, n, m, it, crop, G, ldg, M, ldm, evals, lde)
        switch (c) {
            case 1: IG_ESP_JAC(1); break;
            case 2: IG_ESP_JAC(2); break;
            case 3: IG_ESP_JAC(3); break;
            case 4: IG_ESP_JAC(4); break;
            case 5: IG_ESP_JAC(5); break;
            case 6: IG_ESP_JAC(6); break;
            case 7: IG_ESP_JAC(7); break;
            default: IG_ESP_JAC(8); break;
        }
#undef IG_ESP_JAC
    } else if (nc <= 16) {
        esp_launch_orth<4, 4>(ctx, n, c, m, it, crop, G, ldg, M, ldm, evals, lde);
    } else {
        esp_launch_orth<2, 16>(ctx, n, c, m, it, crop, G, ldg, M, ldm, evals, lde);
    }
    IG_LAUNCH_CHECK(ctx, "k_esp_eig");
    return IG_OK;
}
