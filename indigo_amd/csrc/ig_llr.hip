// Block-wise singular-value thresholding and nuclear norms of the frame panel: the proximal map and the value of the locally
// low-rank penalty (Backend.llr_threshold / llr_norm, pics --llr).
//
// x is the N x nt panel of nt frames of an F-ordered n0 x n1 x n2 volume (N voxels, axis 0 fastest).  Voxel i has the shifted
// coordinates j_a = (i_a + s_a) mod n_a and belongs to block (j_0 / b_0, j_1 / b_1, j_2 / b_2); the blocks tile the shifted
// volume, the last one of an axis is shorter when b_a does not divide n_a, and with a shift a block wraps around in i.  There
// are nb = prod ceil(n_a / b_a) blocks, numbered F-order.  M_b is the (voxels of block b) x nt matrix of x:
//   svt : M_b <- M_b P_b,  P_b = V diag(sigma_k > tau ? 1 - tau / sigma_k : 0) V^H,  M_b^H M_b = V diag(sigma_k^2) V^H
//   nuc : nuc[b] = sum_k sigma_k
//
// One workgroup per block at a time (the grid strides over the blocks), one lane per voxel, the lane's nt values in registers:
//   1. the lanes load their rows; x-neighbours of a block are neighbouring lanes, so b_0 = 8 voxels are one 64-byte run;
//   2. the nt x nt Hermitian Gram matrix M^H M, its upper triangle, is accumulated in float64: the rows go through LDS 128
//      voxels at a time, a thread owns one entry (a, b) and a slice of the voxels, and the slices are added in a fixed order
//      (no atomics: equal inputs give equal bits).  Products of two floats are exact in float64; what is rounded is the sum;
//   3. the whole workgroup diagonalises it by Jacobi rotations in float64, in the round-robin order that makes the nt/2
//      rotations of a round independent: a thread updates the 2 x 2 group of entries that a pair of pairs owns, in place.
//      A sweep in which no off-diagonal entry exceeded 1e-15 * trace ends the iteration (at most 15 sweeps);
//   4. P_b in float32 in LDS, and every lane multiplies its row by it and stores it: x moves once in and once out, 16 bytes
//      per voxel and frame.  The norms stop after step 3 (no eigenvectors): 8 bytes per voxel and frame, 4 per block.
// tau == 0 goes through P_b = V V^H like any other value; tau >= every sigma makes P_b exactly 0.
#include "ig_common.h"

namespace {

constexpr int LLR_MAXT = 32;           // frames
constexpr int LLR_MAXV = 1024;         // voxels of a block = threads of the workgroup
constexpr int LLR_STAGE = 128;         // voxels whose rows are in LDS at a time while the Gram matrix is accumulated
constexpr int LLR_SWEEPS = 15;

struct cd { double x, y; };

struct llr_geom {
    int64_t n0, n1, n2, nb0, nb1, nb;
    int b0, b1, b2, s0, s1, s2, nt;
};

// index of entry (i, j), i <= j, in the row-wise upper triangle of an nt x nt matrix
__device__ __forceinline__ int tri(int i, int j, int nt) { return i * nt - i * (i - 1) / 2 + (j - i); }

// side of a block: b, or what is left of the axis
__device__ __forceinline__ int extent(int b, int64_t left) { return left < b ? (int)left : b; }

// NT: the even compile-time bound of the register image, nt <= NT.  SVT false: the nuclear norms
template <int NT, bool SVT>
__global__ void __launch_bounds__(LLR_MAXV)
k_llr(llr_geom g, float tau, float2* __restrict__ x, int64_t ldx, float* __restrict__ nuc) {
    constexpr int TRI = NT * (NT + 1) / 2;
    constexpr int SLD = NT + 1;                                    // odd row stride of the staged rows, in float2
    constexpr int STAGE_BYTES = LLR_STAGE * SLD * 8;               // a multiple of 16
    constexpr int GRAM_BYTES = STAGE_BYTES + LLR_MAXV * 16;
    constexpr int EIG_BYTES = NT * NT * (16 + 16 + 8);
    constexpr int RAW_BYTES = GRAM_BYTES > EIG_BYTES ? GRAM_BYTES : EIG_BYTES;
    // steps 2 and 3 / 4 use the same memory one after the other
    __shared__ __align__(16) unsigned char raw[RAW_BYTES];
    __shared__ cd gtri[TRI];
    __shared__ unsigned char pa[TRI], pb[TRI];                     // (a, b) of a triangle entry
    __shared__ double rc[NT];                                      // cosine of the rotation of an index; then the shrink factors
    __shared__ cd roff[NT];                                        // J[partner(i)][i]
    __shared__ unsigned char prp[NT / 2], prq[NT / 2];             // the pairs of this round
    __shared__ int flags[LLR_SWEEPS];
    float2* const stage = reinterpret_cast<float2*>(raw);
    cd* const partial = reinterpret_cast<cd*>(raw + STAGE_BYTES);
    cd* const A = reinterpret_cast<cd*>(raw);
    cd* const V = A + NT * NT;
    float2* const P = reinterpret_cast<float2*>(V + NT * NT);

    const int nt = g.nt, m = nt + (nt & 1), h = m / 2, ntri = nt * (nt + 1) / 2;
    const int bd = blockDim.x, tid = threadIdx.x;
    const int nsl = bd >= ntri ? bd / ntri : 1, nwork = ntri * nsl;     // nwork <= max(bd, ntri) <= LLR_MAXV

    for (int e = tid; e < ntri; e += bd) {
        int a = 0, r = e;
        while (r >= nt - a) { r -= nt - a; ++a; }
        pa[e] = (unsigned char)a;
        pb[e] = (unsigned char)(a + r);
    }

    for (int64_t blk = blockIdx.x; blk < g.nb; blk += gridDim.x) {
        // ---- 1. this block's extent and this lane's voxel
        const int64_t k0 = blk % g.nb0, k1 = (blk / g.nb0) % g.nb1, k2 = blk / (g.nb0 * g.nb1);
        const int e0 = extent(g.b0, g.n0 - k0 * g.b0), e1 = extent(g.b1, g.n1 - k1 * g.b1), e2 = extent(g.b2, g.n2 - k2 * g.b2);
        const int vblk = e0 * e1 * e2;                                  // 1 <= vblk <= bd
        const bool active = tid < vblk;
        int64_t idx = 0;
        if (active) {
            int64_t i0 = k0 * g.b0 + tid % e0 - g.s0, i1 = k1 * g.b1 + (tid / e0) % e1 - g.s1, i2 = k2 * g.b2 + tid / (e0 * e1) - g.s2;
            if (i0 < 0) i0 += g.n0;
            if (i1 < 0) i1 += g.n1;
            if (i2 < 0) i2 += g.n2;
            idx = i0 + g.n0 * (i1 + g.n1 * i2);
        }
        float2 xr[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) xr[t] = (active && t < nt) ? x[idx + t * ldx] : make_float2(0.f, 0.f);

        // ---- 2. the Gram matrix
        for (int e = tid; e < ntri; e += bd) gtri[e] = cd{0.0, 0.0};
        for (int c0 = 0; c0 < vblk; c0 += LLR_STAGE) {
            const int cnt = min(LLR_STAGE, vblk - c0);
            if (tid >= c0 && tid < c0 + cnt) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t < nt) stage[(tid - c0) * SLD + t] = xr[t];
            }
            __syncthreads();
            for (int w = tid; w < nwork; w += bd) {
                const int e = w % ntri, s = w / ntri, a = pa[e], b = pb[e];
                double re = 0.0, im = 0.0;
                for (int v = s; v < cnt; v += nsl) {                    // conj(p) * q
                    const float2 p = stage[v * SLD + a], q = stage[v * SLD + b];
                    const double px = p.x, py = p.y, qx = q.x, qy = q.y;
                    re = fma(px, qx, re); re = fma(py, qy, re);
                    im = fma(px, qy, im); im = fma(-py, qx, im);
                }
                partial[w] = cd{re, im};
            }
            __syncthreads();
            for (int e = tid; e < ntri; e += bd) {
                cd acc = gtri[e];
                for (int s = 0; s < nsl; ++s) { acc.x += partial[e + s * ntri].x; acc.y += partial[e + s * ntri].y; }
                gtri[e] = acc;
            }
            __syncthreads();
        }

        // ---- 3. A = the m x m Hermitian matrix (a zero row and column when nt is odd), V = I; Jacobi
        double trace = 0.0;
        for (int k = 0; k < nt; ++k) trace += gtri[tri(k, k, nt)].x;
        const double thr = 1e-15 * trace, thr2 = thr * thr;
        for (int it = tid; it < m * m; it += bd) {
            const int i = it / m, j = it % m;
            cd val{0.0, 0.0};
            if (i < nt && j < nt) {
                if (i <= j) val = gtri[tri(i, j, nt)];
                else { val = gtri[tri(j, i, nt)]; val.y = -val.y; }
                if (i == j) val.y = 0.0;
            }
            A[i * NT + j] = val;
            if (SVT) V[i * NT + j] = cd{i == j ? 1.0 : 0.0, 0.0};
        }
        if (tid < LLR_SWEEPS) flags[tid] = 0;
        __syncthreads();
        for (int sweep = 0; sweep < LLR_SWEEPS; ++sweep) {
            for (int r = 0; r < m - 1; ++r) {
                if (tid < h) {                                          // pair tid of round r and its rotation
                    const int p = tid == 0 ? r : (r + tid) % (m - 1), q = tid == 0 ? m - 1 : (r - tid + m - 1) % (m - 1);
                    const double al = A[p * NT + p].x, be = A[q * NT + q].x;
                    const cd ga = A[p * NT + q];
                    const double g2 = ga.x * ga.x + ga.y * ga.y;
                    double c = 1.0;
                    cd op{0.0, 0.0}, oq{0.0, 0.0};
                    if (g2 > thr2) {                                    // (false for a NaN: the block then stays NaN, untouched)
                        const double ag = sqrt(g2), ux = ga.x / ag, uy = ga.y / ag;
                        const double th = (be - al) / (2.0 * ag);
                        const double t = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        const double s = t * c;
                        op = cd{-s * ux, s * uy};                       // J[q][p] = -s conj(u)
                        oq = cd{s * ux, s * uy};                        // J[p][q] =  s u
                        flags[sweep] = 1;
                    }
                    rc[p] = c; rc[q] = c;
                    roff[p] = op; roff[q] = oq;
                    prp[tid] = (unsigned char)p; prq[tid] = (unsigned char)q;
                }
                __syncthreads();
                // A <- J^H A J: the entries in rows {p1, p2} and columns {q1, q2} depend on one another only
                for (int it = tid; it < h * h; it += bd) {
                    const int p1 = prp[it / h], p2 = prq[it / h], q1 = prp[it % h], q2 = prq[it % h];
                    const double cp = rc[p1], cq = rc[q1];
                    const cd o1 = roff[p1], o2 = roff[p2], f1 = roff[q1], f2 = roff[q2];
                    const cd a11 = A[p1 * NT + q1], a12 = A[p1 * NT + q2], a21 = A[p2 * NT + q1], a22 = A[p2 * NT + q2];
                    // B = A J
                    const cd b11{a11.x * cq + a12.x * f1.x - a12.y * f1.y, a11.y * cq + a12.x * f1.y + a12.y * f1.x};
                    const cd b12{a11.x * f2.x - a11.y * f2.y + a12.x * cq, a11.x * f2.y + a11.y * f2.x + a12.y * cq};
                    const cd b21{a21.x * cq + a22.x * f1.x - a22.y * f1.y, a21.y * cq + a22.x * f1.y + a22.y * f1.x};
                    const cd b22{a21.x * f2.x - a21.y * f2.y + a22.x * cq, a21.x * f2.y + a21.y * f2.x + a22.y * cq};
                    // J^H B: row p1 = cp B1 + conj(o1) B2, row p2 = conj(o2) B1 + cp B2
                    A[p1 * NT + q1] = cd{cp * b11.x + o1.x * b21.x + o1.y * b21.y, cp * b11.y + o1.x * b21.y - o1.y * b21.x};
                    A[p1 * NT + q2] = cd{cp * b12.x + o1.x * b22.x + o1.y * b22.y, cp * b12.y + o1.x * b22.y - o1.y * b22.x};
                    A[p2 * NT + q1] = cd{o2.x * b11.x + o2.y * b11.y + cp * b21.x, o2.x * b11.y - o2.y * b11.x + cp * b21.y};
                    A[p2 * NT + q2] = cd{o2.x * b12.x + o2.y * b12.y + cp * b22.x, o2.x * b12.y - o2.y * b12.x + cp * b22.y};
                }
                if (SVT)                                                // V <- V J
                    for (int it = tid; it < m * h; it += bd) {
                        const int k = it / h, q1 = prp[it % h], q2 = prq[it % h];
                        const double cq = rc[q1];
                        const cd f1 = roff[q1], f2 = roff[q2];
                        const cd v1 = V[k * NT + q1], v2 = V[k * NT + q2];
                        V[k * NT + q1] = cd{v1.x * cq + v2.x * f1.x - v2.y * f1.y, v1.y * cq + v2.x * f1.y + v2.y * f1.x};
                        V[k * NT + q2] = cd{v1.x * f2.x - v1.y * f2.y + v2.x * cq, v1.x * f2.y + v1.y * f2.x + v2.y * cq};
                    }
                __syncthreads();
            }
            if (!flags[sweep]) break;                                   // written before the round's barriers: the same for every thread
        }

        if (!SVT) {
            if (tid == 0) {
                double sum = 0.0;
                for (int k = 0; k < nt; ++k) sum += sqrt(fmax(A[k * NT + k].x, 0.0));
                nuc[blk] = (float)sum;
            }
        } else {
            // ---- 4. P = V diag(f) V^H, and the rows times P
            if (tid < nt) {
                const double sg = sqrt(fmax(A[tid * NT + tid].x, 0.0));
                rc[tid] = sg > (double)tau ? 1.0 - (double)tau / sg : 0.0;
            }
            __syncthreads();
            for (int it = tid; it < nt * nt; it += bd) {
                const int a = it / nt, b = it % nt;
                double re = 0.0, im = 0.0;
                for (int k = 0; k < nt; ++k) {                          // f_k V[a][k] conj(V[b][k])
                    const cd va = V[a * NT + k], vb = V[b * NT + k];
                    re += rc[k] * (va.x * vb.x + va.y * vb.y);
                    im += rc[k] * (va.y * vb.x - va.x * vb.y);
                }
                P[a * NT + b] = make_float2((float)re, (float)im);
            }
            __syncthreads();
            if (active) {
#pragma unroll 1
                for (int b = 0; b < nt; ++b) {
                    float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                    for (int a = 0; a < NT; ++a)
                        if (a < nt) cfma(acc, xr[a], P[a * NT + b]);
                    x[idx + b * ldx] = acc;
                }
            }
        }
        __syncthreads();                                                // the next block stages its rows over A, V and P
    }
}

template <bool SVT>
void llr_launch(ig_ctx* ctx, const llr_geom& g, int threads, float tau, float2* x, int64_t ldx, float* nuc) {
    const int64_t cap = (int64_t)ctx->num_cu * 8;
    const dim3 grid((unsigned)(g.nb < cap ? g.nb : cap)), block((unsigned)threads);
#define IG_LLR_CASE(NT) hipLaunchKernelGGL((k_llr<NT, SVT>), grid, block, 0, ctx->stream, g, tau, x, ldx, nuc)
    if (g.nt <= 2) IG_LLR_CASE(2);
    else if (g.nt <= 4) IG_LLR_CASE(4);
    else if (g.nt <= 8) IG_LLR_CASE(8);
    else if (g.nt <= 16) IG_LLR_CASE(16);
    else IG_LLR_CASE(32);
#undef IG_LLR_CASE
}

// the checks that both entries share; IG_OK with *empty set when there is nothing to do
int llr_prepare(ig_ctx* ctx, const char* who, int64_t n0, int64_t n1, int64_t n2, int64_t nt, int64_t b0, int64_t b1, int64_t b2,
                int64_t s0, int64_t s1, int64_t s2, const void* x, int64_t ldx, llr_geom* g, int* threads, bool* empty) {
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && nt >= 0, "%s: negative dimension", who);
    IG_REQUIRE(ctx, b0 >= 1 && b1 >= 1 && b2 >= 1, "%s: block side below 1 (%lld, %lld, %lld)", who, (long long)b0, (long long)b1, (long long)b2);
    const int64_t vol = n0 * n1 * n2;
    IG_REQUIRE(ctx, ldx >= vol, "%s: leading dimension %lld below N = %lld", who, (long long)ldx, (long long)vol);
    *empty = (vol == 0 || nt == 0);
    if (*empty) return IG_OK;
    b0 = b0 < n0 ? b0 : n0; b1 = b1 < n1 ? b1 : n1; b2 = b2 < n2 ? b2 : n2;
    IG_REQUIRE(ctx, s0 >= 0 && s0 < b0 && s1 >= 0 && s1 < b1 && s2 >= 0 && s2 < b2,
               "%s: shift (%lld, %lld, %lld) outside [0, block side) for the clamped block (%lld, %lld, %lld)", who,
               (long long)s0, (long long)s1, (long long)s2, (long long)b0, (long long)b1, (long long)b2);
    IG_REQUIRE(ctx, x != nullptr, "%s: NULL pointer", who);
    if (nt > LLR_MAXT)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "%s: %lld frames, at most %d are supported", who, (long long)nt, LLR_MAXT);
    if (b0 * b1 * b2 > LLR_MAXV)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "%s: a block of %lld x %lld x %lld = %lld voxels, at most %d are supported", who,
                       (long long)b0, (long long)b1, (long long)b2, (long long)(b0 * b1 * b2), LLR_MAXV);
    g->n0 = n0; g->n1 = n1; g->n2 = n2;
    g->nb0 = (n0 + b0 - 1) / b0; g->nb1 = (n1 + b1 - 1) / b1;
    g->nb = g->nb0 * g->nb1 * ((n2 + b2 - 1) / b2);
    g->b0 = (int)b0; g->b1 = (int)b1; g->b2 = (int)b2;
    g->s0 = (int)s0; g->s1 = (int)s1; g->s2 = (int)s2;
    g->nt = (int)nt;
    *threads = (int)((b0 * b1 * b2 + 63) / 64 * 64);
    return IG_OK;
}

}  // namespace

int ig_llr_svt_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t nt, int64_t b0, int64_t b1, int64_t b2,
                   int64_t s0, int64_t s1, int64_t s2, float tau, void* x, int64_t ldx) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_llr_svt_c64: ctx is NULL");
    IG_REQUIRE(ctx, tau >= 0.f, "ig_llr_svt_c64: threshold %g is not >= 0", (double)tau);
    llr_geom g;
    int threads = 0;
    bool empty = false;
    if (int rc = llr_prepare(ctx, "ig_llr_svt_c64", n0, n1, n2, nt, b0, b1, b2, s0, s1, s2, x, ldx, &g, &threads, &empty)) return rc;
    if (empty) return IG_OK;
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, "llr_svt", (double)n0 * n1 * n2 * nt * 16.0);
    llr_launch<true>(ctx, g, threads, tau, (float2*)x, ldx, nullptr);
    IG_LAUNCH_CHECK(ctx, "k_llr (svt)");
    return IG_OK;
}

int ig_llr_nuc_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t nt, int64_t b0, int64_t b1, int64_t b2,
                   int64_t s0, int64_t s1, int64_t s2, const void* x, int64_t ldx, float* nuc) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_llr_nuc_c64: ctx is NULL");
    llr_geom g;
    int threads = 0;
    bool empty = false;
    if (int rc = llr_prepare(ctx, "ig_llr_nuc_c64", n0, n1, n2, nt, b0, b1, b2, s0, s1, s2, x, ldx, &g, &threads, &empty)) return rc;
    if (empty) return IG_OK;
    IG_REQUIRE(ctx, nuc != nullptr, "ig_llr_nuc_c64: NULL pointer");
    const uintptr_t p0 = (uintptr_t)x, p1 = p0 + (uintptr_t)((nt - 1) * ldx + n0 * n1 * n2) * sizeof(float2);
    const uintptr_t q0 = (uintptr_t)nuc, q1 = q0 + (uintptr_t)g.nb * sizeof(float);
    IG_REQUIRE(ctx, !(p0 < q1 && q0 < p1), "ig_llr_nuc_c64: nuc overlaps x");
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, "llr_nuc", (double)n0 * n1 * n2 * nt * 8.0 + (double)g.nb * 4.0);
    llr_launch<false>(ctx, g, threads, 0.f, (float2*)const_cast<void*>(x), ldx, nuc);
    IG_LAUNCH_CHECK(ctx, "k_llr (nuc)");
    return IG_OK;
}
