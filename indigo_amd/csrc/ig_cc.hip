// The coil Gram matrix of coil compression and noise prewhitening (indigo_amd.cc, Backend.coil_gram).
//
// x is a column-major n x nc panel of samples (coil c is column c, ldx >= n).  G[p, q] = sum_i x[i, p] conj(x[i, q]) is Hermitian;
// the kernel writes, for every slab of `slab` consecutive samples, one row of `parts`: the row-wise upper triangle of that slab's G
// in the packing of ig_espirit_eig_c64 (column p nc - p (p - 1) / 2 + (q - p) is [p, q], p <= q).  The host adds the rows in float64.
//
// A tall-skinny Hermitian rank-n update on the matrix cores with float32 inputs (v_mfma_f32_32x32x2_f32, v_mfma_f32_16x16x4_f32: exact
// float32 products, one rounding per product, at the vector rate).  With Z = [Re x | Im x], a real n x 2 CP panel (CP = nc rounded up to
// 8, 16, 32 or 64; the columns of coils >= nc are zero), M = Z^T Z is symmetric and
//     Re G[p, q] = M[p, q] + M[CP + p, CP + q],      Im G[p, q] = M[CP + p, q] - M[p, CP + q].
// M is cut into 32 x 32 tiles and only the tiles of its block upper triangle are computed (a tile below it is the transpose of one
// above): 10 tiles at CP = 64, 3 at CP = 32; at CP = 16 M is one 32 x 32 tile, at CP = 8 one 16 x 16 tile (K = 4 samples per MFMA).
// Both operands of a tile come from Z: lane (column, k slot) of a wave holds one float per 32-column block of Z, which is the A
// operand of the tiles in that block row and the B operand of the tiles in that block column -- at CP = 64 two 8-byte loads feed ten
// MFMAs.  No LDS on the way in: the k slots of an MFMA may hold any samples as long as A and B agree, so lane (column, slot s) takes the
// R consecutive samples [s R, (s + 1) R) of the wave's chunk of K R samples for its R MFMA steps: every lane reads a contiguous run of
// 8 R bytes of its coil's column, and the next chunk's loads are issued before the current chunk's MFMAs.
//
// Summation order (fixed: no atomics, two calls give the same bits).  One workgroup of NW waves per slab, NW = 8 (4 at CP = 64).
// Wave w takes the chunks w, w + NW, ... of the slab, so an accumulator is a float32 fma chain over slab / NW samples (2048 at the
// default slab of 16384, 4096 at CP = 64); the waves' tiles are then added pairwise through LDS, (w, w + NW / 2), ..., (w, w + 1), and
// the 2 CP x 2 CP image of M in LDS gives the packed row.  The diagonal's imaginary part is written as an exact zero.  Samples beyond
// the slab's end are never loaded (their operand is a literal zero), so rows of x below n are never read; a lane whose coil is >= nc
// reads inside the panel and uses a literal zero.
#include "ig_common.h"

#include <type_traits>

namespace {

constexpr int GRAM_MAXC = 64;
constexpr int64_t GRAM_MAXGRID = 1 << 20;       // workgroups; the slab loop strides beyond that

typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));

template <int CP>
struct gram_cfg {
    static constexpr bool SMALL = CP == 8;                  // one 16 x 16 tile, K = 4
    static constexpr int TD = SMALL ? 16 : 32;              // tile side
    static constexpr int K = 64 / TD;                       // samples per MFMA
    static constexpr int NBC = CP <= 32 ? 1 : CP / 32;      // 32-coil blocks: 8-byte loads per lane and sample
    static constexpr int NBZ = CP <= 16 ? 1 : 2 * NBC;      // 32-column blocks of Z
    static constexpr int NT = NBZ * (NBZ + 1) / 2;          // tiles of the block upper triangle of M
    static constexpr int AR = SMALL ? 4 : 16;               // accumulator registers of a tile
    // waves of a workgroup and consecutive samples of a lane per chunk.  CP = 64 holds 160 accumulators: four waves, one per SIMD with
    // the whole register file, and chunks of 32 samples (a 128-byte line per lane, 10240 MFMA cycles) so that the one chunk in flight
    // covers the memory latency; with eight waves and room for chunks of 4 samples only, 2^24 samples took 5.2 ms in place of 3.0
    static constexpr int NW = CP == 64 ? 4 : 8;
    static constexpr int R = CP == 64 ? 16 : 8;
    typedef typename std::conditional<SMALL, f32x4_t, f32x16_t>::type acc_t;
};

template <int CP>
__device__ __forceinline__ typename gram_cfg<CP>::acc_t gram_mfma(float a, float b, typename gram_cfg<CP>::acc_t c) {
    if constexpr (gram_cfg<CP>::SMALL) return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// the lane's operands of chunk `ch` of the slab [s0, s1): z[b][r] is its element of block b of Z at its sample r -- the real part
// of its coil in the blocks of Re x, the imaginary part in those of Im x; where Z is one block, `imag` says which of the two the
// lane's column is.  Zero past the slab's end, where nothing is read, and for a coil >= nc: a chunk that lies inside the slab
// (wave-uniform) is loaded without per-sample tests, a lane whose coil is >= nc reading coil nc - 1 and discarding it.
template <int CP>
__device__ __forceinline__ void gram_load(float (&z)[gram_cfg<CP>::NBZ][gram_cfg<CP>::R], const float2* __restrict__ x, int64_t ldx,
                                          int nc, int coil0, bool imag, int slot, int64_t s0, int64_t s1, int64_t ch) {
    typedef gram_cfg<CP> cfg;
    const int64_t chunk0 = s0 + ch * (cfg::K * cfg::R), first = chunk0 + slot * cfg::R;
    const bool whole = chunk0 + cfg::K * cfg::R <= s1;
#pragma unroll
    for (int P = 0; P < cfg::NBC; ++P) {
        const int coil = coil0 + 32 * P;
        const bool live = coil < nc;
        const float2* xp = x + first + (int64_t)(live ? coil : nc - 1) * ldx;
        float2 v[cfg::R];
        if (whole) {
#pragma unroll
            for (int r = 0; r < cfg::R; ++r) v[r] = xp[r];
        } else {
#pragma unroll
            for (int r = 0; r < cfg::R; ++r) v[r] = first + r < s1 ? xp[r] : make_float2(0.f, 0.f);
        }
#pragma unroll
        for (int r = 0; r < cfg::R; ++r) {
            if constexpr (cfg::NBZ == 1) {
                z[0][r] = live ? (imag ? v[r].y : v[r].x) : 0.f;
            } else {
                z[P][r] = live ? v[r].x : 0.f;
                z[cfg::NBC + P][r] = live ? v[r].y : 0.f;
            }
        }
    }
}

// element (a, b) of the symmetric M from the tiles of its block upper triangle
template <int CP>
__device__ __forceinline__ float gram_m(const float (*mt)[gram_cfg<CP>::TD * gram_cfg<CP>::TD], int a, int b) {
    typedef gram_cfg<CP> cfg;
    if constexpr (cfg::NBZ == 1) {
        return mt[0][a * cfg::TD + b];
    } else {
        int I = a >> 5, J = b >> 5, i = a & 31, j = b & 31;
        if (I > J) { int t = I; I = J; J = t; t = i; i = j; j = t; }
        return mt[I * cfg::NBZ - I * (I - 1) / 2 + (J - I)][i * 32 + j];
    }
}

template <int CP>
__global__ void __launch_bounds__(64 * gram_cfg<CP>::NW)
k_coil_gram(int64_t n, int nc, const float2* __restrict__ x, int64_t ldx, int64_t slab, int64_t nslabs, float2* __restrict__ parts, int64_t ldp) {
    typedef gram_cfg<CP> cfg;
    typedef typename cfg::acc_t acc_t;
    __shared__ float red[cfg::NW / 2][cfg::AR * 64];
    __shared__ float mt[cfg::NT][cfg::TD * cfg::TD];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & (cfg::TD - 1), slot = lane / cfg::TD;
    // the coil of the lane's loads (block 0) and, where Z is one block, whether its column of Z is the imaginary part
    const int coil0 = CP <= 16 ? (col & (CP - 1)) : col;
    const bool imag = CP <= 16 && col >= CP;
    constexpr int64_t CHUNK = cfg::K * cfg::R;

    for (int64_t j = blockIdx.x; j < nslabs; j += gridDim.x) {
        const int64_t s0 = j * slab, s1 = s0 + slab < n ? s0 + slab : n;
        const int64_t nch = (s1 - s0 + CHUNK - 1) / CHUNK;
        acc_t acc[cfg::NT];
#pragma unroll
        for (int t = 0; t < cfg::NT; ++t)
#pragma unroll
            for (int r = 0; r < cfg::AR; ++r) acc[t][r] = 0.f;

        float cur[cfg::NBZ][cfg::R], nxt[cfg::NBZ][cfg::R];
        gram_load<CP>(cur, x, ldx, nc, coil0, imag, slot, s0, s1, wave);
        for (int64_t ch = wave; ch < nch; ch += cfg::NW) {
            gram_load<CP>(nxt, x, ldx, nc, coil0, imag, slot, s0, s1, ch + cfg::NW);          // (past the slab's end: zeros, no loads)
#pragma unroll
            for (int r = 0; r < cfg::R; ++r) {
                int t = 0;
#pragma unroll
                for (int I = 0; I < cfg::NBZ; ++I)
#pragma unroll
                    for (int J = I; J < cfg::NBZ; ++J, ++t) acc[t] = gram_mfma<CP>(cur[I][r], cur[J][r], acc[t]);
            }
#pragma unroll
            for (int b = 0; b < cfg::NBZ; ++b)
#pragma unroll
                for (int r = 0; r < cfg::R; ++r) cur[b][r] = nxt[b][r];
        }

        // the waves' tiles, added pairwise; wave 0 leaves the sums in mt as M's tiles, row-major
#pragma unroll
        for (int t = 0; t < cfg::NT; ++t) {
#pragma unroll
            for (int half = cfg::NW / 2; half >= 1; half >>= 1) {
                if (wave >= half && wave < 2 * half) {
#pragma unroll
                    for (int r = 0; r < cfg::AR; ++r) red[wave - half][r * 64 + lane] = acc[t][r];
                }
                __syncthreads();
                if (wave < half) {
#pragma unroll
                    for (int r = 0; r < cfg::AR; ++r) acc[t][r] += red[wave][r * 64 + lane];
                }
                __syncthreads();
            }
            if (wave == 0) {
#pragma unroll
                for (int r = 0; r < cfg::AR; ++r) {
                    const int row = cfg::SMALL ? 4 * (lane >> 4) + r : (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    mt[t][row * cfg::TD + col] = acc[t][r];
                }
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < nc * nc; e += 64 * cfg::NW) {
            const int p = e / nc, q = e - p * nc;
            if (q < p) continue;
            const float re = gram_m<CP>(mt, p, q) + gram_m<CP>(mt, CP + p, CP + q);
            const float im = p == q ? 0.f : gram_m<CP>(mt, CP + p, q) - gram_m<CP>(mt, p, CP + q);
            parts[j + ldp * (int64_t)(p * nc - p * (p - 1) / 2 + (q - p))] = make_float2(re, im);
        }
        __syncthreads();                                        // mt is rewritten by the next slab
    }
}

}  // namespace

int ig_coil_gram_c64(ig_ctx* ctx, int64_t n, int64_t nc, const void* x, int64_t ldx, int64_t slab, void* parts, int64_t ldp) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_coil_gram_c64: ctx is NULL");
    if (nc < 1 || nc > GRAM_MAXC)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_coil_gram_c64: %lld coils, between 1 and %d are supported", (long long)nc, GRAM_MAXC);
    if (n < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_coil_gram_c64: %lld samples, at least 1 is supported", (long long)n);
    if (slab < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_coil_gram_c64: a slab of %lld samples, at least 1 is supported", (long long)slab);
    const int64_t nslabs = (n + slab - 1) / slab, ntri = nc * (nc + 1) / 2;
    IG_REQUIRE(ctx, ldx >= n, "ig_coil_gram_c64: leading dimension %lld of x below n = %lld", (long long)ldx, (long long)n);
    IG_REQUIRE(ctx, ldp >= nslabs, "ig_coil_gram_c64: leading dimension %lld of parts below its %lld rows", (long long)ldp, (long long)nslabs);
    IG_REQUIRE(ctx, x && parts, "ig_coil_gram_c64: NULL pointer");
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (uintptr_t)((nc - 1) * ldx + n) * sizeof(float2);
    const uintptr_t p0 = (uintptr_t)parts, p1 = p0 + (uintptr_t)((ntri - 1) * ldp + nslabs) * sizeof(float2);
    IG_REQUIRE(ctx, !(x0 < p1 && p0 < x1), "ig_coil_gram_c64: parts overlaps x");
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, "coil_gram", 8.0 * ((double)n * (double)nc + (double)nslabs * (double)ntri));
    const dim3 grid((unsigned)(nslabs < GRAM_MAXGRID ? nslabs : GRAM_MAXGRID));
#define IG_GRAM_GO(CP) hipLaunchKernelGGL((k_coil_gram<CP>), grid, dim3(64 * gram_cfg<CP>::NW), 0, ctx->stream, n, (int)nc, (const float2*)x, ldx, slab, nslabs, (float2*)parts, ldp)
    if (nc <= 8) IG_GRAM_GO(8); else if (nc <= 16) IG_GRAM_GO(16); else if (nc <= 32) IG_GRAM_GO(32); else IG_GRAM_GO(64);
#undef IG_GRAM_GO
    IG_LAUNCH_CHECK(ctx, "k_coil_gram");
    return IG_OK;
}
