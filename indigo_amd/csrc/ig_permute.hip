// Batched 3-D axis permutation of complex64 volumes (operators.AxisPermute):
//   y[:, j] = beta * y[:, j] + alpha * permute(x[:, j]),   output axis a = input axis perm[a]
// Column j of x is an F-ordered n0 x n1 x n2 volume (x fastest).  Two kernels, both pure HBM streams:
//   perm[0] == 0   input x stays the fastest axis: rows of n0 elements are moved whole, 16 bytes per lane where
//                  the rows allow it (even n0, 16-byte aligned columns), 8 bytes otherwise;
//   perm[0] != 0   a 32 x 32 LDS tile transposes input axis 0 against input axis perm[0], looping over the third axis:
//                  lanes read along input x and write along output x (both coalesced, 256 bytes per half-wave row).
//                  Tile rows are padded by one element: a column read of 8-byte elements then touches 32 distinct
//                  bank pairs per 32-lane group (no conflict).
#include "ig_common.h"

namespace {

constexpr int PT = 32;          // tile edge (elements)
constexpr int PR = 8;           // tile rows per pass of a 256-lane block (PT x PR lanes)
constexpr int BLK = PT * PR;
constexpr int MAXY = 65535;     // grid.y / grid.z cap (the kernels stride over what does not fit)

// MODE 0: y = x (alpha == 1, beta == 0: a bit-exact copy)   MODE 1: y = alpha x   MODE 2: y = beta y + alpha x
template <int MODE>
__device__ __forceinline__ float2 combine(float2 v, const float2* yp, float2 a, float2 b) {
    if (MODE == 0) return v;
    float2 r = cmul(a, v);
    if (MODE == 2) cfma(r, b, *yp);
    return r;
}

// perm[0] == 0.  Output row r = o1 + m1 * o2 (m1 = n[perm[1]]) takes input row o1 * sin1 + o2 * sin2 (in elements, a multiple
// of n0).  Block: 64 lanes along the row x 4 rows; grid.y strides over output rows, grid.z over columns.
template <int MODE, bool VEC>
__global__ void __launch_bounds__(BLK)
k_permute_rows(int64_t n0, int64_t nrows, int64_t m1, int64_t sin1, int64_t sin2, int64_t ncols,
               const float2* __restrict__ x, int64_t ldx, float2 a, float2 b, float2* __restrict__ y, int64_t ldy) {
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int64_t j = blockIdx.z; j < ncols; j += gridDim.z) {
        const float2* xc = x + j * ldx;
        float2* yc = y + j * ldy;
        for (int64_t r = (int64_t)blockIdx.y * 4 + ty; r < nrows; r += (int64_t)gridDim.y * 4) {
            const int64_t o1 = r % m1, o2 = r / m1;
            const float2* xr = xc + o1 * sin1 + o2 * sin2;
            float2* yr = yc + r * n0;
            if (VEC) {
                const float4* x4 = reinterpret_cast<const float4*>(xr);
                float4* y4 = reinterpret_cast<float4*>(yr);
                for (int64_t e = (int64_t)blockIdx.x * 64 + tx; e < n0 / 2; e += (int64_t)gridDim.x * 64) {
                    const float4 v = x4[e];
                    if (MODE == 0) { y4[e] = v; continue; }
                    float2 yv[2];
                    if (MODE == 2) { const float4 w = y4[e]; yv[0] = make_float2(w.x, w.y); yv[1] = make_float2(w.z, w.w); }
                    const float2 r0 = combine<MODE>(make_float2(v.x, v.y), &yv[0], a, b);
                    const float2 r1 = combine<MODE>(make_float2(v.z, v.w), &yv[1], a, b);
                    y4[e] = make_float4(r0.x, r0.y, r1.x, r1.y);
                }
            } else {
                for (int64_t e = (int64_t)blockIdx.x * 64 + tx; e < n0; e += (int64_t)gridDim.x * 64)
                    yr[e] = combine<MODE>(xr[e], yr + e, a, b);
            }
        }
    }
}

// perm[0] = A != 0: a PT x PT tile of (input axis 0, input axis A) at one index of the third input axis B.
// Input strides (1, sA, sB); output strides (o0, 1, oB) of input axes (0, A, B).  grid.x = tiles of axis 0 x tiles of axis A,
// grid.y strides over axis B, grid.z over columns.
template <int MODE>
__global__ void __launch_bounds__(BLK)
k_permute_tile(int64_t n0, int64_t nA, int64_t nB, int64_t sA, int64_t sB, int64_t o0, int64_t oB, int64_t tiles0, int64_t ncols,
               const float2* __restrict__ x, int64_t ldx, float2 a, float2 b, float2* __restrict__ y, int64_t ldy) {
    __shared__ float2 tile[PT][PT + 1];
    const int tx = threadIdx.x % PT, ty = threadIdx.x / PT;
    const int64_t i0b = (int64_t)(blockIdx.x % tiles0) * PT;
    const int64_t iAb = (int64_t)(blockIdx.x / tiles0) * PT;
    for (int64_t j = blockIdx.z; j < ncols; j += gridDim.z) {
        const float2* xc = x + j * ldx;
        float2* yc = y + j * ldy;
        for (int64_t iB = blockIdx.y; iB < nB; iB += gridDim.y) {
            // read: lanes along input axis 0
            const int64_t i0 = i0b + tx;
#pragma unroll
            for (int k = 0; k < PT; k += PR) {
                const int64_t iA = iAb + ty + k;
                if (i0 < n0 && iA < nA) tile[ty + k][tx] = xc[i0 + iA * sA + iB * sB];
            }
            __syncthreads();
            // write: lanes along input axis A = output axis 0
            const int64_t iA = iAb + tx;
#pragma unroll
            for (int k = 0; k < PT; k += PR) {
                const int64_t i0w = i0b + ty + k;
                if (iA < nA && i0w < n0) {
                    float2* yp = yc + iA + i0w * o0 + iB * oB;
                    *yp = combine<MODE>(tile[tx][ty + k], yp, a, b);
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace

int ig_permute3_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, const int perm[3], int64_t ncols,
                    const void* x, int64_t ldx, float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_permute3_c64: ctx is NULL");
    IG_REQUIRE(ctx, perm != nullptr, "ig_permute3_c64: perm is NULL");
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && ncols >= 0, "ig_permute3_c64: negative dimension");
    const int p0 = perm[0], p1 = perm[1], p2 = perm[2];
    IG_REQUIRE(ctx, p0 >= 0 && p0 < 3 && p1 >= 0 && p1 < 3 && p2 >= 0 && p2 < 3 && p0 != p1 && p0 != p2 && p1 != p2,
               "ig_permute3_c64: perm (%d, %d, %d) is no permutation of (0, 1, 2)", p0, p1, p2);
    const int64_t vol = n0 * n1 * n2;
    IG_REQUIRE(ctx, ldx >= vol && ldy >= vol, "ig_permute3_c64: leading dimension (%lld, %lld) below the volume %lld",
               (long long)ldx, (long long)ldy, (long long)vol);
    if (vol == 0 || ncols == 0) return IG_OK;
    IG_REQUIRE(ctx, x && y, "ig_permute3_c64: NULL pointer");
    IG_REQUIRE(ctx, x != y, "ig_permute3_c64: x and y are the same array (no in-place permutation)");
    if (int rc = ig_set_device(ctx)) return rc;

    const int64_t n[3] = {n0, n1, n2};
    const int64_t sin[3] = {1, n0, n0 * n1};                            // input strides
    const int64_t m0 = n[p0], m1 = n[p1];
    int64_t sout[3];                                                    // output stride of each INPUT axis
    sout[p0] = 1; sout[p1] = m0; sout[p2] = m0 * m1;

    const bool b0 = (br == 0.f && bi == 0.f);
    const int mode = b0 ? ((ar == 1.f && ai == 0.f) ? 0 : 1) : 2;
    const float2 a = make_float2(ar, ai), b = make_float2(br, bi);
    ig_prof_scope prof(ctx, "permute3", (double)vol * ncols * 8.0 * (b0 ? 2 : 3));
    const int64_t gz = ig_clamp1(ncols, MAXY);

    if (p0 == 0) {
        const int64_t nrows = n1 * n2;
        const bool vec = n0 % 2 == 0 && ldx % 2 == 0 && ldy % 2 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0;
        const int64_t per_row = vec ? n0 / 2 : n0;
        // enough blocks for ~8 per CU over all columns; long rows split over grid.x
        const int64_t gx = ig_clamp1((per_row + 63) / 64, 64);
        const int64_t gy = ig_clamp1((nrows + 3) / 4, MAXY);
        const dim3 g((unsigned)gx, (unsigned)gy, (unsigned)gz);
#define IG_PERM_ROWS(M_, V_) hipLaunchKernelGGL((k_permute_rows<M_, V_>), g, dim3(BLK), 0, ctx->stream, n0, nrows, m1, sin[p1], sin[p2], ncols, \
                                                (const float2*)x, ldx, a, b, (float2*)y, ldy)
        if (vec) { if (mode == 0) IG_PERM_ROWS(0, true); else if (mode == 1) IG_PERM_ROWS(1, true); else IG_PERM_ROWS(2, true); }
        else     { if (mode == 0) IG_PERM_ROWS(0, false); else if (mode == 1) IG_PERM_ROWS(1, false); else IG_PERM_ROWS(2, false); }
#undef IG_PERM_ROWS
        IG_LAUNCH_CHECK(ctx, "k_permute_rows");
        return IG_OK;
    }

    const int A = p0, B = 3 - p0;                                       // {A, B} = {1, 2}
    const int64_t tiles0 = (n0 + PT - 1) / PT, tilesA = (n[A] + PT - 1) / PT;
    IG_REQUIRE(ctx, tiles0 * tilesA <= INT32_MAX, "ig_permute3_c64: %lld x %lld tiles do not fit one grid axis",
               (long long)tiles0, (long long)tilesA);
    const dim3 g((unsigned)(tiles0 * tilesA), (unsigned)ig_clamp1(n[B], MAXY), (unsigned)gz);
#define IG_PERM_TILE(M_) hipLaunchKernelGGL((k_permute_tile<M_>), g, dim3(BLK), 0, ctx->stream, n0, n[A], n[B], sin[A], sin[B], sout[0], sout[B], \
                                            tiles0, ncols, (const float2*)x, ldx, a, b, (float2*)y, ldy)
    if (mode == 0) IG_PERM_TILE(0); else if (mode == 1) IG_PERM_TILE(1); else IG_PERM_TILE(2);
#undef IG_PERM_TILE
    IG_LAUNCH_CHECK(ctx, "k_permute_tile");
    return IG_OK;
}
