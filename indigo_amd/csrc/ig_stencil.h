// The lane layout and the voxel loop of the streaming stencils on F-ordered n0 x n1 x n2 volumes: the total-variation kernels
// (ig_tv.hip) and the total-generalized-variation kernels (ig_tgv.hip, §3.20).  A workgroup owns 256 / LX
// x-contiguous rows, LX = 8 .. 64 lanes along x (the smallest power of two that covers n0); grid.x strides along the row, grid.y
// over groups of rows, grid.z over columns.  Each unit gets its own copy (an unnamed namespace).
#pragma once
#include "ig_common.h"

namespace {

constexpr int TV_BLK = 256;
constexpr int TV_MAXROWS = 2048;       // grid.y cap: with grid.x that is a few workgroups per CU in flight, the rest strides
constexpr int MAXG = 65535;

struct tv_dims { int64_t n0, n1, n2, vol; int lx_log2; };

// the voxel loop shared by the kernels: body(column j, i0, i1, i2, voxel index i)
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

inline tv_dims make_dims(int64_t n0, int64_t n1, int64_t n2) {
    int l = 3;
    while (l < 6 && (int64_t(1) << l) < n0) ++l;
    return tv_dims{n0, n1, n2, n0 * n1 * n2, l};
}

inline dim3 make_grid(const tv_dims& d, int64_t ncols) {
    const int64_t lx = int64_t(1) << d.lx_log2, rows = TV_BLK / lx;
    return dim3((unsigned)ig_clamp1((d.n0 + lx - 1) / lx, 64), (unsigned)ig_clamp1((d.n1 * d.n2 + rows - 1) / rows, TV_MAXROWS),
                (unsigned)ig_clamp1(ncols, MAXG));
}

}  // namespace
