// Orthonormal periodic 3-D discrete wavelet transform and complex soft threshold of complex64 volumes
// (operators.Wavelet, Backend.dwt3 / soft_threshold).
//
// A column is an F-ordered n0 x n1 x n2 volume (axis 0 fastest).  One split of one axis of length d, for k < d/2:
//   low[k]  = sum_j h[j] v[(2k + j) mod d]      -> position k
//   high[k] = sum_j g[j] v[(2k + j) mod d]      -> position d/2 + k,      g[j] = (-1)^j h[TAPS-1-j]
// Level 1 splits the whole volume, level l+1 the low-pass corner box level l left; within a level the axes go 0, 1, 2,
// and an axis splits only while its current length is even and >= 2 TAPS.  The inverse runs the transposed passes in
// the reverse order (levels coarsest first, axes 2, 1, 0).
//
// k_dwt_lines does one split of one axis of the current box, one launch per (level, axis) that splits.  A workgroup owns
// whole lines: for axis 0 a few contiguous lines, for axes 1 and 2 a strip of 16 x-consecutive lines, so that every row of
// the strip is one 128-byte line of memory.  It stages its lines in LDS, waits, and only then writes low and high (or, inverse,
// the reconstructed samples) back -- in place when src == dst.  That is safe because every output of a line is computed
// after the whole line is in LDS, and no other workgroup reads or writes that line.
#include "ig_common.h"

namespace {

constexpr int DWT_BLK = 512;
constexpr int DWT_STRIP = 16;          // lines per workgroup along x for axes 1 and 2 (16 x 8 B = 128 B rows)
constexpr int DWT_MAXLEN = 1024;       // longest axis: a 16-line strip of 1024 samples is 128 KB of the 160 KB LDS
constexpr int DWT_AX0_ELEMS = 4096;    // axis 0: lines per workgroup = max(1, DWT_AX0_ELEMS / d)  (32 KB)
constexpr int MAXG = 65535;

// Daubechies minimum-phase low-pass filters (haar, db2, db4), compile-time constants
template <int TAPS>
__device__ __forceinline__ constexpr float lo(int j) {
    if constexpr (TAPS == 2) {
        constexpr float h[2] = {0.70710678118654752f, 0.70710678118654752f};
        return h[j];
    } else if constexpr (TAPS == 4) {
        constexpr float h[4] = {0.48296291314453416f, 0.8365163037378079f, 0.22414386804201339f, -0.12940952255126037f};
        return h[j];
    } else {
        constexpr float h[8] = {0.23037781330889645f, 0.7148465705529156f, 0.630880767929859f, -0.027983769416859594f,
                                -0.18703481171909306f, 0.03084138183556063f, 0.032883011666885176f, -0.010597401785069018f};
        return h[j];
    }
}
template <int TAPS>
__device__ __forceinline__ constexpr float hi(int j) { return (j & 1 ? -1.f : 1.f) * lo<TAPS>(TAPS - 1 - j); }

// One split of one axis for the lines (p, q), p < P, q < Q: line (p, q) starts at p * sp + q * sq and has d samples spaced s
// apart.  CONTIG (axis 0): s == 1, a workgroup takes W consecutive p, LDS holds line w at [w * d, (w + 1) * d).
// Otherwise (axes 1, 2): sp == 1, a workgroup takes a strip of W = DWT_STRIP consecutive p (x-consecutive lines), LDS holds
// sample k of line w at k * W + w, so that lanes w = 0..15 of a row read and write one 128-byte line of memory.
// grid.x: groups of W lines along p; grid.y strides over q; grid.z over columns.  dst = alpha * split(src).
template <int TAPS, bool INVERSE, bool CONTIG>
__global__ void __launch_bounds__(DWT_BLK)
k_dwt_lines(int d, int64_t s, int64_t P, int64_t sp, int64_t Q, int64_t sq, int W, int64_t ncols,
            const float2* src, int64_t lds_, float2* dst, int64_t ldd, float2 alpha) {
    extern __shared__ float2 line[];
    const int half = d / 2;
    const int64_t p0 = (int64_t)blockIdx.x * W;
    const int nw = (int)(P - p0 < W ? P - p0 : W);                // lines of this group
    const int lw = CONTIG ? d : 1, lk = CONTIG ? 1 : W;           // LDS strides of (line, sample)
    for (int64_t j = blockIdx.z; j < ncols; j += gridDim.z) {
        for (int64_t q = blockIdx.y; q < Q; q += gridDim.y) {
            const float2* sc = src + j * lds_ + q * sq + p0 * sp;
            float2* dc = dst + j * ldd + q * sq + p0 * sp;
            const int total = nw * d;
#pragma unroll 8
            for (int e = threadIdx.x; e < total; e += DWT_BLK) {
                const int w = CONTIG ? e / d : e % nw, k = CONTIG ? e % d : e / nw;
                line[w * lw + k * lk] = sc[w * sp + k * s];
            }
            __syncthreads();                                      // the whole line is staged: outputs may overwrite it in memory
            const int pairs = nw * half;
            for (int e = threadIdx.x; e < pairs; e += DWT_BLK) {
                const int w = CONTIG ? e / half : e % nw, k = CONTIG ? e % half : e / nw;
                const float2* lv = line + w * lw;
                float2* out = dc + w * sp;
                if (!INVERSE) {
                    // low[k], high[k] from v[(2k + j) mod d], j < TAPS
                    float2 a = make_float2(0.f, 0.f), b = make_float2(0.f, 0.f);
#pragma unroll
                    for (int t = 0; t < TAPS; ++t) {
                        int i = 2 * k + t;
                        i = i >= d ? i - d : i;
                        const float2 v = lv[i * lk];
                        a.x = fmaf(lo<TAPS>(t), v.x, a.x); a.y = fmaf(lo<TAPS>(t), v.y, a.y);
                        b.x = fmaf(hi<TAPS>(t), v.x, b.x); b.y = fmaf(hi<TAPS>(t), v.y, b.y);
                    }
                    out[(int64_t)k * s] = cmul(alpha, a);
                    out[(int64_t)(half + k) * s] = cmul(alpha, b);
                } else {
                    // v[2k + r] = sum_i h[2i + r] low[(k - i) mod d/2] + g[2i + r] high[(k - i) mod d/2],  r = 0, 1
                    float2 e0 = make_float2(0.f, 0.f), e1 = make_float2(0.f, 0.f);
#pragma unroll
                    for (int t = 0; t < TAPS / 2; ++t) {
                        int m = k - t;
                        m = m < 0 ? m + half : m;
                        const float2 l = lv[m * lk], h = lv[(half + m) * lk];
                        e0.x = fmaf(lo<TAPS>(2 * t), l.x, e0.x);     e0.y = fmaf(lo<TAPS>(2 * t), l.y, e0.y);
                        e0.x = fmaf(hi<TAPS>(2 * t), h.x, e0.x);     e0.y = fmaf(hi<TAPS>(2 * t), h.y, e0.y);
                        e1.x = fmaf(lo<TAPS>(2 * t + 1), l.x, e1.x); e1.y = fmaf(lo<TAPS>(2 * t + 1), l.y, e1.y);
                        e1.x = fmaf(hi<TAPS>(2 * t + 1), h.x, e1.x); e1.y = fmaf(hi<TAPS>(2 * t + 1), h.y, e1.y);
                    }
                    out[(int64_t)(2 * k) * s] = cmul(alpha, e0);
                    out[(int64_t)(2 * k + 1) * s] = cmul(alpha, e1);
                }
            }
            __syncthreads();                                      // LDS is reused by the next q / column
        }
    }
}

// y[:, j] = beta * y[:, j] + alpha * x[:, j] over n elements of ncols columns; READ_Y false: y is not read
template <bool READ_Y>
__global__ void __launch_bounds__(256)
k_dwt_combine(int64_t n, int64_t ncols, const float2* __restrict__ x, int64_t ldx, float2 a, float2 b,
              float2* __restrict__ y, int64_t ldy) {
    for (int64_t j = blockIdx.y; j < ncols; j += gridDim.y)
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
            float2 r = cmul(a, x[j * ldx + i]);
            if (READ_Y) cfma(r, b, y[j * ldy + i]);
            y[j * ldy + i] = r;
        }
}

// x <- x * max(0, 1 - tau / |x|) for every element outside the coarse box [0, c0) x [0, c1) x [0, c2); |x| <= tau gives
// exactly 0 (compared as |x|^2 <= tau^2, so that x = tau on an axis is a zero however the square root rounds).
__global__ void __launch_bounds__(256)
k_csoft(int64_t n0, int64_t n1, int64_t n, int64_t c0, int64_t c1, int64_t c2, int64_t ncols, float tau,
        float2* __restrict__ x, int64_t ldx) {
    const float tau2 = tau * tau;
    for (int64_t j = blockIdx.y; j < ncols; j += gridDim.y)
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
            const int64_t i0 = i % n0, r = i / n0, i1 = r % n1, i2 = r / n1;
            if (i0 < c0 && i1 < c1 && i2 < c2) continue;           // the coarse approximation band is kept
            float2* p = x + j * ldx + i;
            const float2 v = *p;
            const float r2 = v.x * v.x + v.y * v.y;
            if (r2 <= tau2) {
                *p = make_float2(0.f, 0.f);
            } else {
                const float f = 1.f - tau / sqrtf(r2);
                *p = make_float2(v.x * f, v.y * f);
            }
        }
}

int filter_taps(int wavelet) { return wavelet == 0 ? 2 : wavelet == 1 ? 4 : wavelet == 2 ? 8 : 0; }

struct split { int64_t c[3]; int axis; };                         // the box (before the split) and the axis split

// the forward passes in order; the coarse box left in `coarse`
std::vector<split> plan(const int64_t n[3], int taps, int levels, int64_t coarse[3]) {
    std::vector<split> out;
    int64_t c[3] = {n[0], n[1], n[2]};
    for (int l = 0; l < levels; ++l) {
        bool any = false;
        for (int a = 0; a < 3; ++a)
            if (c[a] % 2 == 0 && c[a] >= 2 * taps) {
                out.push_back(split{{c[0], c[1], c[2]}, a});
                c[a] /= 2;
                any = true;
            }
        if (!any) break;
    }
    for (int a = 0; a < 3; ++a) coarse[a] = c[a];
    return out;
}

template <int TAPS, bool INV>
int launch_split(ig_ctx* ctx, const split& sp, const int64_t n[3], int64_t ncols, const float2* src, int64_t lds_,
                 float2* dst, int64_t ldd, float2 alpha) {
    const int a = sp.axis;
    const int d = (int)sp.c[a];
    const int64_t stride[3] = {1, n[0], n[0] * n[1]};
    // lines (p, q): axis 0 -> (i1, i2); axis 1 -> (i0, i2); axis 2 -> (i0, i1)
    const int pa = a == 0 ? 1 : 0, qa = a == 2 ? 1 : 2;
    const int64_t P = sp.c[pa], Q = sp.c[qa];
    const int W = a == 0 ? (int)ig_clamp1(DWT_AX0_ELEMS / d, DWT_STRIP) : DWT_STRIP;
    const size_t lds = (size_t)W * d * sizeof(float2);
    const dim3 g((unsigned)((P + W - 1) / W), (unsigned)ig_clamp1(Q, MAXG), (unsigned)ig_clamp1(ncols, MAXG));
    ig_prof_scope prof(ctx, "dwt_lines", (double)sp.c[0] * sp.c[1] * sp.c[2] * ncols * 16.0);
    if (a == 0) {
        auto k = &k_dwt_lines<TAPS, INV, true>;
        if (lds > 65536) IG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, g, dim3(DWT_BLK), lds, ctx->stream, d, stride[a], P, stride[pa], Q, stride[qa], W, ncols,
                           src, lds_, dst, ldd, alpha);
    } else {
        auto k = &k_dwt_lines<TAPS, INV, false>;
        if (lds > 65536) IG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k, g, dim3(DWT_BLK), lds, ctx->stream, d, stride[a], P, stride[pa], Q, stride[qa], W, ncols,
                           src, lds_, dst, ldd, alpha);
    }
    IG_LAUNCH_CHECK(ctx, "k_dwt_lines");
    return IG_OK;
}

int combine(ig_ctx* ctx, int64_t n, int64_t ncols, const float2* x, int64_t ldx, float2 a, float2 b, float2* y, int64_t ldy,
            bool read_y) {
    const dim3 g((unsigned)ig_clamp1((n + 255) / 256, 4096), (unsigned)ig_clamp1(ncols, MAXG));
    ig_prof_scope prof(ctx, "dwt_combine", (double)n * ncols * 8.0 * (read_y ? 3 : 2));
    if (read_y) hipLaunchKernelGGL(k_dwt_combine<true>, g, dim3(256), 0, ctx->stream, n, ncols, x, ldx, a, b, y, ldy);
    else        hipLaunchKernelGGL(k_dwt_combine<false>, g, dim3(256), 0, ctx->stream, n, ncols, x, ldx, a, b, y, ldy);
    IG_LAUNCH_CHECK(ctx, "k_dwt_combine");
    return IG_OK;
}

// dst = alpha * W src (or W^H): src == dst is in place.  The first forward pass covers the whole volume, so it reads src and
// writes dst; the inverse's first pass covers only the coarse box, so the inverse copies src to dst first.
template <int TAPS>
int transform(ig_ctx* ctx, const int64_t n[3], int levels, bool inverse, int64_t ncols, const float2* src, int64_t lds_,
              float2* dst, int64_t ldd, float2 alpha) {
    int64_t coarse[3];
    const std::vector<split> passes = plan(n, TAPS, levels, coarse);
    const int64_t vol = n[0] * n[1] * n[2];
    const float2 one = make_float2(1.f, 0.f);
    if (passes.empty() || inverse) {
        if (src != dst || alpha.x != 1.f || alpha.y != 0.f)
            if (int rc = combine(ctx, vol, ncols, src, lds_, alpha, make_float2(0.f, 0.f), dst, ldd, false)) return rc;
        for (size_t i = passes.size(); i-- > 0;)
            if (int rc = launch_split<TAPS, true>(ctx, passes[i], n, ncols, dst, ldd, dst, ldd, one)) return rc;
        return IG_OK;
    }
    for (size_t i = 0; i < passes.size(); ++i) {
        const bool first = i == 0;
        if (int rc = launch_split<TAPS, false>(ctx, passes[i], n, ncols, first ? src : dst, first ? lds_ : ldd, dst, ldd,
                                               first ? alpha : one)) return rc;
    }
    return IG_OK;
}

int transform_any(ig_ctx* ctx, int taps, const int64_t n[3], int levels, bool inverse, int64_t ncols, const float2* src,
                  int64_t lds_, float2* dst, int64_t ldd, float2 alpha) {
    if (taps == 2) return transform<2>(ctx, n, levels, inverse, ncols, src, lds_, dst, ldd, alpha);
    if (taps == 4) return transform<4>(ctx, n, levels, inverse, ncols, src, lds_, dst, ldd, alpha);
    return transform<8>(ctx, n, levels, inverse, ncols, src, lds_, dst, ldd, alpha);
}

}  // namespace

int ig_dwt3_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int wavelet, int levels, int inverse, int64_t ncols,
                const void* x, int64_t ldx, float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_dwt3_c64: ctx is NULL");
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && ncols >= 0 && levels >= 0, "ig_dwt3_c64: negative dimension or level count");
    IG_REQUIRE(ctx, n0 <= DWT_MAXLEN && n1 <= DWT_MAXLEN && n2 <= DWT_MAXLEN,
               "ig_dwt3_c64: axis longer than %d in %lld x %lld x %lld", DWT_MAXLEN, (long long)n0, (long long)n1, (long long)n2);
    const int taps = filter_taps(wavelet);
    IG_REQUIRE(ctx, taps > 0, "ig_dwt3_c64: unknown wavelet %d (0 haar, 1 db2, 2 db4)", wavelet);
    const int64_t vol = n0 * n1 * n2;
    IG_REQUIRE(ctx, ldx >= vol && ldy >= vol, "ig_dwt3_c64: leading dimension (%lld, %lld) below the volume %lld",
               (long long)ldx, (long long)ldy, (long long)vol);
    if (vol == 0 || ncols == 0) return IG_OK;
    IG_REQUIRE(ctx, x && y, "ig_dwt3_c64: NULL pointer");
    const bool b0 = (br == 0.f && bi == 0.f);
    IG_REQUIRE(ctx, b0 || x != y, "ig_dwt3_c64: beta != 0 needs y distinct from x");
    IG_REQUIRE(ctx, x != y || ldx == ldy, "ig_dwt3_c64: in place with different leading dimensions");
    IG_REQUIRE(ctx, x == y || !ig_panels_overlap(x, ldx, vol, ncols, y, ldy, vol, ncols),
               "ig_dwt3_c64: y overlaps x (y == x with ldy == ldx is the in-place form)");
    if (int rc = ig_set_device(ctx)) return rc;
    const int64_t n[3] = {n0, n1, n2};
    const float2 a = make_float2(ar, ai), one = make_float2(1.f, 0.f);
    const float2* xp = (const float2*)x;
    float2* yp = (float2*)y;
    if (b0) return transform_any(ctx, taps, n, levels, inverse != 0, ncols, xp, ldx, yp, ldy, a);
    // y = beta y + alpha T x = T (beta T^H y + alpha x) for the orthogonal T: no scratch panel, three passes over y
    if (int rc = transform_any(ctx, taps, n, levels, inverse == 0, ncols, yp, ldy, yp, ldy, one)) return rc;
    if (int rc = combine(ctx, vol, ncols, xp, ldx, a, make_float2(br, bi), yp, ldy, true)) return rc;
    return transform_any(ctx, taps, n, levels, inverse != 0, ncols, yp, ldy, yp, ldy, one);
}

int ig_csoft_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t c0, int64_t c1, int64_t c2, int64_t ncols,
                 float tau, void* x, int64_t ldx) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_csoft_c64: ctx is NULL");
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && ncols >= 0 && c0 >= 0 && c1 >= 0 && c2 >= 0,
               "ig_csoft_c64: negative dimension");
    IG_REQUIRE(ctx, tau >= 0.f, "ig_csoft_c64: negative threshold %g", (double)tau);
    const int64_t vol = n0 * n1 * n2;
    IG_REQUIRE(ctx, ldx >= vol, "ig_csoft_c64: leading dimension %lld below the volume %lld", (long long)ldx, (long long)vol);
    if (vol == 0 || ncols == 0) return IG_OK;
    IG_REQUIRE(ctx, x != nullptr, "ig_csoft_c64: x is NULL");
    if (int rc = ig_set_device(ctx)) return rc;
    const dim3 g((unsigned)ig_clamp1((vol + 255) / 256, 4096), (unsigned)ig_clamp1(ncols, MAXG));
    ig_prof_scope prof(ctx, "csoft", (double)vol * ncols * 16.0);
    hipLaunchKernelGGL(k_csoft, g, dim3(256), 0, ctx->stream, n0, n1, vol, c0, c1, c2, ncols, tau, (float2*)x, ldx);
    IG_LAUNCH_CHECK(ctx, "k_csoft");
    return IG_OK;
}
