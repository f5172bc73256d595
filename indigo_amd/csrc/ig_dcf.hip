// Density compensation (indigo_amd.dcf, Backend.dcf_spread / dcf_gather_div / row_scale, pics --dcf): the two
// halves of one Pipe-Menon iteration  w <- w / (G G^H w)  on ONE real column, and the diagonal of the weighted data term.
//
// Both halves compute their taps from the separable records of ig_interp3_sep (built without modulation and with scale 1: plain
// positive weights).  A tap is the float32 product (w1 * w2) * w0 -- two roundings, no fused multiply-add -- exactly as
// interp.sep_expand forms it.
//
//   spread   acc[cell] += rint(tap * w[i] * scale)   in 64-bit integers.  tap * w[i] is exact in double (24 + 24 bits), scale is a
//            power of two, so a contribution carries ONE rounding, of at most half a quantum, and integer addition is associative:
//            the result does not depend on the order in which the adds arrive, whatever route they take.  The samples come binned by
//            the 16 x 8 x 8 tile of the grid their (wrapped) first tap lies in (grid_formats.dcf_tiles); one workgroup per non-empty
//            tile.  A tile of at least lds_min samples sums into an LDS image of the tile plus a halo of tw - 1 cells per axis
//            (ds_add_u64) and adds the image's non-zero cells to the grid, modulo its dimensions, with global 64-bit atomics; a
//            tile below lds_min adds straight to the grid.  A wave takes one sample at a time, its lanes the sample's taps: the adds
//            of one wave instruction go to distinct cells.
//   gather   s = sum tap * (double)acc[cell] / scale in double (lanes over the taps, a butterfly over the wave), w_out = w / s
//            rounded once to float, and the maxima of w_out and |s - 1| through atomicMax on the float bit patterns (non-negative
//            values: the bits order like the numbers).
#include "ig_common.h"

namespace {

constexpr int DCF_BLK = 256;                    // four waves
constexpr int DCF_WAVES = DCF_BLK / 64;
constexpr int DCF_T0 = 16, DCF_T1 = 8, DCF_T2 = 8;      // the tile, in cells of axis 0 / 1 / 2
constexpr int DCF_SPW = 8;                      // samples a wave of the gather takes at once
constexpr int DCF_GROUPS = 8;                   // ... and how many times it does so: 256 samples per workgroup

typedef unsigned long long u64;

// a sample's record in the lanes of a wave: lane l < 3 TW + 2 holds word l (every lane of the wave calls these)
struct dcf_rec {
    int j0, j1, j2, c0, c1, c2;
};
// the words of sample i; a sample number beyond M (a caller's mistake) reads nothing and gives a record without taps
template <int TW>
__device__ __forceinline__ uint32_t dcf_words(const uint32_t* __restrict__ records, int64_t rec_stride, int64_t M, uint32_t i, int lane) {
    return (lane < 3 * TW + 2 && (int64_t)i < M) ? records[(int64_t)i * rec_stride + lane] : 0u;
}
template <int TW>
__device__ __forceinline__ dcf_rec dcf_head(uint32_t word) {
    const uint32_t h0 = (uint32_t)__shfl((int)word, 3 * TW), h1 = (uint32_t)__shfl((int)word, 3 * TW + 1);
    dcf_rec r;
    r.j0 = (int)(h0 & 0xffffu); r.j1 = (int)(h0 >> 16); r.j2 = (int)(h1 & 0xffffu);
    r.c0 = (int)((h1 >> 16) & 15u); r.c1 = (int)((h1 >> 20) & 15u); r.c2 = (int)((h1 >> 24) & 15u);
    return r;
}
// tap t = a + TW (b + TW c) of the record whose words the wave's lanes hold
template <int TW>
__device__ __forceinline__ float dcf_tap(uint32_t word, int t, int& a, int& b, int& c) {
    a = t % TW; b = (t / TW) % TW; c = t / (TW * TW);
    const int cc = c < TW ? c : TW - 1;                                  // (lanes beyond the last tap read a valid lane)
    const float w0 = __uint_as_float((uint32_t)__shfl((int)word, a));
    const float w1 = __uint_as_float((uint32_t)__shfl((int)word, TW + b));
    const float w2 = __uint_as_float((uint32_t)__shfl((int)word, 2 * TW + cc));
    return __fmul_rn(__fmul_rn(w1, w2), w0);
}

// One workgroup per entry of (tile_ptr, tile_ids): a tile, or a piece of a heavy one.  A wave takes every fourth sample of the piece,
// 64 of them per batch: their numbers with one load (lane l: the wave's l-th sample of the batch), and the record and weight of the
// next sample while the taps of the current one are added -- a sample costs no memory latency of its own.
template <int TW>
__global__ void __launch_bounds__(DCF_BLK)
k_dcf_spread(int64_t M, const uint32_t* __restrict__ records, int64_t rec_stride, const uint32_t* __restrict__ order,
             const int64_t* __restrict__ tile_ptr, const int32_t* __restrict__ tile_ids, const float* __restrict__ w, double scale,
             int64_t lds_min, u64* __restrict__ acc, int n0, int nm, int ns) {
    constexpr int L0 = DCF_T0 + TW - 1, L1 = DCF_T1 + TW - 1, L2 = DCF_T2 + TW - 1, LN = L0 * L1 * L2;
    constexpr int NT = TW * TW * TW, ROUNDS = (NT + 63) / 64;
    __shared__ u64 img[LN];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // (pointers, tile ids and sample numbers are the caller's: whatever they hold, nothing outside the arrays is touched)
    const int64_t lo = max((int64_t)0, tile_ptr[blockIdx.x]), hi = min(M, tile_ptr[blockIdx.x + 1]);
    const int tile = tile_ids[blockIdx.x] & 0x7fffffff;
    const int nt0 = (n0 + DCF_T0 - 1) / DCF_T0, nt1 = (nm + DCF_T1 - 1) / DCF_T1, nt2 = (ns + DCF_T2 - 1) / DCF_T2;
    const int o0 = (tile % nt0) * DCF_T0, o1 = ((tile / nt0) % nt1) * DCF_T1, o2 = ((tile / (nt0 * nt1)) % nt2) * DCF_T2;
    const bool dense = hi - lo >= lds_min;                                 // (block-uniform)
    if (dense) {
        for (int k = threadIdx.x; k < LN; k += DCF_BLK) img[k] = 0ull;
        __syncthreads();
    }
    for (int64_t base = lo + wave; base < hi; base += 64 * DCF_WAVES) {
        const int64_t left = (hi - base + DCF_WAVES - 1) / DCF_WAVES;     // the wave's samples from here on
        const int cnt = left < 64 ? (int)left : 64;
        const uint32_t mine = lane < cnt ? order[base + (int64_t)DCF_WAVES * lane] : 0xffffffffu;
        uint32_t i_next = (uint32_t)__shfl((int)mine, 0);
        uint32_t word_next = dcf_words<TW>(records, rec_stride, M, i_next, lane);
        float w_next = (int64_t)i_next < M ? w[i_next] : 0.f;
        for (int k = 0; k < cnt; ++k) {
            const uint32_t word = word_next;
            const double wi = (double)w_next * scale;                     // (a power of two: exact)
            if (k + 1 < cnt) {
                i_next = (uint32_t)__shfl((int)mine, k + 1);
                word_next = dcf_words<TW>(records, rec_stride, M, i_next, lane);
                w_next = (int64_t)i_next < M ? w[i_next] : 0.f;
            }
            const dcf_rec r = dcf_head<TW>(word);
            // a sample whose first tap is not in this tile takes the direct route: the same bits
            const bool local = dense && (unsigned)(r.j0 - o0) < (unsigned)DCF_T0 && (unsigned)(r.j1 - o1) < (unsigned)DCF_T1 &&
                               (unsigned)(r.j2 - o2) < (unsigned)DCF_T2;
#pragma unroll
            for (int q4 = 0; q4 < ROUNDS; ++q4) {
                int a, b, c;
                const float tap = dcf_tap<TW>(word, lane + 64 * q4, a, b, c);
                if (a < r.c0 && b < r.c1 && c < r.c2) {
                    const u64 q = (u64)__double2ll_rn((double)tap * wi);
                    if (local) {
                        atomicAdd(&img[(r.j0 - o0 + a) + L0 * ((r.j1 - o1 + b) + L1 * (r.j2 - o2 + c))], q);
                    } else {
                        int g0 = r.j0 + a, g1 = r.j1 + b, g2 = r.j2 + c;  // (first taps are wrapped and every axis holds >= TW cells)
                        g0 -= g0 >= n0 ? n0 : 0; g1 -= g1 >= nm ? nm : 0; g2 -= g2 >= ns ? ns : 0;
                        if (g0 < n0 && g1 < nm && g2 < ns)
                            atomicAdd(acc + ((int64_t)g0 + (int64_t)n0 * ((int64_t)g1 + (int64_t)nm * g2)), q);
                    }
                }
            }
        }
    }
    if (dense) {
        __syncthreads();
        // the image's rows, one after the other; a zero cell adds nothing
        for (int k = threadIdx.x; k < LN; k += DCF_BLK) {
            const u64 q = img[k];
            if (q != 0ull) {
                const int g0 = (o0 + k % L0) % n0, g1 = (o1 + (k / L0) % L1) % nm, g2 = (o2 + k / (L0 * L1)) % ns;
                atomicAdd(acc + ((int64_t)g0 + (int64_t)n0 * ((int64_t)g1 + (int64_t)nm * g2)), q);
            }
        }
    }
}

// A wave takes DCF_SPW consecutive samples of `order` at once: their numbers with one load, their records with DCF_SPW independent
// loads, the cells of all of them before any sum is reduced -- three memory latencies per wave, not per sample --, then lane l
// divides and stores for the l-th sample.  The two maxima are reduced over the workgroup's 256 samples first, and the two words are
// only raised by a workgroup that finds them below its own values (an agent-scope load first): every workgroup adding to the same
// two addresses is the contention case -- 2^21 waves' atomics on one address took 45 of the kernel's 48 ms.
template <int TW>
__global__ void __launch_bounds__(DCF_BLK)
k_dcf_gather_div(int64_t M, const uint32_t* __restrict__ records, int64_t rec_stride, const uint32_t* __restrict__ order,
                 const long long* __restrict__ acc, int n0, int nm, int ns, double inv_scale, const float* w, float* w_out,
                 float* s_out, unsigned* maxima) {
    constexpr int NT = TW * TW * TW, ROUNDS = (NT + 63) / 64;
    __shared__ float red[2][DCF_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float wmax = 0.f, dmax = 0.f;
    for (int g = 0; g < DCF_GROUPS; ++g) {
    const int64_t first = (((int64_t)blockIdx.x * DCF_GROUPS + g) * DCF_WAVES + wave) * DCF_SPW;
    if (first >= M) break;                                                // (wave-uniform)
    const uint32_t mine = (lane < DCF_SPW && first + lane < M) ? order[first + lane] : 0xffffffffu;
    const bool live = (int64_t)mine < M;
    const float wi = live ? w[mine] : 0.f;                                // (w_out may be w: read before the store)
    uint32_t word[DCF_SPW];
#pragma unroll
    for (int k = 0; k < DCF_SPW; ++k) word[k] = dcf_words<TW>(records, rec_stride, M, (uint32_t)__shfl((int)mine, k), lane);
    double s[DCF_SPW];
#pragma unroll
    for (int k = 0; k < DCF_SPW; ++k) {
        const dcf_rec r = dcf_head<TW>(word[k]);
        s[k] = 0.0;
#pragma unroll
        for (int q4 = 0; q4 < ROUNDS; ++q4) {
            int a, b, c;
            const float tap = dcf_tap<TW>(word[k], lane + 64 * q4, a, b, c);
            if (a < r.c0 && b < r.c1 && c < r.c2) {
                int g0 = r.j0 + a, g1 = r.j1 + b, g2 = r.j2 + c;
                g0 -= g0 >= n0 ? n0 : 0; g1 -= g1 >= nm ? nm : 0; g2 -= g2 >= ns ? ns : 0;
                if (g0 < n0 && g1 < nm && g2 < ns)
                    s[k] += (double)tap * (double)acc[(int64_t)g0 + (int64_t)n0 * ((int64_t)g1 + (int64_t)nm * g2)];
            }
        }
    }
    double sl = 0.0;
#pragma unroll
    for (int k = 0; k < DCF_SPW; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s[k] += __shfl_xor(s[k], d);
        if (lane == k) sl = s[k];
    }
    sl *= inv_scale;
    float q = 0.f, dev = 0.f;
    if (live) {
        q = sl == 0.0 ? 0.f : (float)((double)wi / sl);
        dev = (float)fabs(sl - 1.0);
        w_out[mine] = q;
        if (s_out) s_out[mine] = (float)sl;
    }
#pragma unroll
    for (int d = DCF_SPW / 2; d >= 1; d >>= 1) {
        q = fmaxf(q, __shfl_xor(q, d));
        dev = fmaxf(dev, __shfl_xor(dev, d));
    }
    wmax = fmaxf(wmax, q);
    dmax = fmaxf(dmax, dev);
    }
    if (lane == 0) { red[0][wave] = wmax; red[1][wave] = dmax; }
    __syncthreads();
    if (threadIdx.x < 2) {
        float v = red[threadIdx.x][0];
#pragma unroll
        for (int k = 1; k < DCF_WAVES; ++k) v = fmaxf(v, red[threadIdx.x][k]);
        const unsigned bits = __float_as_uint(v);
        // (the words only grow during the kernel: a value read now is a lower bound of the final one)
        if (bits > __hip_atomic_load(maxima + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(maxima + threadIdx.x, bits);
    }
}

// Y[i, c] = w[i] * X[i, c]: V rows per thread (V == 2: 16-byte accesses), the weight loaded once for all columns.  Y may be X.
template <int V>
__global__ void __launch_bounds__(DCF_BLK)
k_rowscale(int64_t nv, int64_t ncols, const float* __restrict__ w, const float2* x, int64_t ldx, float2* y, int64_t ldy) {
    for (int64_t it = (int64_t)blockIdx.x * DCF_BLK + threadIdx.x; it < nv; it += (int64_t)gridDim.x * DCF_BLK) {
        float s[V];
        if constexpr (V == 2) { const float2 q = *reinterpret_cast<const float2*>(w + 2 * it); s[0] = q.x; s[1] = q.y; }
        else s[0] = w[it];
        for (int64_t c = 0; c < ncols; ++c) {
            float2 v[V];
            ldv<V>(v, x + it * V + c * ldx);
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = make_float2(s[k] * v[k].x, s[k] * v[k].y);
            stv<V>(y + it * V + c * ldy, v);
        }
    }
}

int dcf_check(ig_ctx* ctx, const char* what, int64_t M, int tw, const void* records, int64_t rec_stride, const void* order,
              int64_t n0, int64_t nm, int64_t ns, double scale) {
    if (tw != 4 && tw != 6 && tw != 8)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "%s: %d taps per axis, 4, 6 and 8 are supported", what, tw);
    if (M < 0 || M >= ((int64_t)1 << 32))
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "%s: %lld samples, fewer than 2^32 are supported (32-bit sample order)", what, (long long)M);
    if (n0 < tw || nm < tw || ns < tw || n0 > 65535 || nm > 65535 || ns > 65535)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "%s: grid %lld x %lld x %lld, every axis must hold between %d and 65535 cells", what,
                       (long long)n0, (long long)nm, (long long)ns, tw);
    IG_REQUIRE(ctx, rec_stride >= ig_interp3_sep_words(tw), "%s: rec_stride %lld below the %d words of a record", what,
               (long long)rec_stride, ig_interp3_sep_words(tw));
    IG_REQUIRE(ctx, M == 0 || (records && order), "%s: NULL pointer", what);
    int e = 0;
    const double m = frexp(scale, &e);
    IG_REQUIRE(ctx, scale > 0 && m == 0.5, "%s: scale %g is no positive power of two", what, scale);
    return IG_OK;
}

}  // namespace

int ig_dcf_spread_r32(ig_ctx* ctx, int64_t M, int tw, const uint32_t* records, int64_t rec_stride, const uint32_t* order,
                      const int64_t* tile_ptr, const int32_t* tile_ids, int64_t ntiles, const float* w, double scale, int64_t lds_min,
                      int64_t* acc, int64_t n0, int64_t nm, int64_t ns) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_dcf_spread_r32: ctx is NULL");
    if (int rc = dcf_check(ctx, "ig_dcf_spread_r32", M, tw, records, rec_stride, order, n0, nm, ns, scale)) return rc;
    IG_REQUIRE(ctx, acc != nullptr && (M == 0 || w != nullptr), "ig_dcf_spread_r32: NULL pointer");
    IG_REQUIRE(ctx, ntiles >= 0 && ntiles <= M && (ntiles == 0 || (tile_ptr && tile_ids)), "ig_dcf_spread_r32: %lld tiles for %lld samples",
               (long long)ntiles, (long long)M);
    if (ntiles > 0x7fffffff)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_dcf_spread_r32: %lld tiles exceed one launch", (long long)ntiles);
    if (int rc = ig_set_device(ctx)) return rc;
    const int64_t cells = n0 * nm * ns;
    IG_HIP(ctx, hipMemsetAsync(acc, 0, (size_t)cells * sizeof(int64_t), ctx->stream));
    if (ntiles == 0) return IG_OK;
    // per tap: one 8-byte atomic; per sample its record and weight
    ig_prof_scope prof(ctx, "dcf_spread", (double)M * (4.0 * (double)rec_stride + 8.0 + 8.0 * tw * tw * tw));
    u64* ap = reinterpret_cast<u64*>(acc);
    const dim3 grid((unsigned)ntiles), blk(DCF_BLK);
#define IG_DCF_SPREAD(TW) \
    hipLaunchKernelGGL((k_dcf_spread<TW>), grid, blk, 0, ctx->stream, M, records, rec_stride, order, tile_ptr, tile_ids, w, scale, lds_min, ap, \
                       (int)n0, (int)nm, (int)ns)
    if (tw == 4) IG_DCF_SPREAD(4); else if (tw == 6) IG_DCF_SPREAD(6); else IG_DCF_SPREAD(8);
#undef IG_DCF_SPREAD
    IG_LAUNCH_CHECK(ctx, "k_dcf_spread");
    return IG_OK;
}

int ig_dcf_gather_div_r32(ig_ctx* ctx, int64_t M, int tw, const uint32_t* records, int64_t rec_stride, const uint32_t* order,
                          const int64_t* acc, int64_t n0, int64_t nm, int64_t ns, double scale, const float* w, float* w_out,
                          float* s_out, float* maxima) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_dcf_gather_div_r32: ctx is NULL");
    if (int rc = dcf_check(ctx, "ig_dcf_gather_div_r32", M, tw, records, rec_stride, order, n0, nm, ns, scale)) return rc;
    IG_REQUIRE(ctx, acc != nullptr && maxima != nullptr && (M == 0 || (w && w_out)), "ig_dcf_gather_div_r32: NULL pointer");
    const uintptr_t w0 = (uintptr_t)w, o0 = (uintptr_t)w_out, s0 = (uintptr_t)s_out, nb = (uintptr_t)M * sizeof(float);
    IG_REQUIRE(ctx, w == w_out || !ig_bytes_overlap(w0, w0 + nb, o0, o0 + nb), "ig_dcf_gather_div_r32: w_out overlaps w (w_out == w is the in-place form)");
    IG_REQUIRE(ctx, !s_out || (!ig_bytes_overlap(s0, s0 + nb, w0, w0 + nb) && !ig_bytes_overlap(s0, s0 + nb, o0, o0 + nb)),
               "ig_dcf_gather_div_r32: s_out overlaps w or w_out");
    if (int rc = ig_set_device(ctx)) return rc;
    IG_HIP(ctx, hipMemsetAsync(maxima, 0, 2 * sizeof(float), ctx->stream));
    if (M == 0) return IG_OK;
    const int64_t blocks = (M + DCF_WAVES * DCF_SPW * DCF_GROUPS - 1) / (DCF_WAVES * DCF_SPW * DCF_GROUPS);
    ig_prof_scope prof(ctx, "dcf_gather_div", (double)M * (4.0 * (double)rec_stride + 12.0 + 8.0 * tw * tw * tw));
    const dim3 grid((unsigned)blocks), blk(DCF_BLK);
    const long long* ap = reinterpret_cast<const long long*>(acc);
    unsigned* mp = reinterpret_cast<unsigned*>(maxima);
#define IG_DCF_GATHER(TW) \
    hipLaunchKernelGGL((k_dcf_gather_div<TW>), grid, blk, 0, ctx->stream, M, records, rec_stride, order, ap, (int)n0, (int)nm, (int)ns, \
                       1.0 / scale, w, w_out, s_out, mp)
    if (tw == 4) IG_DCF_GATHER(4); else if (tw == 6) IG_DCF_GATHER(6); else IG_DCF_GATHER(8);
#undef IG_DCF_GATHER
    IG_LAUNCH_CHECK(ctx, "k_dcf_gather_div");
    return IG_OK;
}

int ig_rowscale_r32_c64(ig_ctx* ctx, int64_t n, int64_t ncols, const float* w, const void* x, int64_t ldx, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_rowscale_r32_c64: ctx is NULL");
    if (n < 1 || ncols < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_rowscale_r32_c64: a panel of %lld x %lld, at least 1 x 1 is supported", (long long)n, (long long)ncols);
    IG_REQUIRE(ctx, w && x && y, "ig_rowscale_r32_c64: NULL pointer");
    IG_REQUIRE(ctx, ldx >= n && ldy >= n, "ig_rowscale_r32_c64: leading dimension (%lld, %lld) below the %lld rows", (long long)ldx, (long long)ldy, (long long)n);
    IG_REQUIRE(ctx, (x == y && ldx == ldy) || !ig_panels_overlap(x, ldx, n, ncols, y, ldy, n, ncols),
               "ig_rowscale_r32_c64: y overlaps x (y == x with ldy == ldx is the in-place form)");
    const uintptr_t w0 = (uintptr_t)w, y0 = (uintptr_t)y;
    IG_REQUIRE(ctx, !ig_bytes_overlap(w0, w0 + (uintptr_t)n * sizeof(float), y0, y0 + (uintptr_t)((ncols - 1) * ldy + n) * sizeof(float2)),
               "ig_rowscale_r32_c64: y overlaps w");
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, "rowscale", 16.0 * (double)n * (double)ncols + 4.0 * (double)n);
    const bool wide = n % 2 == 0 && ldx % 2 == 0 && ldy % 2 == 0 && (uintptr_t)x % 16 == 0 && y0 % 16 == 0 && w0 % 8 == 0;
    const int64_t nv = wide ? n / 2 : n;
    const dim3 grid = ig_grid_1d(nv, DCF_BLK, (int64_t)ctx->num_cu * 16);
    if (wide) hipLaunchKernelGGL((k_rowscale<2>), grid, dim3(DCF_BLK), 0, ctx->stream, nv, ncols, w, (const float2*)x, ldx, (float2*)y, ldy);
    else      hipLaunchKernelGGL((k_rowscale<1>), grid, dim3(DCF_BLK), 0, ctx->stream, nv, ncols, w, (const float2*)x, ldx, (float2*)y, ldy);
    IG_LAUNCH_CHECK(ctx, "k_rowscale");
    return IG_OK;
}
