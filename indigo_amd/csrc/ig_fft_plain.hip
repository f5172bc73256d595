// The FFT kernels that are not on the SENSE path (that one is k_fft_2stage, ig_fft.hip), each with its one launch function:
//
//  * the two-launch 256^3 transform k_fft3d_a / k_fft3d_b (below);
//
//  * LDS kernel k_fft_lds (n <= 4096 with prime factors in {2,3,5,7}):
//    a workgroup owns a tile of W neighbouring columns.  The tile is loaded
//    with coalesced global reads (for axis 0, where a column is a contiguous
//    line, the tile is one contiguous block and is transposed on the way in),
//    kept in LDS as [n][W+1] (one pad element per row against bank conflicts)
//    next to an LDS copy of the n twiddles, transformed by radix-8/4/2/3/5/7
//    Stockham stages (each thread holds up to 8 elements in registers between
//    the read barrier and the write barrier, so one LDS buffer suffices), and
//    written back the way it came.  Tiles are disjoint, so an axis can run in
//    place.  HBM traffic: exactly one read and one write of the volume per axis.
//
//  * generic kernel k_fft_generic_stage (anything else: large prime factors, n > 4096):
//    one Stockham stage per launch through global memory, one thread per
//    output element, any radix (a prime radix p is a direct p-point DFT).
//    Slow, but exact in structure for every size; needs a ping-pong workspace.
//
//  * the elementwise steps k_chirp_pre / _mul / _post of the unfused chirp-z route.
//
// No other unit names these kernels.  The inverse transform is computed as conj(FFT(conj(x))).
#include "ig_common.h"
#include "ig_packed.h"
#include "ig_fft_plan.h"
#include "ig_fft_regs.h"

namespace {

// ---- 256^3 in TWO launches ------------------------------------------------------------------------------------
// The plain 3-D transform (one k_fft_2stage pass per axis, ig_fft.hip) is three passes = 6 x the volume in HBM traffic; the reference's own accounting
// (benchmark.py:55) prices a 3-D transform at 4 x.  For 256^3 volumes (BASELINE config 2) two launches suffice if a
// workgroup owns 16384 elements (2 x 64 registers per thread pair ... 32 complex values per thread, 512 threads) and the
// y axis is split 64 x 4 between the launches:
//
//   launch A, workgroup (z, n2):  the 64 lines y = 4*n1 + n2 of plane z.  y stage 1 (64-point DFT over n1 = 8 x 8), the
//             inter-stage twiddle w256^(n2 k1), then the full 256-point x transform (4 x 8 x 8).  Lines go out to
//             y' = k1 + 64*n2: one contiguous 128 KB block per workgroup.  Out of place.
//   launch B, workgroup (16 x, k1): the 4 rows y' = k1 + 64*n2 for all 256 z.  y stage 2 (4-point DFT over n2, giving
//             ky = k1 + 64*k2 in place), then the full 256-point z transform (8 x 32).  In place.
//
// Every stage is a register DFT on values the thread already holds; between stages the workgroup redistributes through
// LDS in four 32 KB rounds (launch A: twice across waves and once inside each wave; launch B: once).  All LDS address
// maps below are conflict-free (one lane per 8-byte slot modulo 64); tools/fft2pass_model.py is a thread-level numpy
// model of exactly these maps, checked against numpy.fft.fftn.
// Streaming hints of the two launches, as measured: launch A loads with the hint, stores WITHOUT it -- it stores 16-byte pieces,
// two instructions per 128-byte line, and a streaming hint on partial-line stores is ruinous (1.48 against 0.78 ms) --, launch B
// uses none (1.746 against 1.788 ms per 256^3 x 16 transform with them).  The blocks of both launches are renumbered so that every
// XCD walks a contiguous range.
constexpr bool F3A_NT_LD = true, F3A_NT_ST = false, F3B_NT_LD = false, F3B_NT_ST = false;
constexpr int F3_LDS_ELEMS = 64 * 72;            // largest exchange image (launch A, second exchange)

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ void __launch_bounds__(512, 4)
k_fft3d_a(const float2* __restrict__ in, float2* __restrict__ out, const float2* __restrict__ tw, int inverse) {
    extern __shared__ float2 lds[];
    float2* __restrict__ tws = lds + F3_LDS_ELEMS;
    const int tid = threadIdx.x;
    for (int k = tid; k < 256; k += 512) tws[k] = tw[k];       // (round 5: written behind the loads instead, as in k_fft_2stage, the transform took 1.73 against 1.69 ms)
    // each XCD walks a contiguous range of (n2, z, volume) triples: the four n2 workgroups of a plane -- interleaved 2 KB lines
    // of the same 512 KB -- run behind one L2 at about the same time
    const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), tot = gridDim.x * gridDim.y * gridDim.z;
    const unsigned logical = (lin & 7u) * (tot >> 3) + (lin >> 3);            // (tot is a multiple of 8: 256 * 4 * batch)
    const int n2 = (int)(logical & 3u), z = (int)((logical >> 2) & 255u);
    const int64_t base = ((int64_t)(logical >> 10) << 24) + ((int64_t)z << 16);
    const int xl = tid & 63, a = tid >> 6;
    const bool inv = inverse != 0;

    // role 0: lane = x mod 64, wave = a.  v[j][b]: line n1 = a + 8b, x = xl + 64j (a wave load = 512 contiguous bytes)
    // (buffer loads: descriptor at the wave's first line, one 32-bit lane offset, the (b, j) displacement as a scalar / immediate
    // offset -- 32 loads in flight without 32 address register pairs)
    cx v[4][8];
    {
        const int a_u = __builtin_amdgcn_readfirstlane(a);              // the wave index is wave-uniform
        const rsrc_t r_in = make_rsrc(in + base + 256 * n2 + 1024 * a_u);
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j][b] = from2(buf_ld<F3A_NT_LD>(r_in, (unsigned)xl * 8u, (unsigned)(64 * j + 8192 * b) * 8u));
                if (inv) v[j][b] = cconj(v[j][b]);
            }
    }
    __syncthreads();                                   // twiddle table visible
    // y stage 1a: 8-point DFT over b, twiddle w64^(a kb)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        PFFT<8, false, false>::run(v[j]);
#pragma unroll
        for (int kb = 1; kb < 8; ++kb) v[j][kb] = cxmul(v[j][kb], from2(tws[(4 * a * kb) & 255]));
    }
    // exchange 1 (a <-> kb between waves, lane kept): image [a][kb][xl], two images (two j) per round
    cx r[4][8];
    float2* __restrict__ img1 = lds + F3_LDS_ELEMS + 256;         // second image (behind the twiddle table)
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
        if (jp) __syncthreads();
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            lds[(a * 8 + kb) * 64 + xl] = to2(v[2 * jp][kb]);
            img1[(a * 8 + kb) * 64 + xl] = to2(v[2 * jp + 1][kb]);
        }
        __syncthreads();
#pragma unroll
        for (int ap = 0; ap < 8; ++ap) {
            r[2 * jp][ap] = from2(lds[(ap * 8 + a) * 64 + xl]);
            r[2 * jp + 1][ap] = from2(img1[(ap * 8 + a) * 64 + xl]);
        }
    }
    const int kb = a;                                  // role 1: the wave index now names kb
    // y stage 1b: 8-point DFT over a -> line k1 = kb + 8 ka; inter-launch twiddle w256^(n2 k1); x stage 1: 4-point DFT over j
    cx p[8][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) PFFT<8, false, false>::run(r[j]);
#pragma unroll
    for (int ka = 0; ka < 8; ++ka) {
        const cx wy = from2(tws[(n2 * (kb + 8 * ka)) & 255]);
        cx t4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) t4[j] = cxmul(r[j][ka], wy);
        PFFT<4, false, false>::run(t4);
        p[ka][0] = t4[0];
#pragma unroll
        for (int kj = 1; kj < 4; ++kj) p[ka][kj] = cxmul(t4[kj], from2(tws[(xl * kj) & 255]));
    }
    // exchange 2: image [line][72] (x within a line); role 2 = (c = x mod 8, line): lane = c + 8*(line mod 8), wave = line / 8
    const int c = tid & 7, l = (tid >> 3) & 7, line = (tid >> 3);
    cx q[4][8];
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
        __syncthreads();
#pragma unroll
        for (int ka = 0; ka < 8; ++ka) {
            lds[(kb + 8 * ka) * 72 + xl] = to2(p[ka][2 * jp]);
            img1[(kb + 8 * ka) * 72 + xl] = to2(p[ka][2 * jp + 1]);
        }
        __syncthreads();
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            q[2 * jp][d] = from2(lds[line * 72 + c + 8 * d]);
            q[2 * jp + 1][d] = from2(img1[line * 72 + c + 8 * d]);
        }
    }
    // x stage 2: 8-point DFT over d, twiddle w64^(c kd)
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) {
        PFFT<8, false, false>::run(q[kj]);
#pragma unroll
        for (int kd = 1; kd < 8; ++kd) q[kj][kd] = cxmul(q[kj][kd], from2(tws[(4 * c * kd) & 255]));
    }
    // exchange 3 (c <-> kd among the 8 lanes of a line: inside the wave): image [line][64], swizzled both ways
    __syncthreads();                                   // the last round of exchange 2 has been read everywhere
    const int kd3 = c;                                 // role 3: the low lane bits now name kd
    cx t3[4][8];
#pragma unroll
    for (int jp = 0; jp < 2; ++jp) {
        if (jp) wave_sync();
#pragma unroll
        for (int kd = 0; kd < 8; ++kd) {
            lds[line * 64 + 8 * ((c + l) & 7) + ((kd + l) & 7)] = to2(q[2 * jp][kd]);
            img1[line * 64 + 8 * ((c + l) & 7) + ((kd + l) & 7)] = to2(q[2 * jp + 1][kd]);
        }
        wave_sync();
#pragma unroll
        for (int cc = 0; cc < 8; ++cc) {
            t3[2 * jp][cc] = from2(lds[line * 64 + 8 * ((cc + l) & 7) + ((kd3 + l) & 7)]);
            t3[2 * jp + 1][cc] = from2(img1[line * 64 + 8 * ((cc + l) & 7) + ((kd3 + l) & 7)]);
        }
    }
    // x stage 3: 8-point DFT over c -> kx = kj + 4 kd + 32 kc; four adjacent kx per thread and kc: two 16-byte stores
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) PFFT<8, false, false>::run(t3[kj]);
    const rsrc_t r_out = make_rsrc(out + base + 256 * 64 * n2);
    const unsigned l_out = (unsigned)(256 * line + 4 * kd3) * 8u;
#pragma unroll
    for (int kc = 0; kc < 8; ++kc) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            cx e0 = t3[2 * h][kc], e1 = t3[2 * h + 1][kc];
            if (inv) { e0 = cconj(e0); e1 = cconj(e1); }
            // the displacement goes into the instruction's immediate offset (lane offset + constant), NOT into the scalar
            // offset operand: a 16-byte buffer store with a scalar-register offset whose data registers are overwritten by the
            // next VALU instruction stored stale upper lanes on gfx950 (the compiler only pads that hazard for immediate offsets)
            buf_st_f4<F3A_NT_ST>(r_out, l_out + (unsigned)(32 * kc + 2 * h) * 8u, make_float4(e0.v.x, e0.v.y, e1.v.x, e1.v.y));
        }
    }
}

__global__ void __launch_bounds__(512, 4)
k_fft3d_b(const float2* __restrict__ in, float2* __restrict__ out, const float2* __restrict__ tw, int inverse) {
    extern __shared__ float2 lds[];
    float2* __restrict__ tws = lds + 2 * F3_LDS_ELEMS;
    const int tid = threadIdx.x;
    for (int k = tid; k < 256; k += 512) tws[k] = tw[k];       // (round 5: written behind the loads instead, as in k_fft_2stage, the transform took 1.73 against 1.69 ms)
    // blocks are dealt round-robin to the 8 XCDs: give each XCD a contiguous range of (x tile, k1, volume) triples, so that the
    // sixteen x tiles of a row group -- adjacent 128-byte pieces of the same 2 KB rows -- run behind one L2 at about the same time
    const unsigned lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z), tot = gridDim.x * gridDim.y * gridDim.z;
    const unsigned logical = (lin & 7u) * (tot >> 3) + (lin >> 3);            // (tot is a multiple of 8: 16 * 64 * batch)
    const int xs = (int)(logical & 15u) * 16, k1 = (int)((logical >> 4) & 63u);
    const int64_t base = ((int64_t)(logical >> 10) << 24) + xs;
    // role 0: h = lane bit 0 picks the rows n2 = h, h + 2 (the other two live in the neighbouring lane); w = x; t = z mod 16
    const int h = tid & 1, w = (tid >> 1) & 15, t = tid >> 5;
    const bool inv = inverse != 0;
    cx v[2][16];                                       // [m][k]: row n2 = h + 2m, z = t + 16k
    const unsigned l_io = ((unsigned)w + ((unsigned)t << 16) + (unsigned)h * (256u * 64u)) * 8u;   // x + 65536*(z mod 16) + the row of h
#pragma unroll
    for (int k = 0; k < 16; ++k)
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            // descriptor re-based per (k, m): a scalar add; the lane offset stays below 8.6 MB
            v[m][k] = from2(buf_ld<F3B_NT_LD>(make_rsrc(in + base + 256 * (k1 + 128 * m) + ((int64_t)(16 * k) << 16)), l_io, 0));
            if (inv) v[m][k] = cconj(v[m][k]);
        }
    __syncthreads();
    // y stage 2: 4-point DFT over n2 = h + 2m -> ky = k1 + 64 k2, k2 = q + 2h.  In the thread: the sum / difference over m
    // (q = 0, 1) and the twiddle w4^(h q) = -i for h = q = 1; then one exchange with the neighbouring lane (h ^ 1):
    // h = 0 keeps own + partner (k2 = q), h = 1 keeps partner - own (k2 = q + 2).
    cx y[2][16];                                       // [q][k]
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        cx a0 = v[0][k] + v[1][k], a1 = v[0][k] - v[1][k];
        if (h) a1 = cmul_mi_c(a1);
        cx p0, p1;
        p0.v = v2f{dpp_f<0xB1>(a0.v.x), dpp_f<0xB1>(a0.v.y)};      // quad_perm [1,0,3,2]: the lane with the other h
        p1.v = v2f{dpp_f<0xB1>(a1.v.x), dpp_f<0xB1>(a1.v.y)};
        y[0][k] = h ? p0 - a0 : a0 + p0;
        y[1][k] = h ? p1 - a1 : a1 + p1;
    }
    __builtin_amdgcn_sched_barrier(0);
    // z stage 1: 16-point DFT over k, twiddle w256^(t kk); exchange (t <-> kk among the threads of one (x, h)); z stage 2:
    // 16-point DFT over t -> kz = kk + 16 rr.  One round per q: every thread writes 16 and reads 16 values.
    const int kk1 = t;                                 // role 1: the same thread index now names kk
    const int k2_base = 2 * h;
    const unsigned l_st = ((unsigned)w + ((unsigned)kk1 << 16) + (unsigned)k2_base * (256u * 64u)) * 8u;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        PFFT<16, false, false>::run(y[q]);
        if (q) __syncthreads();
        // twiddle and hand over four values at a time; the compiler-level fences keep the scheduler from hoisting all
        // fifteen twiddle loads (30 registers) above the transform, which spilled y[1] at the 128-register cap
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int kk = 4 * g; kk < 4 * g + 4; ++kk) {
                if (kk) y[q][kk] = cxmul(y[q][kk], from2(tws[(t * kk) & 255]));
                lds[t * 544 + kk * 32 + h * 16 + w] = to2(y[q][kk]);
            }
            asm volatile("" ::: "memory");
        }
        __syncthreads();
        cx r[16];
#pragma unroll
        for (int tt = 0; tt < 16; ++tt) r[tt] = from2(lds[tt * 544 + kk1 * 32 + h * 16 + w]);
        PFFT<16, false, false>::run(r);
        const float2* const ob = out + base + 256 * (k1 + 64 * q);
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) {
            cx e = r[rr];
            if (inv) e = cconj(e);
            buf_st<F3B_NT_ST>(make_rsrc(ob + ((int64_t)(16 * rr) << 16)), l_st, 0, to2(e));
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// AXIS0: inner == 1 (columns are contiguous lines of n elements).
template <bool AXIS0>
__global__ void __launch_bounds__(1024)
k_fft_lds(const float2* __restrict__ x, float2* __restrict__ y, const float2* __restrict__ tw,
          int n, int64_t inner, int64_t ncols, int W, int T, int nstages, Radices rad, int inverse) {
    extern __shared__ float2 lds[];
    const int WP = W + 1;
    float2* __restrict__ tws = lds + (size_t)n * WP;
    const int tid = threadIdx.x, nth = blockDim.x;
    const int64_t c0 = (int64_t)blockIdx.x * W;
    const int wcount = (int)((ncols - c0 < W) ? (ncols - c0) : W);

    for (int k = tid; k < n; k += nth) tws[k] = tw[k];

    const int w = tid % W, t = tid / W;
    int64_t colbase = 0;
    if (AXIS0) {
        const float2* __restrict__ src = x + c0 * n;
        const int cnt = wcount * n;
        for (int e = tid; e < cnt; e += nth) {
            const int ww = e / n, j = e - ww * n;
            float2 v = src[e];
            if (inverse) v.y = -v.y;
            lds[j * WP + ww] = v;
        }
    } else {
        if (w < wcount) {
            const int64_t col = c0 + w;
            const int64_t o = col / inner, i = col - o * inner;
            colbase = i + inner * n * o;
            const float2* __restrict__ src = x + colbase;
            for (int j = t; j < n; j += T) {
                float2 v = src[(int64_t)j * inner];
                if (inverse) v.y = -v.y;
                lds[j * WP + w] = v;
            }
        }
    }
    __syncthreads();

    int Ns = 1;
    for (int s = 0; s < nstages; ++s) {
        const int R = rad.r[s];
        switch (R) {
            case 8: lds_stage<8>(lds, tws, n, Ns, T, t, w, WP); break;
            case 4: lds_stage<4>(lds, tws, n, Ns, T, t, w, WP); break;
            case 2: lds_stage<2>(lds, tws, n, Ns, T, t, w, WP); break;
            case 3: lds_stage<3>(lds, tws, n, Ns, T, t, w, WP); break;
            case 5: lds_stage<5>(lds, tws, n, Ns, T, t, w, WP); break;
            case 7: lds_stage<7>(lds, tws, n, Ns, T, t, w, WP); break;
            default: break;   // the planner never emits other radices for this kernel
        }
        Ns *= R;
    }

    if (AXIS0) {
        float2* __restrict__ dst = y + c0 * n;
        const int cnt = wcount * n;
        for (int e = tid; e < cnt; e += nth) {
            const int ww = e / n, j = e - ww * n;
            float2 v = lds[j * WP + ww];
            if (inverse) v.y = -v.y;
            dst[e] = v;
        }
    } else {
        if (w < wcount) {
            float2* __restrict__ dst = y + colbase;
            for (int j = t; j < n; j += T) {
                float2 v = lds[j * WP + w];
                if (inverse) v.y = -v.y;
                dst[(int64_t)j * inner] = v;
            }
        }
    }
}

// One Stockham stage through global memory, one thread per output element.
__global__ void __launch_bounds__(256)
k_fft_generic_stage(const float2* __restrict__ in, float2* __restrict__ out, const float2* __restrict__ tw,
                    int64_t n, int64_t inner, int64_t total, int R, int64_t Ns, int inverse) {
    const int64_t nb = n / R;
    const int64_t tstride = nb / Ns;
    const int64_t rstride = n / R;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t i = idx % inner;
        const int64_t rest = idx / inner;
        const int64_t jo = rest % n;
        const int64_t o = rest / n;
        const int64_t m = jo % Ns;
        const int64_t k = (jo / Ns) % R;
        const int64_t b = (jo / (Ns * R)) * Ns + m;
        const float2* __restrict__ src = in + i + inner * n * o;
        float2 acc = make_float2(0.f, 0.f);
        for (int q = 0; q < R; ++q) {
            const float2 v = src[(b + q * nb) * inner];
            const int64_t ti = (q * m * tstride + (int64_t)((q * k) % R) * rstride) % n;
            float2 wv = tw[ti];
            if (inverse) wv.y = -wv.y;
            cfma(acc, v, wv);
        }
        out[idx] = acc;
    }
}

// elementwise steps of the unfused chirp-z route (contiguous axes, lengths beyond the A x B kernel)
__global__ void __launch_bounds__(256)
k_chirp_pre(const float2* __restrict__ x, float2* __restrict__ W, const float2* __restrict__ b, int64_t n, int64_t m, int64_t inner, int64_t total_m) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total_m; idx += (int64_t)gridDim.x * 256) {
        const int64_t i = idx % inner, rest = idx / inner, j = rest % m, o = rest / m;
        W[idx] = j < n ? cmul(x[i + inner * (j + n * o)], b[j]) : make_float2(0.f, 0.f);
    }
}
__global__ void __launch_bounds__(256)
k_chirp_mul(float2* __restrict__ W, const float2* __restrict__ bhat, int64_t m, int64_t inner, int64_t total_m) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total_m; idx += (int64_t)gridDim.x * 256)
        W[idx] = cmul(W[idx], bhat[(idx / inner) % m]);
}
__global__ void __launch_bounds__(256)
k_chirp_post(const float2* __restrict__ W, float2* __restrict__ y, const float2* __restrict__ bout, int64_t n, int64_t m, int64_t inner, int64_t total_n) {
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total_n; idx += (int64_t)gridDim.x * 256) {
        const int64_t i = idx % inner, rest = idx / inner, k = rest % n, o = rest / n;
        y[idx] = cmul(W[i + inner * (k + m * o)], bout[k]);
    }
}

}  // namespace

// ---- the launches ---------------------------------------------------------------------------------------------------------------

// two exchange images + the twiddle table: 75.7 KB per workgroup (two workgroups per CU), above the 64 KB a kernel may use
// without opting in
constexpr size_t F3_LDS_BYTES = (size_t)(2 * F3_LDS_ELEMS + 256) * sizeof(float2);
static int fft3d_opt_in(ig_ctx* ctx) {
    if (ctx->fft3d_attr) return IG_OK;
    IG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fft3d_a), hipFuncAttributeMaxDynamicSharedMemorySize, (int)F3_LDS_BYTES));
    IG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fft3d_b), hipFuncAttributeMaxDynamicSharedMemorySize, (int)F3_LDS_BYTES));
    ctx->fft3d_attr = true;
    return IG_OK;
}
int ig_launch_fft3d_a(ig_ctx* ctx, const float2* in, float2* out, const float2* tw, int64_t batch, int inverse) {
    if (int rc = fft3d_opt_in(ctx)) return rc;
    hipLaunchKernelGGL(k_fft3d_a, dim3(256, 4, (unsigned)batch), dim3(512), F3_LDS_BYTES, ctx->stream, in, out, tw, inverse);
    IG_LAUNCH_CHECK(ctx, "k_fft3d_a");
    return IG_OK;
}
int ig_launch_fft3d_b(ig_ctx* ctx, const float2* in, float2* out, const float2* tw, int64_t batch, int inverse) {
    if (int rc = fft3d_opt_in(ctx)) return rc;
    hipLaunchKernelGGL(k_fft3d_b, dim3(16, 64, (unsigned)batch), dim3(512), F3_LDS_BYTES, ctx->stream, in, out, tw, inverse);
    IG_LAUNCH_CHECK(ctx, "k_fft3d_b");
    return IG_OK;
}

// one axis pass of the LDS kernel, in -> out (in place allowed: a workgroup holds its columns before it stores)
int ig_launch_fft_lds(ig_ctx* ctx, const AxisPlan& ax, const float2* in, float2* out, int inverse) {
    const int64_t ncols = ax.inner * ax.outer;
    const int64_t blocks = (ncols + ax.W - 1) / ax.W;
    IG_REQUIRE(ctx, blocks <= 0x7fffffffLL, "ig_fft_exec: too many tiles");
    if (ax.lds_bytes > 48 * 1024 && !ctx->fft_lds_attr) {
        // more than the default dynamic-LDS limit: opt in (gfx950 has 160 KiB per CU)
        IG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fft_lds<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BUDGET));
        IG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fft_lds<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BUDGET));
        ctx->fft_lds_attr = true;
    }
    const dim3 grid((unsigned)blocks), block((unsigned)(ax.W * ax.T));
    with_flag(ax.inner == 1, [&](auto axis0) {
        hipLaunchKernelGGL(k_fft_lds<axis0>, grid, block, ax.lds_bytes, ctx->stream, in, out, ax.d_tw,
                           (int)ax.n, ax.inner, ncols, ax.W, ax.T, ax.nstages, ax.rad, inverse); });
    IG_LAUNCH_CHECK(ctx, "k_fft_lds");
    return IG_OK;
}

int ig_launch_fft_generic_stage(ig_ctx* ctx, unsigned blocks, const float2* in, float2* out, const float2* tw, int64_t n, int64_t inner,
                                int64_t total, int R, int64_t Ns, int inverse) {
    hipLaunchKernelGGL(k_fft_generic_stage, dim3(blocks), dim3(256), 0, ctx->stream, in, out, tw, n, inner, total, R, Ns, inverse);
    IG_LAUNCH_CHECK(ctx, "k_fft_generic_stage");
    return IG_OK;
}

int ig_launch_chirp_pre(ig_ctx* ctx, unsigned blocks, const float2* x, float2* W, const float2* b, int64_t n, int64_t m, int64_t inner, int64_t total_m) {
    hipLaunchKernelGGL(k_chirp_pre, dim3(blocks), dim3(256), 0, ctx->stream, x, W, b, n, m, inner, total_m);
    IG_LAUNCH_CHECK(ctx, "k_chirp_pre");
    return IG_OK;
}
int ig_launch_chirp_mul(ig_ctx* ctx, unsigned blocks, float2* W, const float2* bhat, int64_t m, int64_t inner, int64_t total_m) {
    hipLaunchKernelGGL(k_chirp_mul, dim3(blocks), dim3(256), 0, ctx->stream, W, bhat, m, inner, total_m);
    IG_LAUNCH_CHECK(ctx, "k_chirp_mul");
    return IG_OK;
}
int ig_launch_chirp_post(ig_ctx* ctx, unsigned blocks, const float2* W, float2* y, const float2* bout, int64_t n, int64_t m, int64_t inner, int64_t total_n) {
    hipLaunchKernelGGL(k_chirp_post, dim3(blocks), dim3(256), 0, ctx->stream, W, y, bout, n, m, inner, total_n);
    IG_LAUNCH_CHECK(ctx, "k_chirp_post");
    return IG_OK;
}
