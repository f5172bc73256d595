// The register DFT building blocks of the FFT kernels (ig_fft.hip, ig_fft_plain.hip): lane exchanges, butterflies, the LDS stage and
// the 4 ... 32-point transforms on float2 and on packed (ig_packed.h) values.  Device helpers only -- no kernels: a kernel template
// in a shared header would be instantiated, and compiled, once per unit.
#pragma once
#include "ig_common.h"
#include "ig_packed.h"
#include "ig_fft_plan.h"        // E

namespace {

// lane exchange inside a row of 16 lanes by a DPP control word (out-of-row sources read as zero)
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true));
}

// ---- butterflies --------------------------------------------------------------
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }   // a * (-i)

// streaming (non-temporal) 8-byte accesses: an axis pass touches every byte exactly once
typedef float v2f_t __attribute__((ext_vector_type(2)));
template <bool NT>
__device__ __forceinline__ float2 ld_stream(const float2* p) {
    if (NT) { const v2f_t v = __builtin_nontemporal_load(reinterpret_cast<const v2f_t*>(p)); return make_float2(v.x, v.y); }
    return *p;
}
template <bool NT>
__device__ __forceinline__ void st_stream(float2* p, float2 a) {
    if (NT) { v2f_t v; v.x = a.x; v.y = a.y; __builtin_nontemporal_store(v, reinterpret_cast<v2f_t*>(p)); }
    else *p = a;
}

__device__ __forceinline__ void bfly2(float2& a, float2& b) {
    const float2 t = csub(a, b);
    a = cadd(a, b);
    b = t;
}

// forward 4-point DFT in place, natural output order
__device__ __forceinline__ void bfly4(float2& a0, float2& a1, float2& a2, float2& a3) {
    const float2 t0 = cadd(a0, a2), t1 = csub(a0, a2);
    const float2 t2 = cadd(a1, a3), t3 = mul_mi(csub(a1, a3));
    a0 = cadd(t0, t2); a2 = csub(t0, t2);
    a1 = cadd(t1, t3); a3 = csub(t1, t3);
}

template <int R>
struct Bfly {
    // generic small prime: direct R-point DFT, roots read from the LDS twiddle
    // table of the enclosing length-n transform (R divides n)
    __device__ static __forceinline__ void run(float2 (&v)[R], const float2* __restrict__ tws, int n) {
        float2 o[R];
        const int step = n / R;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            float2 acc = v[0];
#pragma unroll
            for (int q = 1; q < R; ++q) cfma(acc, v[q], tws[((q * k) % R) * step]);
            o[k] = acc;
        }
#pragma unroll
        for (int k = 0; k < R; ++k) v[k] = o[k];
    }
};
template <> struct Bfly<2> {
    __device__ static __forceinline__ void run(float2 (&v)[2], const float2*, int) { bfly2(v[0], v[1]); }
};
template <> struct Bfly<4> {
    __device__ static __forceinline__ void run(float2 (&v)[4], const float2*, int) { bfly4(v[0], v[1], v[2], v[3]); }
};
template <> struct Bfly<8> {
    __device__ static __forceinline__ void run(float2 (&v)[8], const float2*, int) {
        // two 4-point DFTs on even / odd inputs, then the 8th-root twiddles
        bfly4(v[0], v[2], v[4], v[6]);
        bfly4(v[1], v[3], v[5], v[7]);
        const float h = 0.70710678118654752440f;
        const float2 w1 = make_float2(h, -h), w3 = make_float2(-h, -h);
        v[3] = cmul(v[3], w1);
        v[5] = mul_mi(v[5]);
        v[7] = cmul(v[7], w3);
        // after bfly4 the even half holds E[0..3] in v[0],v[2],v[4],v[6] and the odd half O[0..3] in v[1],v[3],v[5],v[7]
        bfly2(v[0], v[1]);   // X0, X4
        bfly2(v[2], v[3]);   // X1, X5
        bfly2(v[4], v[5]);   // X2, X6
        bfly2(v[6], v[7]);   // X3, X7
        // reorder to natural output order X0..X7
        const float2 x4 = v[1], x1 = v[2], x5 = v[3], x2 = v[4], x6 = v[5], x3 = v[6];
        v[1] = x1; v[2] = x2; v[3] = x3; v[4] = x4; v[5] = x5; v[6] = x6;
    }
};

// One Stockham stage over the LDS tile.  lds[j*WP + w] is element j of column w.
// Thread (w, t) handles butterflies b = t, t+T, ... (< n/R) of column w.
template <int R>
__device__ __forceinline__ void lds_stage(float2* __restrict__ lds, const float2* __restrict__ tws,
                                          int n, int Ns, int T, int t, int w, int WP) {
    constexpr int BPT = E / R;
    const int nb = n / R;
    float2 v[BPT][R];
#pragma unroll
    for (int q = 0; q < BPT; ++q) {
        const int b = t + q * T;
        if (b < nb) {
#pragma unroll
            for (int k = 0; k < R; ++k) v[q][k] = lds[(b + k * nb) * WP + w];
        }
    }
    __syncthreads();
    const int tstride = nb / Ns;     // n / (Ns * R)
#pragma unroll
    for (int q = 0; q < BPT; ++q) {
        const int b = t + q * T;
        if (b < nb) {
            const int m = b % Ns;
            if (Ns > 1) {
#pragma unroll
                for (int k = 1; k < R; ++k) v[q][k] = cmul(v[q][k], tws[k * m * tstride]);
            }
            Bfly<R>::run(v[q], tws, n);
            const int base = (b - m) * R + m;
#pragma unroll
            for (int k = 0; k < R; ++k) lds[(base + k * Ns) * WP + w] = v[q][k];
        }
    }
    __syncthreads();
}

// ---- register-resident DFTs of 16 and 32 points --------------------------------
// cos(2 pi j / 32); compile-time foldable so that unrolled code carries literals
__host__ __device__ constexpr float cos32(int j) {
    j &= 31;
    if (j > 16) j = 32 - j;
    const float T[9] = {1.0f, 0.980785251f, 0.923879504f, 0.831469595f, 0.707106769f,
                        0.555570245f, 0.382683426f, 0.195090324f, 0.0f};
    return j <= 8 ? T[j] : -T[16 - j];
}
// a * exp(-2 pi i j / 32), trivial rotations without multiplies (j is a constant after unrolling)
__device__ __forceinline__ float2 mul_w32(float2 a, int j) {
    j &= 31;
    if (j == 0) return a;
    if (j == 8) return make_float2(a.y, -a.x);
    if (j == 16) return make_float2(-a.x, -a.y);
    if (j == 24) return make_float2(-a.y, a.x);
    const float c = cos32(j), s = -cos32(j + 24);      // w = c + i s, s = -sin(2 pi j/32)
    return make_float2(fmaf(a.x, c, -a.y * s), fmaf(a.x, s, a.y * c));
}

template <int N> struct RegFFT;       // in-place forward DFT of N register values, natural order out
template <> struct RegFFT<4> {
    __device__ static __forceinline__ void run(float2 (&x)[4]) { bfly4(x[0], x[1], x[2], x[3]); }
};
template <> struct RegFFT<8> {
    __device__ static __forceinline__ void run(float2 (&x)[8]) { Bfly<8>::run(x, nullptr, 0); }
};
template <int N> struct RegFFT {      // N = 16, 32: radix-4 decimation in frequency over N/4-point DFTs
    __device__ static __forceinline__ void run(float2 (&x)[N]) {
        constexpr int M = N / 4;
        float2 z[4][M];
#pragma unroll
        for (int r = 0; r < M; ++r) {
            bfly4(x[r], x[r + M], x[r + 2 * M], x[r + 3 * M]);
            z[0][r] = x[r];
#pragma unroll
            for (int q = 1; q < 4; ++q) z[q][r] = mul_w32(x[r + q * M], r * q * (32 / N));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) RegFFT<M>::run(z[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < M; ++k) x[4 * k + q] = z[q][k];
    }
};

// The same DFT when only the middle half of the inputs, x[N/4 .. 3N/4), is non-zero (the image box of a
// 2x-oversampled grid): the first radix-4 layer collapses to one add/sub pair per butterfly and the outer
// quarters of x are never read, so they cost neither loads nor registers.
template <int N> struct RegFFTHalfIn {
    __device__ static __forceinline__ void run(float2 (&x)[N]) {
        constexpr int M = N / 4;
        float2 z[4][M];
#pragma unroll
        for (int r = 0; r < M; ++r) {
            const float2 a1 = x[r + M], a2 = x[r + 2 * M];
            const float2 t3 = mul_mi(a1);
            z[0][r] = cadd(a2, a1);
            z[1][r] = mul_w32(csub(t3, a2), r * (32 / N));
            z[2][r] = mul_w32(csub(a2, a1), r * 2 * (32 / N));
            const float2 s = cadd(a2, t3);
            z[3][r] = mul_w32(make_float2(-s.x, -s.y), r * 3 * (32 / N));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) RegFFT<M>::run(z[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < M; ++k) x[4 * k + q] = z[q][k];
    }
};

// (packed complex arithmetic -- one 64-bit register pair per complex number, v_pk_* instructions: ig_packed.h)
__device__ __forceinline__ void pbfly2(cx& a, cx& b) { const cx t = a - b; a = a + b; b = t; }
// Direction as arithmetic: INV = true is the same butterfly network with every constant conjugated (the unnormalised inverse
// DFT), so an inverse pass needs no conjugation of its inputs and outputs -- that cost the cropped passes two VALU
// instructions per element on each side (a packed negate and a move), a tenth of their vector instructions.
// (ASM = false keeps the compiler's own lowering of the -+i products: the second launch of the two-launch 256^3 transform is
// scheduled around it -- with the assembly forms it went from 94 to 128 registers and spilled.)
template <bool INV = false, bool ASM = true>
__device__ __forceinline__ void pbfly4(cx& a0, cx& a1, cx& a2, cx& a3) {
    const cx t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, dd = a1 - a3;
    a0 = t0 + t2; a2 = t0 - t2;
    if (ASM) {
        a1 = INV ? padd_pi(t1, dd) : padd_mi(t1, dd);          // t1 -+ i dd
        a3 = INV ? padd_mi(t1, dd) : padd_pi(t1, dd);
    } else {
        const cx t3 = INV ? cmul_pi_c(dd) : cmul_mi_c(dd);
        a1 = t1 + t3; a3 = t1 - t3;
    }
}
// a * exp(-+2 pi i j / 32) with a literal root (j constant after unrolling), trivial rotations without multiplies
template <bool INV = false, bool ASM = true>
__device__ __forceinline__ cx pmul_w32(cx a, int j) {
    j &= 31;
    if (INV) j = (32 - j) & 31;
    if (j == 0) return a;
    if (j == 8) return ASM ? cmul_mi(a) : cmul_mi_c(a);
    if (j == 16) return cneg(a);
    if (j == 24) return ASM ? cmul_pi(a) : cmul_pi_c(a);
    const float c = cos32(j), s = -cos32(j + 24);      // w = c + i s
    return cxmul(a, mk(c, s));
}
template <int N, bool INV = false, bool ASM = true> struct PFFT;          // in-place DFT of N packed register values, natural order out
template <bool INV, bool ASM> struct PFFT<4, INV, ASM> {
    __device__ static __forceinline__ void run(cx (&x)[4]) { pbfly4<INV, ASM>(x[0], x[1], x[2], x[3]); }
};
template <bool INV, bool ASM> struct PFFT<8, INV, ASM> {
    __device__ static __forceinline__ void run(cx (&v)[8]) {
        pbfly4<INV, ASM>(v[0], v[2], v[4], v[6]);
        pbfly4<INV, ASM>(v[1], v[3], v[5], v[7]);
        const float h = 0.70710678118654752440f;
        v[3] = cxmul(v[3], mk(h, INV ? h : -h));
        v[7] = cxmul(v[7], mk(-h, INV ? h : -h));
        pbfly2(v[0], v[1]); pbfly2(v[2], v[3]); pbfly2(v[6], v[7]);
        if (ASM) {   // v[4] +- (-+i) v[5]
            const cx e = v[4], o = v[5];
            v[4] = INV ? padd_pi(e, o) : padd_mi(e, o);
            v[5] = INV ? padd_mi(e, o) : padd_pi(e, o);
        } else {
            v[5] = INV ? cmul_pi_c(v[5]) : cmul_mi_c(v[5]);
            pbfly2(v[4], v[5]);
        }
        const cx x4 = v[1], x1 = v[2], x5 = v[3], x2 = v[4], x6 = v[5], x3 = v[6];
        v[1] = x1; v[2] = x2; v[3] = x3; v[4] = x4; v[5] = x5; v[6] = x6;
    }
};
template <int N, bool INV, bool ASM> struct PFFT {         // N = 16, 32: radix-4 decimation in frequency over N/4-point DFTs
    __device__ static __forceinline__ void run(cx (&x)[N]) {
        constexpr int M = N / 4;
        cx z[4][M];
#pragma unroll
        for (int r = 0; r < M; ++r) {
            pbfly4<INV, ASM>(x[r], x[r + M], x[r + 2 * M], x[r + 3 * M]);
            z[0][r] = x[r];
#pragma unroll
            for (int q = 1; q < 4; ++q) z[q][r] = pmul_w32<INV, ASM>(x[r + q * M], r * q * (32 / N));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) PFFT<M, INV, ASM>::run(z[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < M; ++k) x[4 * k + q] = z[q][k];
    }
};
// only the middle half of the inputs, x[N/4 .. 3N/4), is non-zero: the first radix-4 layer collapses
template <int N> struct PFFTHalfIn {
    __device__ static __forceinline__ void run(cx (&x)[N]) {
        constexpr int M = N / 4;
        cx z[4][M];
#pragma unroll
        for (int r = 0; r < M; ++r) {
            const cx a1 = x[r + M], a2 = x[r + 2 * M];
            z[0][r] = a2 + a1;
            z[1][r] = pmul_w32(cneg(padd_pi(a2, a1)), r * (32 / N));          // (-i) a1 - a2
            z[2][r] = pmul_w32(a2 - a1, r * 2 * (32 / N));
            z[3][r] = pmul_w32(cneg(padd_mi(a2, a1)), r * 3 * (32 / N));      // -(a2 + (-i) a1)
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) PFFT<M>::run(z[q]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < M; ++k) x[4 * k + q] = z[q][k];
    }
};

}  // namespace
