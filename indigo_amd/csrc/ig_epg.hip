// Extended-phase-graph signal simulation: the signal curves of a dictionary of (T1, T2, B1) atoms under one pulse program
// (indigo_amd.dictmatch --model fse / fisp, Backend.epg_signal; tests/epg64.py restates it in float64).
//
// An atom's state is (F+_k, F-_k, Z_k), k < nstates, all complex, Z_0 = 1 and the rest 0 at the start.  Step s of the program holds
// (alpha, phi, a, b, flags) and runs  RF(B1 alpha, phi); relax(a); shift if SHIFT_A; record F+_0 if RECORD; relax(b); shift if
// SHIFT_B; F+ = F- = 0 if SPOIL.  With theta = B1 alpha, c = cos^2(theta/2), s = sin^2(theta/2), e = exp(i phi), A = e^2 s and
// B = e sin(theta):
//     F+' = c F+ + A F- - i B Z          F-' = conj(A) F+ + c F- + i conj(B) Z          Z' = -(i/2) conj(B) F+ + (i/2) B F- + cos(theta) Z
// relax(d) multiplies F+ and F- by E2 = exp(-d/T2) and Z by E1 = exp(-d/T1), then adds R = -expm1(-d/T1) to Z_0.  A shift moves F+ one
// state up (what leaves state nstates - 1 is lost: the truncation is part of the definition), F- one state down (a zero enters at
// nstates - 1) and sets F+_0 = conj(F-_0).
//
// A group of W lanes per atom: W = 64, one wavefront per atom, or, for nstates <= 32 and <= 16, W = 32 and 16 with two and four atoms
// in a wavefront.  Lane l of the group keeps the states l, l + 64, ... (SPL = 1, 2 or 4 states per lane, more than one only at
// W = 64: 6, 12 or 24 registers of state), so the RF pulse and the relaxation are lane-local and a shift is a rotation of the group
// by one lane plus the carry between a lane's own registers; no LDS.  States k >= nstates are kept at zero (F+ is cleared there
// after every shift, and nothing else can reach them), and states above the number of shifts executed so far are still zero and
// skipped a register at a time.  A group beyond the last atom repeats the last atom and stores nothing.
//
// Coefficients.  Within a block of W steps lane j of a group forms the twelve coefficients of step j for the group's atom -- E1, E2, R
// of both delays, c, A, B, cos(theta) -- in double from the float32 parameters and the double program and rounds each to float32
// once; the group then reads them lane by lane (v_readlane at W = 64, where the step index is uniform; a ds_bpermute within the
// group otherwise).  The double transcendentals cost 1/W of what they would per lane.  No fast-math intrinsics.  The state update is
// float32 with fused multiply-adds in a fixed order that does not depend on W: an atom's output bits do not depend on where it
// stands among the atoms or on the others.
//
// Records.  Lane r mod W of the group keeps record r; W records, or the last ones, leave as one contiguous run of the atom's column.
#include <cmath>
#include "ig_common.h"

namespace {

constexpr int EPG_MAXSTATES = 256;
constexpr int EPG_MAXSTEPS = 65535;
constexpr int EPG_WAVES = 4;                    // wavefronts of a workgroup: 4 x 64 / W atoms
constexpr int64_t EPG_MAXGRID = 1 << 20;        // workgroups; the atom loop strides beyond that
enum { EPG_SHIFT_A = 1, EPG_SHIFT_B = 2, EPG_RECORD = 4, EPG_SPOIL = 8 };

// one step as the kernel reads it: e = exp(i phi) and e^2 are the same for every atom and come from the host, in double
struct epg_step {
    double alpha, a, b;
    double er, ei, e2r, e2i;
    int32_t flags, pad;
};

// v of lane j of the caller's group of W lanes (base: the group's first lane); j is uniform
template <int W>
__device__ __forceinline__ float epg_lane(float v, int base, int j) {
    if constexpr (W == 64) return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
    else return __shfl(v, base | j);
}

template <int SPL>
struct epg_state {
    float pr[SPL], pi[SPL], mr[SPL], mi[SPL], zr[SPL], zi[SPL];        // F+, F-, Z of the states lane + 64 j
};

// F+ one state up, F- one state down, F+_0 = conj(F-_0); F+ stays zero at k >= nstates
template <int SPL, int W>
__device__ __forceinline__ void epg_shift(epg_state<SPL>& q, int base, int sl, int nstates) {
    const int up = base | ((sl + W - 1) & (W - 1)), down = base | ((sl + 1) & (W - 1));
    float upr[SPL], upi[SPL], dnr[SPL], dni[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        upr[j] = __shfl(q.pr[j], up); upi[j] = __shfl(q.pi[j], up);           // lane 0 holds what lane W - 1 had: state 64 j + 63 at W = 64
        dnr[j] = __shfl(q.mr[j], down); dni[j] = __shfl(q.mi[j], down);       // lane W - 1 holds what lane 0 had: state 64 j
    }
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        const bool last = sl == W - 1;        // (W < 64: SPL == 1 and nstates <= W, so a zero enters here or above nstates - 1)
        q.mr[j] = last ? (j + 1 < SPL ? dnr[j + 1 < SPL ? j + 1 : j] : 0.f) : dnr[j];
        q.mi[j] = last ? (j + 1 < SPL ? dni[j + 1 < SPL ? j + 1 : j] : 0.f) : dni[j];
    }
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        const bool first = sl == 0, live = sl + 64 * j < nstates;
        const float r = first ? (j > 0 ? upr[j > 0 ? j - 1 : 0] : q.mr[0]) : upr[j];
        const float i = first ? (j > 0 ? upi[j > 0 ? j - 1 : 0] : -q.mi[0]) : upi[j];
        q.pr[j] = live ? r : 0.f;
        q.pi[j] = live ? i : 0.f;
    }
}

template <int SPL>
__device__ __forceinline__ void epg_relax(epg_state<SPL>& q, int sl, int used, float E1, float E2, float R) {
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        if (64 * j < used) {                                                   // (uniform)
            q.pr[j] *= E2; q.pi[j] *= E2; q.mr[j] *= E2; q.mi[j] *= E2;
            q.zr[j] = fmaf(q.zr[j], E1, (j == 0 && sl == 0) ? R : 0.f);
            q.zi[j] *= E1;
        }
    }
}

template <int SPL, int W>
__global__ void __launch_bounds__(64 * EPG_WAVES)
k_epg_sim(int64_t na, int nsteps, int nstates, const float* __restrict__ t1, const float* __restrict__ t2, const float* __restrict__ b1,
          const epg_step* __restrict__ prog, float2* __restrict__ out, int64_t ldo) {
    static_assert(W == 64 || SPL == 1, "several states per lane only with a whole wavefront per atom");
    constexpr int P = 64 / W;                   // atoms of a wavefront
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sl = lane & (W - 1), base = lane & ~(W - 1);
    for (int64_t atom0 = ((int64_t)blockIdx.x * EPG_WAVES + wave) * P; atom0 < na; atom0 += (int64_t)gridDim.x * EPG_WAVES * P) {
        const bool valid = atom0 + lane / W < na;
        const int64_t atom = valid ? atom0 + lane / W : na - 1;
        const double T1 = (double)t1[atom], T2 = (double)t2[atom], B1 = (double)b1[atom];
        float2* __restrict__ col = out + atom * ldo;
        epg_state<SPL> q;
#pragma unroll
        for (int j = 0; j < SPL; ++j) { q.pr[j] = q.pi[j] = q.mr[j] = q.mi[j] = q.zr[j] = q.zi[j] = 0.f; }
        if (sl == 0) q.zr[0] = 1.f;
        int used = 1;                           // states below `used` may be non-zero: 1 + the shifts so far, at most nstates
        int nrec = 0;
        float2 rec = make_float2(0.f, 0.f);

        for (int s0 = 0; s0 < nsteps; s0 += W) {
            const int nb = nsteps - s0 < W ? nsteps - s0 : W;
            // lane j of a group: the coefficients of step s0 + j for the group's atom, in double, each rounded to float32 once
            float E1a = 1.f, E2a = 1.f, Ra = 0.f, E1b = 1.f, E2b = 1.f, Rb = 0.f, cc = 1.f, Ar = 0.f, Ai = 0.f, Br = 0.f, Bi = 0.f, ct = 1.f;
            int fl = 0;
            if (sl < nb) {
                const epg_step p = prog[s0 + sl];
                const double theta = B1 * p.alpha;
                double sh, ch, st, c_t;
                sincos(0.5 * theta, &sh, &ch);
                sincos(theta, &st, &c_t);
                E1a = (float)exp(-p.a / T1); E2a = (float)exp(-p.a / T2); Ra = (float)(-expm1(-p.a / T1));
                E1b = (float)exp(-p.b / T1); E2b = (float)exp(-p.b / T2); Rb = (float)(-expm1(-p.b / T1));
                cc = (float)(ch * ch);
                const double ss = sh * sh;
                Ar = (float)(p.e2r * ss); Ai = (float)(p.e2i * ss);
                Br = (float)(p.er * st); Bi = (float)(p.ei * st);
                ct = (float)c_t;
                fl = p.flags;
            }
#pragma unroll 1
            for (int j = 0; j < nb; ++j) {
                const float c = epg_lane<W>(cc, base, j), ar = epg_lane<W>(Ar, base, j), ai = epg_lane<W>(Ai, base, j),
                            br = epg_lane<W>(Br, base, j), bi = epg_lane<W>(Bi, base, j), cth = epg_lane<W>(ct, base, j);
                const float hr = 0.5f * br, hi = 0.5f * bi;                   // B / 2, exact
                const int flags = __builtin_amdgcn_readlane(fl, j);          // (the same program for every group: group 0's copy)
                // RF
#pragma unroll
                for (int r = 0; r < SPL; ++r) {
                    if (64 * r < used) {                                       // (uniform)
                        const float pr = q.pr[r], pi = q.pi[r], mr = q.mr[r], mi = q.mi[r], zr = q.zr[r], zi = q.zi[r];
                        // F+' = c F+ + A F- - i B Z,  -i B Z = (br zi + bi zr) - i (br zr - bi zi)
                        q.pr[r] = fmaf(bi, zr, fmaf(br, zi, fmaf(-ai, mi, fmaf(ar, mr, c * pr))));
                        q.pi[r] = fmaf(bi, zi, fmaf(-br, zr, fmaf(ai, mr, fmaf(ar, mi, c * pi))));
                        // F-' = conj(A) F+ + c F- + i conj(B) Z,  i conj(B) Z = (bi zr - br zi) + i (br zr + bi zi)
                        q.mr[r] = fmaf(-br, zi, fmaf(bi, zr, fmaf(ai, pi, fmaf(ar, pr, c * mr))));
                        q.mi[r] = fmaf(bi, zi, fmaf(br, zr, fmaf(-ai, pr, fmaf(ar, pi, c * mi))));
                        // Z' = -(i/2) conj(B) F+ + (i/2) B F- + cos(theta) Z, with h = B / 2:
                        //   -i conj(h) F+ = (hr pi - hi pr) - i (hr pr + hi pi),   i h F- = -(hr mi + hi mr) + i (hr mr - hi mi)
                        q.zr[r] = fmaf(-hi, mr, fmaf(-hr, mi, fmaf(-hi, pr, fmaf(hr, pi, cth * zr))));
                        q.zi[r] = fmaf(-hi, mi, fmaf(hr, mr, fmaf(-hi, pi, fmaf(-hr, pr, cth * zi))));
                    }
                }
                epg_relax<SPL>(q, sl, used, epg_lane<W>(E1a, base, j), epg_lane<W>(E2a, base, j), epg_lane<W>(Ra, base, j));
                if (flags & EPG_SHIFT_A) { epg_shift<SPL, W>(q, base, sl, nstates); used = used < nstates ? used + 1 : used; }
                if (flags & EPG_RECORD) {
                    const float fr = epg_lane<W>(q.pr[0], base, 0), fi = epg_lane<W>(q.pi[0], base, 0);
                    if (sl == (nrec & (W - 1))) rec = make_float2(fr, fi);
                    ++nrec;
                    if ((nrec & (W - 1)) == 0 && valid) col[nrec - W + sl] = rec;  // W records: one contiguous run (512 bytes at W = 64)
                }
                epg_relax<SPL>(q, sl, used, epg_lane<W>(E1b, base, j), epg_lane<W>(E2b, base, j), epg_lane<W>(Rb, base, j));
                if (flags & EPG_SHIFT_B) { epg_shift<SPL, W>(q, base, sl, nstates); used = used < nstates ? used + 1 : used; }
                if (flags & EPG_SPOIL) {
#pragma unroll
                    for (int r = 0; r < SPL; ++r) { q.pr[r] = q.pi[r] = q.mr[r] = q.mi[r] = 0.f; }
                }
            }
        }
        if (sl < (nrec & (W - 1)) && valid) col[(nrec & ~(W - 1)) + sl] = rec;  // the last, partial run
    }
}

}  // namespace

int ig_epg_sim_c64(ig_ctx* ctx, int64_t na, int64_t nsteps, int64_t nstates, const float* t1, const float* t2, const float* b1,
                   const double* steps, const int32_t* flags, void* out, int64_t ldo) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_epg_sim_c64: ctx is NULL");
    if (na < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_epg_sim_c64: %lld atoms, at least 1 is supported", (long long)na);
    if (nsteps < 1 || nsteps > EPG_MAXSTEPS)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_epg_sim_c64: %lld steps, between 1 and %d are supported", (long long)nsteps, EPG_MAXSTEPS);
    if (nstates < 1 || nstates > EPG_MAXSTATES)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_epg_sim_c64: %lld states, between 1 and %d are supported", (long long)nstates, EPG_MAXSTATES);
    IG_REQUIRE(ctx, t1 && t2 && b1 && steps && flags && out, "ig_epg_sim_c64: NULL pointer");
    int64_t nrec = 0;
    std::vector<epg_step> prog((size_t)nsteps);
    for (int64_t s = 0; s < nsteps; ++s) {
        const double alpha = steps[4 * s], phi = steps[4 * s + 1], a = steps[4 * s + 2], b = steps[4 * s + 3];
        IG_REQUIRE(ctx, flags[s] >= 0 && flags[s] <= 15, "ig_epg_sim_c64: step %lld has the flags %d, 0 ... 15 are defined", (long long)s, (int)flags[s]);
        IG_REQUIRE(ctx, std::isfinite(alpha) && std::isfinite(phi) && std::isfinite(a) && std::isfinite(b),
                   "ig_epg_sim_c64: step %lld holds a value that is not finite", (long long)s);
        IG_REQUIRE(ctx, a >= 0 && b >= 0, "ig_epg_sim_c64: step %lld has a negative duration (%g, %g)", (long long)s, a, b);
        nrec += (flags[s] & EPG_RECORD) ? 1 : 0;
        const double er = std::cos(phi), ei = std::sin(phi);
        prog[(size_t)s] = epg_step{alpha, a, b, er, ei, er * er - ei * ei, 2.0 * er * ei, flags[s], 0};
    }
    IG_REQUIRE(ctx, nrec >= 1, "ig_epg_sim_c64: the program records nothing (no step has the RECORD flag, 4)");
    IG_REQUIRE(ctx, ldo >= nrec, "ig_epg_sim_c64: leading dimension %lld of out below the %lld records of the program", (long long)ldo, (long long)nrec);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)((na - 1) * ldo + nrec) * sizeof(float2);
    const float* par[3] = {t1, t2, b1};
    const char* names[3] = {"t1", "t2", "b1"};
    for (int i = 0; i < 3; ++i)
        IG_REQUIRE(ctx, !ig_bytes_overlap(o0, o1, (uintptr_t)par[i], (uintptr_t)par[i] + (uintptr_t)na * sizeof(float)), "ig_epg_sim_c64: out overlaps %s", names[i]);
    if (int rc = ig_set_device(ctx)) return rc;
    const size_t need = prog.size() * sizeof(epg_step);
    if (ctx->epg_bytes < need) {
        if (ctx->d_epg) { IG_HIP(ctx, hipStreamSynchronize(ctx->stream)); IG_HIP(ctx, hipFree(ctx->d_epg)); ctx->d_epg = nullptr; ctx->epg_bytes = 0; }
        IG_HIP(ctx, hipMalloc(&ctx->d_epg, need));
        ctx->epg_bytes = need;
    }
    // stream-ordered behind an earlier simulation that still reads the scratch; `prog` is gone when this function returns
    IG_HIP(ctx, hipMemcpyAsync(ctx->d_epg, prog.data(), need, hipMemcpyHostToDevice, ctx->stream));
    IG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ig_prof_scope prof(ctx, "epg_sim", (double)na * (12.0 + 8.0 * (double)nrec));
#define IG_EPG_GO(SPL, W) hipLaunchKernelGGL((k_epg_sim<SPL, W>), ig_grid_1d(na, EPG_WAVES * (64 / W), EPG_MAXGRID), dim3(64 * EPG_WAVES), 0, ctx->stream, \
                                             na, (int)nsteps, (int)nstates, t1, t2, b1, (const epg_step*)ctx->d_epg, (float2*)out, ldo)
    if (nstates <= 16) IG_EPG_GO(1, 16); else if (nstates <= 32) IG_EPG_GO(1, 32); else if (nstates <= 64) IG_EPG_GO(1, 64);
    else if (nstates <= 128) IG_EPG_GO(2, 64); else IG_EPG_GO(4, 64);
#undef IG_EPG_GO
    IG_LAUNCH_CHECK(ctx, "k_epg_sim");
    return IG_OK;
}
