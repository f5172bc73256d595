// Batched complex-to-complex FFT for complex64 on gfx950 -- hand-written
// Stockham autosort kernels, no vendor FFT library.
//
// Contract (Backend.fftn/ifftn, indigo/backends/backend.py:497-509; oracle
// np.py:102-115; cuFFT usage cuda.py:470-498): Fortran-ordered volume
// dims[0..rank-1] (dims[0] contiguous) times `batch` contiguous volumes,
// unnormalised in both directions.
//
// One pass per axis.  For an axis of length n the array is viewed as
// [outer][n][inner] (inner contiguous), i.e. inner*outer independent
// "columns" of n elements with stride `inner`.
//
//  * two-stage register kernel k_fft_2stage (n = 512 = 32x16, n = 256 = 16x16; every pass of the SENSE path):
//    a thread loads its 32 (16) inputs straight from HBM, runs a register DFT, hands the results over through LDS
//    in two 32 KB rounds, runs the second register DFT and stores straight back.  The same kernel serves the
//    zero-pad-aware forward / cropped inverse transforms (boxes, diagonal weights, k-space support bitmap,
//    coil-interleaved layouts, coil combination) through one pass descriptor; see PassDesc and the kernel below.
//
//  * the kernels off that path -- the two-launch 256^3 transform, the LDS kernel (n <= 4096 with prime factors in {2,3,5,7}), the
//    generic kernel (anything else) and the elementwise steps of the unfused chirp-z route: ig_fft_plain.hip.
//  * A x B lengths and one-launch chirp-z passes: ig_fft_ab.h, compiled in ig_fft_abd0..3.hip.
//
// This unit holds k_fft_2stage and its launch and nothing else; planning, execution and the C ABI are ig_fft_plan.hip.
// The inverse transform is computed as conj(FFT(conj(x))).
#include "ig_common.h"
#include "ig_packed.h"
#include "ig_fft_ab.h"
#include "ig_fft_plan.h"
#include "ig_fft_regs.h"

namespace {

// Choices measured in rounds 1-3 and now fixed in the code (the rejected alternatives are recorded in DESIGN.md section 3.1; what
// is left to switch lives in tools/kernel_lab.py, not here):
//  * non-temporal (streaming) loads and stores in the 2-stage axis passes -- every byte of a pass is touched exactly once
//    (256^3 x 8 SENSE evaluation: 8.95 ms with either one off, 8.58 ms with both on);
//  * wave-uniform skipping of the load instructions no lane wants, and scalar-gated stores (one opaque asm block each) on
//    unweighted passes with a run-time output box;
//  * the strided half-OUTPUT variants are not capped at 128 VGPRs (the cap spilled and was slower).

// Two-stage kernel for n = R1*R2 (256 = 16x16, 512 = 32x16): the whole column lives in registers
// twice -- stage 1 reads its R1 inputs straight from global memory, stage 2 writes its R2 outputs
// straight back -- with ONE LDS exchange in between (Stockham index map, inter-stage twiddles applied
// on the way into LDS).  A workgroup = W columns x T threads; lanes run along the direction that is
// contiguous in memory (columns for strided axes, elements for axis 0), so every wave access is a
// set of 128-byte segments and every LDS access is conflict-free at the minimum cycle count
// (axis 0 uses a 16-element XOR swizzle of the line).  Inputs outside [in_lo, in_hi) are zeros that
// are never loaded and outputs outside [out_lo, out_hi) are never stored: that is what makes the
// zero-padded forward / cropped inverse transforms cheap (SENSE: 1/8 of the grid is non-zero).
// HALF selects boxes known at compile time (the image box of a 2x-oversampled grid is [n/4, 3n/4)):
//   1: input half, output box at run time      3: input half, output full
//   2: output half, input box at run time      4: output half, input full
// Half inputs prune the first butterfly layer; compile-time boxes need no predicates or bounds registers.
// Loads and stores carry the non-temporal (streaming) hint: every byte of a pass is touched exactly once.
// KEEP_ST: the stores take the default cache policy instead -- the first pass of a chunk of the x / y pair (ig_fft_xy.h), whose
// output the chunk's second pass reads back a few launches later (measured: DESIGN.md section 3.1; the loads stay streaming).
template <int R1, int R2, int T, int W, bool AXIS0, int WMODE, bool BOXED, int HALF, bool KEEP_ST = false>
__global__ void __launch_bounds__(W * T, (!AXIS0 && R1 == 32 && (W == 32 || HALF == 1 || HALF == 3)) ? 4 : 1)
k_fft_2stage(PassDesc d, const float2* __restrict__ tw) {
    constexpr int n = R1 * R2, B1 = R2 / T, B2 = R1 / T, NT = W * T;
    constexpr bool NT_LD = true, NT_ST = !KEEP_ST;      // streaming hints on both sides (KEEP_ST: on the loads only)
    constexpr bool HALF_IN = HALF == 1 || HALF == 3, HALF_OUT = HALF == 2 || HALF == 4;
    constexpr int SUMW = WMODE >= 3 ? (1 << (WMODE - 3)) : 0;       // WMODE 3 + log2(coils): 3 -> 1 (no sum), 4 -> 2, 5 -> 4, 6 -> 8, 7 -> 16
    // direction: the half-input variants only serve forward (zero-padded) passes and the half-output variants only
    // inverse (cropped) ones, so their conjugations are sign modifiers, not a select per element
    // (SINV: the inverse transform by conjugated constants, PFFT<N, true>; the run-time direction of the general variants by
    // conjugating inputs and outputs around the forward network)
    constexpr bool SINV = HALF_OUT;
    const bool inv = (HALF_OUT || HALF_IN) ? false : (d.inverse != 0);
    static_assert(R2 % T == 0 && R1 % T == 0 && T == 16 && B1 == 1, "lane groups of 16, one stage-1 butterfly per thread");
    extern __shared__ float2 lds[];
    float2* __restrict__ tws = lds + (AXIS0 ? 16 * 17 * W : 16 * T * W);
    const int tid = threadIdx.x;
    // inter-stage twiddles in the order the threads read them: entry t * R1 + k = w_n^(t k) (the second half of the plan's table),
    // so a thread's R1 - 1 reads are one base address plus compile-time offsets, two values per LDS instruction
    // (NT == n: one value per thread, requested here and written to LDS only after the stage-1 loads have been issued -- written
    // straight away, the copy is a round trip of its own at the head of every workgroup: the compiler waits for it before anything else)
    constexpr int TWN = n / NT;                      // 1 (32-column tiles) or 2
    constexpr bool TW_LATE = (n % NT == 0) && TWN <= 2;
    float2 tw_mine[TW_LATE ? TWN : 1];
    if (TW_LATE) {
#pragma unroll
        for (int i = 0; i < TWN; ++i) tw_mine[i] = tw[n + tid + i * NT];
    } else for (int k = tid; k < n; k += NT) tws[k] = tw[n + k];

    const int t = AXIS0 ? (tid % T) : (tid / W);
    const int w = AXIS0 ? (tid / T) : (tid % W);
    // ---- the workgroup's tile: W consecutive k0 of one (k1, k2) row; everything below is wave-uniform
    // (Workgroups are dealt round-robin to the 8 XCDs.  Giving each XCD a contiguous range of tiles instead was measured
    // 10 % SLOWER on the z passes: with the default dealing all XCDs stream through the same DRAM pages together, and no
    // tile shares a cache line with another anyway.)
    // (tile of the row, k1, k2): pass_tile, ig_fft_ab.h
    unsigned tr, k1, k2;
    pass_tile(d, tr, k1, k2);
    const int64_t k0u = (int64_t)tr * ((!AXIS0 && d.cw) ? (d.cw_log2 >= 0 ? W >> d.cw_log2 : W / d.cw) : W);
    int in_lo = d.in_lo, in_hi = d.in_hi, out_lo = d.out_lo, out_hi = d.out_hi;
    // the tile's support records, requested here and tested behind the descriptor set-up (pass_records, ig_fft_ab.h)
    short2 k1r = make_short2(0, 0x7fff), trg = make_short2(0, 0x7fff);
    PassRecords rcd{0u, 0u, 0x7fff0000u, 0xffffffffu, false, false, false, true, false};
    if (BOXED && !AXIS0) rcd = pass_records(d, tw, tr, k1, 16, t, true);
    const bool has_k1r = rcd.has_k1r, has_trg = rcd.has_trg, has_zb = rcd.has_zb;
    // Buffer descriptors based at the tile's first column: every access is descriptor + a wave-uniform byte
    // offset (SGPR, or an immediate on axis 0) + ONE per-lane 32-bit offset.  A lane offset of IG_OOB fails the
    // hardware range check -- the load returns zero, the store is dropped -- which is how boxes and the ragged
    // last tile are predicated without a branch, so all loads of a stage issue back to back.
    // Strided passes re-base the descriptor for every group of 16 elements along the axis (a pure SGPR add), so a
    // column may span far more than the 2 GB window (y pass of the interleaved layout: 16 MB per element step).
    // (a side stored piece by piece -- the z-contiguous y <-> z intermediate, ig_fft_zc.h -- places the tile's first column by
    // piece and column of the piece: scalar arithmetic of the workgroup's head, nothing per lane or per element)
    int64_t o_in = k0u * d.in_s[0], o_out = k0u * d.out_s[0];
    if (BOXED && !AXIS0 && WMODE == 0 && d.zc_log2) {
        const int64_t q = k0u >> d.zc_log2, e = k0u - (q << d.zc_log2);
        if (d.in_zt) o_in = q * d.in_zt + e;
        if (d.out_zt) o_out = q * d.out_zt + e;
    }
    const float2* const b_in = d.in + (o_in + (int64_t)k1 * d.in_s[1] + (int64_t)k2 * d.in_s[2]);
    float2* const b_out = d.out + (o_out + (int64_t)k1 * d.out_s[1] + (int64_t)k2 * d.out_s[2]);
    const float2* const b_w = WMODE ? d.w + (k0u * d.w_s[0] + (int64_t)k1 * d.w_s[1] + (int64_t)k2 * d.w_s[2]) : nullptr;
    const rsrc_t r_in = make_rsrc(b_in), r_out = make_rsrc(b_out), r_w = make_rsrc(b_w);
    // x-axis passes run along contiguous memory by construction: unit strides known at compile time
    const unsigned isj = AXIS0 ? 1u : (unsigned)d.in_sj, osj = AXIS0 ? 1u : (unsigned)d.out_sj, wsj = AXIS0 ? 1u : (unsigned)d.w_sj;
    bool valid;
    unsigned l_in, l_out, l_w;
    if (!AXIS0 && d.cw) {
        const unsigned yl = d.cw_log2 >= 0 ? (unsigned)w >> d.cw_log2 : (unsigned)w / (unsigned)d.cw, a = (unsigned)w - yl * (unsigned)d.cw;
        valid = k0u + yl < d.ext0;
        l_in = (a * (unsigned)d.in_sa + yl * (unsigned)d.in_s[0] + (unsigned)t * isj) * 8u;
        l_out = (a * (unsigned)d.out_sa + yl * (unsigned)d.out_s[0] + (unsigned)t * osj) * 8u;
        l_w = (a * (unsigned)d.w_sa + yl * (unsigned)d.w_s[0] + (unsigned)t * wsj) * 8u;
    } else {
        valid = k0u + w < d.ext0;
        l_in = ((unsigned)w * (unsigned)d.in_s[0] + (unsigned)t * isj) * 8u;
        l_out = ((unsigned)w * (unsigned)d.out_s[0] + (unsigned)t * osj) * 8u;
        l_w = ((unsigned)w * (unsigned)d.w_s[0] + (unsigned)t * wsj) * 8u;
    }
    if (!valid) l_in = l_out = l_w = IG_OOB;
    if (!WMODE) l_w = IG_OOB;
    if (SUMW && (w % SUMW) != 0) l_out = IG_OOB;            // only a column's first sub-column stores the coil sum
    // ---- the records are needed from here on (everything above overlapped their round trip)
    if (has_k1r) k1r = rcd.k1_hull();
    if (has_k1r) {
        if ((int)k1 < k1r.x || (int)k1 >= k1r.y) return;
    }
    // (A half-input pass does not wait for its range here where it need not: its loads need nothing of it -- the output side is
    // narrowed behind the loads.  The y pass, whose hulls do not depend on k1 and are never empty inside a support; and a z pass
    // that has the ky hulls for its early exit above: an empty range inside the hull only leaves no store flagged.)
    const bool defer_out = HALF_IN && has_trg && d.tile_range_mode == 1 && (rcd.scalar || has_k1r);
    if (has_trg && !defer_out) {
        const short2 r = trg = rcd.range();
        if (d.tile_range_mode == 1) {
            out_lo = out_lo > r.x ? out_lo : r.x;
            out_hi = out_hi < r.y ? out_hi : r.y;
            if (out_hi <= out_lo) return;                             // nothing of this tile is ever read
        } else {
            in_lo = in_lo > r.x ? in_lo : r.x;
            in_hi = in_hi < r.y ? in_hi : r.y;
        }
    }

    // Element j = t + 16*m of this thread's column <-> bit m of a 32-bit word: ibits flags the inputs to read
    // (stage 1 loads m = k), obits the outputs to keep (stage 2 stores m = q + r*R1/16).  Boxes [lo, hi) become
    // bit ranges; a per-tile bitmap (k-space support at 16-row granularity) is and-ed in.
    auto ceil16 = [](int a) -> int { a += 15; return a <= 0 ? 0 : (a >= 512 ? 32 : a >> 4); };
    auto below = [](int h) -> uint32_t { return h >= 32 ? 0xffffffffu : ((1u << h) - 1u); };
    uint32_t ibits = 0xffffffffu, obits = 0xffffffffu;
    if (BOXED) {
        ibits = below(ceil16(in_hi - t)) & ~below(ceil16(in_lo - t));
        if (has_zb && d.tile_range_mode != 1) ibits &= rcd.bits();
    }
    // Wave-uniform version of the input mask (the OR over the wave's 64 / W values of t): where a bit is clear NO lane of the
    // wave wants that element, and the load instruction itself is skipped by a scalar branch -- a k-space column is
    // mostly unflagged rows (72 % on the headline problem), and an instruction whose lanes are all out of range still
    // costs its issue slot and its pass through the address unit.
    // (Unweighted passes only: the weighted run-time-box x pass went from 155 to 198 registers with them -- three waves per SIMD
    // to two, 1.08 -> 1.86 ms on config 5.  C++ branches around the STORES of the padded z pass cost it its register
    // allocation -- 172 bytes of spills at the 128-register cap -- and predicating them through the execution mask, one opaque
    // v_and / v_cmp / s_and_saveexec / store / s_mov exec block per element, was slower than the out-of-range offsets
    // (padded y pass 1.08 -> 1.14 ms, config 5 41.9 -> 44.3 ms).  What works for the stores is the scalar branch INSIDE one
    // opaque block per store, buf_st_gated below: no control flow for the compiler, padded z pass 1.21 -> 1.14 ms.)
    uint32_t gin = 0xffffffffu;
    if (BOXED && !AXIS0 && WMODE == 0 && !HALF_IN && HALF != 4) {
        gin = 0;
#pragma unroll
        for (int l = 0; l < 64; l += W) gin |= (uint32_t)__builtin_amdgcn_readlane((int)ibits, l);
    }
    constexpr bool GATE_ST = BOXED && !AXIS0 && WMODE == 0 && !HALF_OUT && HALF != 3;
    uint32_t gout = 0xffffffffu;
    // ---- stage 1: radix R1 on inputs j = t + k*R2, results (times w_n^{t k}) to the exchange
    // Strided passes re-base their descriptors once per GRP elements -- one 64-bit scalar add, hidden from the compiler, which
    // otherwise recomputes base + k * step with two 32-bit multiplies, a high multiply and their adds for every element -- and
    // reach the elements in between through the instruction's scalar offset (1, 2, 3 steps: three registers per stream, computed
    // once).  Per-element re-basing was a third of the scalar instructions of these kernels, and a wave issues one instruction
    // of any kind per turn.  (GRP * 16 - 1 element steps plus the tile's lanes must fit the 2 GB window: launch_2stage checks.)
    constexpr int GRP = 4;
    auto opaque = [](const float2*& q) { asm("" : "+s"(q)); };
    cx v[R1];
    {
        cx wv[R1];
        constexpr int K0 = HALF_IN ? R1 / 4 : 0, K1 = HALF_IN ? 3 * R1 / 4 : R1;
        const int64_t st_in = (int64_t)R2 * d.in_sj, st_w = WMODE == 1 ? (int64_t)R2 * d.w_sj : 0;
        const unsigned so_in = (unsigned)st_in * 8u, so_w = (unsigned)st_w * 8u;
        const float2* p_in = AXIS0 ? b_in : b_in + K0 * st_in;
        const float2* p_w = (AXIS0 || WMODE != 1) ? b_w : b_w + K0 * st_w;
        rsrc_t g_in = make_rsrc(p_in), g_w = make_rsrc(p_w);
#pragma unroll
        for (int k = K0; k < K1; ++k) {
            const int g = (k - K0) % GRP;
            if (!AXIS0 && g == 0 && k > K0) {
                p_in += GRP * st_in; opaque(p_in); g_in = make_rsrc(p_in);
                if (WMODE == 1) { p_w += GRP * st_w; opaque(p_w); g_w = make_rsrc(p_w); }
            }
            const bool stat = !BOXED || HALF_IN || HALF == 4;                 // box known at compile time
            // off = all ones (out of range) where the element is not wanted: one bit-field extract + one or
            const unsigned off = stat ? 0u : (unsigned)__builtin_amdgcn_sbfe((int)~ibits, k, 1);
            if (!stat && !AXIS0 && WMODE == 0 && !((gin >> k) & 1u)) v[k] = mk(0.f, 0.f);
            else if (AXIS0) {
                v[k] = from2(buf_ld<NT_LD>(r_in, l_in | off, (unsigned)(k * R2) * 8u));
                if (WMODE == 1) wv[k] = from2(buf_ld<false>(r_w, l_w | off, (unsigned)(k * R2) * 8u));
            } else {
                v[k] = from2(buf_ld<NT_LD>(g_in, l_in | off, (unsigned)g * so_in));
                if (WMODE == 1) wv[k] = from2(buf_ld<false>(g_w, l_w | off, (unsigned)g * so_w));
            }
        }
#pragma unroll
        for (int k = K0; k < K1; ++k) {
            if (WMODE == 1) v[k] = cxmul_r(v[k], wv[k]);
            if (inv) v[k] = cconj(v[k]);
        }
    }
    // ---- the output side of the boxes, behind the loads (the half-input y pass has not waited for its record until here)
    if (defer_out) {
        trg = rcd.range();
        out_lo = out_lo > trg.x ? out_lo : trg.x;
        out_hi = out_hi < trg.y ? out_hi : trg.y;
    }
    if (BOXED) {
        obits = below(ceil16(out_hi - t)) & ~below(ceil16(out_lo - t));
        if (has_zb && d.tile_range_mode == 1) obits &= rcd.bits();
    }
    // the wave-uniform mask for the stores of unweighted passes with a run-time output box -- as ONE opaque block per store (buf_st_gated)
    if (GATE_ST) {
        gout = 0;
#pragma unroll
        for (int l = 0; l < 64; l += W) gout |= (uint32_t)__builtin_amdgcn_readlane((int)obits, l);
    }
    if (TW_LATE) {
#pragma unroll
        for (int i = 0; i < TWN; ++i) tws[tid + i * NT] = tw_mine[i];
    }
    __syncthreads();            // twiddle table visible (the global loads above are already in flight)
    if (HALF_IN) PFFTHalfIn<R1>::run(v);
    else PFFT<R1, SINV>::run(v);
    {
        const float2* __restrict__ twt = tws + t * R1;
#pragma unroll
        for (int k = 1; k < R1; ++k) v[k] = SINV ? cxmulc(from2(twt[k]), v[k]) : cxmul_r(v[k], from2(twt[k]));
    }

    // ---- exchange + stage 2 in B2 = R1/16 rounds.  Stage-2 butterfly b2 = t + 16*q needs, from every
    // stage-1 thread b, exactly its output k = b2: round q therefore moves only the outputs
    // k in [16q, 16q+16) through LDS, i.e. 16 x 16 x W elements = 32 KB per round whatever R1 is.
    // Exchange element (b, kk) lives at row b, slot kk.  Strided axes: [b][kk][w] (lanes along w).  Axis 0: column
    // group w owns 16 rows of 17 slots -- the odd row stride makes both the row-wise writes and the column-wise
    // reads conflict-free, and every address is one per-thread base plus a compile-time offset.
    // (Round 5, not adopted: handing a round over in two halves of 8 slots makes the 32-column tiles' image 32 KB -- three workgroups
    // per CU by LDS -- but a thread then holds its 24 outputs still to hand over beside the 16 inputs of its second transform:
    // at the 80 registers six waves per SIMD allow the kernels spill 18 ... 24 registers.  Not measured.)
    float2* __restrict__ lw = AXIS0 ? lds + w * (16 * 17) + t * 17 : lds + (t * 16) * W + w;     // + kk * (AXIS0 ? 1 : W)
    float2* __restrict__ lr = AXIS0 ? lds + w * (16 * 17) + t      : lds + t * W + w;            // + k2 * (AXIS0 ? 17 : 16 * W)
#pragma unroll
    for (int q = 0; q < B2; ++q) {
        if (q > 0) __syncthreads();             // the previous round's reads are done
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) lw[kk * (AXIS0 ? 1 : W)] = to2(v[16 * q + kk]);
        __syncthreads();
        cx u[R2];
#pragma unroll
        for (int r = 0; r < R2; ++r) u[r] = from2(lr[r * (AXIS0 ? 17 : 16 * W)]);
        PFFT<R2, SINV>::run(u);
        constexpr int Q0 = HALF_OUT ? R2 / 4 : 0, Q1 = HALF_OUT ? 3 * R2 / 4 : R2;          // outputs outside are never stored
        const int64_t st_out = (int64_t)R1 * d.out_sj, st_w = WMODE >= 2 ? (int64_t)R1 * d.w_sj : 0;
        const unsigned so_out = (unsigned)st_out * 8u, so_w = (unsigned)st_w * 8u;
        const float2* p_out = AXIS0 ? b_out : b_out + (q * T) * d.out_sj + Q0 * st_out;
        const float2* p_w = (AXIS0 || WMODE < 2) ? b_w : b_w + (q * T) * d.w_sj + Q0 * st_w;
        cx wv[R2];          // kept outputs j = t + 16*(q + r*B2): bit q + r*B2 of obits
        if (WMODE >= 2) {
            rsrc_t g_w = make_rsrc(p_w);
#pragma unroll
            for (int r = Q0; r < Q1; ++r) {
                const int g = (r - Q0) % GRP;
                if (!AXIS0 && g == 0 && r > Q0) { p_w += GRP * st_w; opaque(p_w); g_w = make_rsrc(p_w); }
                const bool stat = !BOXED || HALF_OUT || HALF == 3;
                const unsigned off = stat ? 0u : (unsigned)__builtin_amdgcn_sbfe((int)~obits, q + r * B2, 1);
                if (AXIS0) wv[r] = from2(buf_ld<false>(r_w, l_w | off, (unsigned)(q * T + r * R1) * 8u));
                else wv[r] = from2(buf_ld<false>(g_w, l_w | off, (unsigned)g * so_w));
            }
        }
        rsrc_t g_out = make_rsrc(p_out);
        v4i_t gw_out = make_rsrc_words(p_out);
#pragma unroll
        for (int r = Q0; r < Q1; ++r) {
            const int g = (r - Q0) % GRP;
            if (!AXIS0 && g == 0 && r > Q0) {
                p_out += GRP * st_out; opaque(p_out);
                if (GATE_ST) gw_out = make_rsrc_words(p_out); else g_out = make_rsrc(p_out);
            }
            const bool stat = !BOXED || HALF_OUT || HALF == 3;
            cx ac = u[r];
            if (inv) ac = cconj(ac);
            if (WMODE >= 2) ac = cxmulc(wv[r], ac);
            float2 a = to2(ac);
            const unsigned off = stat ? 0u : (unsigned)__builtin_amdgcn_sbfe((int)~obits, q + r * B2, 1);
            if (SUMW) {
                // coil combination: the SUMW sub-columns (coils) of a column sit in SUMW consecutive lanes; data-parallel
                // primitives move the partial sums (no LDS traffic, no extra registers): afterwards the group's
                // first lane holds the total (the other lanes' l_out is out of range)
                if (SUMW >= 2)  { a.x += dpp_f<0xB1>(a.x);  a.y += dpp_f<0xB1>(a.y); }      // quad_perm [1,0,3,2]
                if (SUMW >= 4)  { a.x += dpp_f<0x4E>(a.x);  a.y += dpp_f<0x4E>(a.y); }      // quad_perm [2,3,0,1]
                if (SUMW >= 8)  { a.x += dpp_f<0x104>(a.x); a.y += dpp_f<0x104>(a.y); }     // row_shl:4
                if (SUMW >= 16) { a.x += dpp_f<0x108>(a.x); a.y += dpp_f<0x108>(a.y); }     // row_shl:8
            }
            if (AXIS0) buf_st<NT_ST>(r_out, l_out | off, (unsigned)(q * T + r * R1) * 8u, a);
            else if (GATE_ST) buf_st_gated<NT_ST>(gw_out, l_out | off, (unsigned)g * so_out, a, (gout >> (q + r * B2)) & 1u);
            else buf_st<NT_ST>(g_out, l_out | off, (unsigned)g * so_out, a);
        }
    }
}

// (Round 5, measured and removed: two neighbouring tiles per workgroup, software-pipelined -- the second tile's loads issued as soon
// as the first tile's stage-1 outputs sat in the exchange image, 110 registers, no spills, bit-identical results.  Same box,
// alternating runs: 6.652 / 6.657 ms per evaluation against 6.664 / 6.678 ms; two of the four passes 2-5 % faster, two 1-3 % slower.
// profiles/r05_fft_pass_experiments.txt.)

}  // namespace

// The launch grid of a pass kernel: (tiles of a row, k1, k2) in three dimensions where the extents allow (the dispatch order of the
// linear numbering, without the divisions at the head of every workgroup -- pass_tile, ig_fft_ab.h), else linear.  Also notes log2 of
// a power-of-two lane split.
static dim3 pass_grid(PassDesc& d, int64_t tpr) {
    d.tpr = (unsigned)tpr;
    d.cw_log2 = -1;
    if (d.cw > 0 && (d.cw & (d.cw - 1)) == 0) { d.cw_log2 = 0; while ((1 << d.cw_log2) < d.cw) ++d.cw_log2; }
    const int64_t rows = d.ncols / d.ext0, ext2 = d.ext1 > 0 ? rows / d.ext1 : 0;
    d.grid3 = (d.ext1 >= 1 && d.ext1 <= 65535 && ext2 >= 1 && ext2 <= 65535 && d.ext1 * ext2 == rows) ? 1 : 0;
    return d.grid3 ? dim3((unsigned)tpr, (unsigned)d.ext1, (unsigned)ext2) : dim3((unsigned)(tpr * rows));
}

// The tiles of a pass at cpt columns (k0 values) each: the launch grid, after checking that the tile count fits and that every
// in-tile byte offset -- `reach` element steps along the transform axis plus the tile's 16 lanes -- stays inside the 2 GB
// descriptor window (the weights' too where the pass addresses them)
int ig_pass_tiles(ig_ctx* ctx, PassDesc& d, int64_t cpt, int64_t reach, bool weights, const char* kernel, dim3& grid) {
    const int64_t tpr = (d.ext0 + cpt - 1) / cpt;
    const int64_t blocks = tpr * (d.ncols / d.ext0);           // ncols = ext0 * ext1 * ext2
    IG_REQUIRE(ctx, blocks <= 0x7fffffffLL && d.ext1 <= 0x7fffffffLL, "ig_fft: too many tiles");
    grid = pass_grid(d, tpr);
    const int64_t lim = 0x7fffffffLL / 8;
    const int64_t span_in = reach * d.in_sj + 15 * d.in_s[0] + 15 * d.in_sa, span_out = reach * d.out_sj + 15 * d.out_s[0] + 15 * d.out_sa;
    const int64_t span_w = weights ? reach * d.w_sj + 15 * d.w_s[0] + 15 * d.w_sa : 0;
    IG_REQUIRE(ctx, d.in_sj >= 0 && d.out_sj >= 0 && d.in_s[0] >= 0 && d.out_s[0] >= 0 && span_in < lim && span_out < lim && span_w < lim,
               "ig_fft: axis stride too large for the %s kernel", kernel);
    return IG_OK;
}

// Which instantiation a two-stage pass takes: whether it is boxed, its compile-time half box (HALF of k_fft_2stage) and
// whether it runs on 32-column tiles.  (PassDesc::wide fixes the width where the caller has to know it beforehand: the
// z-contiguous intermediate is laid out by the z pass's tile width, and its strides must not change the choice.)
bool ig_two_stage_variant(const AxisPlan& ax, const PassDesc& d, bool axis0, int wmode, bool& boxed, int& half) {
    boxed = d.tile_range || !(d.in_lo <= 0 && d.in_hi >= (int)ax.n && d.out_lo <= 0 && d.out_hi >= (int)ax.n);
    // the image box of a 2x-oversampled grid sits at [n/4, 3n/4): compile-time-pruned variants
    const int qn = (int)ax.n / 4;
    half = 0;
    if (boxed) {
        const bool in_full = d.in_lo <= 0 && d.in_hi >= (int)ax.n, out_full = d.out_lo <= 0 && d.out_hi >= (int)ax.n;
        if (d.in_lo == qn && d.in_hi == 3 * qn && !(d.tile_range && d.tile_range_mode == 2))
            half = (out_full && !d.tile_range && !d.tile_bits) ? 3 : 1;
        else if (d.out_lo == qn && d.out_hi == 3 * qn && !(d.tile_range && d.tile_range_mode == 1))
            half = (in_full && !d.tile_range && !d.tile_bits) ? 4 : 2;
        if (wmode == 1 && half != 3) half = 0;      // weighted variants exist for the fully static boxes only
        if (wmode >= 2 && half != 4) half = 0;
        if (((half == 1 || half == 3) && d.inverse) || ((half == 2 || half == 4) && !d.inverse)) half = 0;   // direction is baked in
    }
    // 32-column tiles (256-byte segments) pay where a side of the pass runs at a huge stride (y passes of the
    // interleaved layout, 16 MB per element: -11...-15 %), for the half-input variants, which fit 128 VGPRs, and -- since
    // round 3 skips the load instructions no lane wants -- for the half-output variants too (cropped z pass 1.28 -> 1.20 ms;
    // before that skip the wider tile lost there: 1.63 against 1.50 ms).
    const bool big_stride = (d.in_sj > d.out_sj ? d.in_sj : d.out_sj) * 8 >= (1 << 20);
    // boxed passes WITHOUT a compile-time half box (e.g. the 320-point box of a 512-point axis, oversampling 1.6) also take
    // 32-column tiles when one side runs at a huge stride: cropped y pass of config 5 0.85 -> 0.74 ms, padded y pass unchanged
    // ... and so do plain (unboxed) passes at a huge stride, through the same run-time-box variant: the z pass of a plain 512^3
    // transform steps 2 MB per element (3.82 -> 3.08 ms for 512^3 x 8)
    // ... and the z passes of such a box once the support bitmap gates their loads / stores (config 5: see DESIGN 3.1)
    const bool w32_generic = half == 0 && (big_stride || d.tile_bits != nullptr);
    const bool w32 = (ax.n == 512 && !axis0 && wmode == 0 && !d.cw && d.ext0 % 32 == 0 &&
        (half == 1 || half == 3 || half == 2 || half == 4 || w32_generic) &&
        (!d.tile_range || d.tile_shift >= 1));
    return d.wide ? d.wide == 2 : w32;
}


// The instantiations of k_fft_2stage: the (WMODE, HALF) pairs that exist, per family.  Weighted kernels come with the fully static
// boxes only (HALF 3 on the way in, 4 on the way out); the coil sums (WMODE 3 + log2(coils)) are strided passes.  Every kernel has the
// same signature, so a launch picks a pointer and goes through one call.
typedef void (*Kernel2S)(PassDesc, const float2*);
template <int WM, int HF> struct V2 {};
template <typename... P> struct V2List {};
using V2_BOXED = V2List<V2<0, 0>, V2<0, 1>, V2<0, 2>, V2<0, 3>, V2<0, 4>, V2<1, 0>, V2<1, 3>, V2<2, 0>, V2<2, 4>>;
using V2_SUM = V2List<V2<3, 0>, V2<3, 4>, V2<4, 0>, V2<4, 4>, V2<5, 0>, V2<5, 4>, V2<6, 0>, V2<6, 4>, V2<7, 0>, V2<7, 4>>;
using V2_W32 = V2List<V2<0, 0>, V2<0, 1>, V2<0, 2>, V2<0, 3>, V2<0, 4>>;
// ... with stores of the default cache policy (KEEP_ST): what writes the x <-> y intermediate -- the weighted padded x pass and the
// cropped (inverse) y pass, strided passes both
using V2_KEEP = V2List<V2<0, 0>, V2<0, 2>, V2<0, 4>, V2<1, 0>, V2<1, 3>>;
using V2_W32_KEEP = V2List<V2<0, 0>, V2<0, 2>, V2<0, 4>>;
// the boxed kernel <R1, 16, 16, W, AXIS0, wm, true, half, KEEP> if the list has the pair, else nullptr
template <int R1, int W, bool AXIS0, bool KEEP = false, int... WM, int... HF>
static Kernel2S pick_2stage(V2List<V2<WM, HF>...>, int wm, int half) {
    Kernel2S k = nullptr;
    ((wm == WM && half == HF ? (void)(k = &k_fft_2stage<R1, 16, 16, W, AXIS0, WM, true, HF, KEEP>) : (void)0), ...);
    return k;
}

// launch one 2-stage axis pass (n in {256, 512}); axis0 selects the lane mapping for contiguous columns; stream: null = the context's;
// keep_out: store with the default cache policy where the pass has such an instantiation (a hint: the results are the same)
int ig_launch_2stage(ig_ctx* ctx, const AxisPlan& ax, const PassDesc& d_in, bool axis0, int wmode, hipStream_t stream, bool keep_out) {
    PassDesc d = d_in;
    if (d.ncols == 0) return IG_OK;
    IG_REQUIRE(ctx, !d.tile_bits || d.tile_words == 16 || d.tile_words == 0, "ig_fft: the two-stage kernel reads support bitmaps of 16 words per entry (got %d)", d.tile_words);
    const int64_t cpt = (!axis0 && d.cw) ? ax.W / d.cw : ax.W;           // columns (k0 values) per tile
    IG_REQUIRE(ctx, !d.cw || (!axis0 && d.cw <= ax.W && ax.W % d.cw == 0), "ig_fft: bad lane split");
    // (strided passes re-base once per 4 groups of 16 elements and reach the three groups in between through the scalar
    // offset -- at 32 elements per step on the output side of a 512-point axis: 3 * 32 + 15 element steps plus the tile's lanes must fit)
    dim3 grid, block((unsigned)(ax.W * ax.T));
    if (int rc = ig_pass_tiles(ctx, d, cpt, axis0 ? ax.n + 15 : 3 * (ax.n / 16) + 15, wmode != 0, "two-stage", grid)) return rc;
    size_t lds = ax.lds_bytes;
    bool boxed; int half;
    Kernel2S k = nullptr;
    if (ig_two_stage_variant(ax, d, axis0, wmode, boxed, half)) {
        // 32-column tiles: 256-byte segments per row, 512 threads, 69.6 KB of LDS (2 workgroups per CU)
        if (d.tile_range) d.tile_shift -= 1;
        grid = pass_grid(d, d.ext0 / 32); block = dim3(512);
        lds = ((size_t)16 * 16 * 32 + 512) * 8;
        if (!ctx->fft_w32_attr) {          // per context (= per device): the attribute is a per-device property
            for (int h = 0; h <= 4; ++h) {
                IG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(pick_2stage<32, 32, false>(V2_W32{}, 0, h)), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
                if (Kernel2S kk = pick_2stage<32, 32, false, true>(V2_W32_KEEP{}, 0, h))
                    IG_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            }
            ctx->fft_w32_attr = true;
        }
        if (keep_out) k = pick_2stage<32, 32, false, true>(V2_W32_KEEP{}, 0, half);
        if (!k) k = pick_2stage<32, 32, false>(V2_W32{}, 0, half);
    } else {
        IG_REQUIRE(ctx, wmode != 3 || (!axis0 && d.cw >= 1), "ig_fft: the coil-summing pass is a strided pass with a lane split");
        const int wm = wmode == 3 ? 3 + d.cw_log2 : wmode;      // (cw is 1, 2, 4, 8 or 16: it divides the tile's 16 columns)
        with_flag(ax.n == 512, [&](auto n512) { with_flag(axis0, [&](auto a0) {
            constexpr int R1 = decltype(n512)::value ? 32 : 16;
            constexpr bool A0 = decltype(a0)::value;
            if (!boxed && wm == 0) k = &k_fft_2stage<R1, 16, 16, 16, A0, 0, false, 0>;
            else if (wm < 3) {
                if constexpr (!A0) { if (keep_out) k = pick_2stage<R1, 16, false, true>(V2_KEEP{}, wm, half); }
                if (!k) k = pick_2stage<R1, 16, A0>(V2_BOXED{}, wm, half);
            }
            else if constexpr (!A0) k = pick_2stage<R1, 16, false>(V2_SUM{}, wm, half);
        }); });
    }
    IG_REQUIRE(ctx, k, "ig_fft: no two-stage kernel for weight mode %d", wmode);
    hipLaunchKernelGGL(k, grid, block, lds, stream ? stream : ctx->stream, d, ax.d_tw);
    IG_LAUNCH_CHECK(ctx, "k_fft_2stage");
    return IG_OK;
}
