// Dictionary matching: the atom of a dictionary that best explains each voxel's subspace coefficients (indigo_amd.dictmatch,
// Backend.dict_match).
//
// x is a column-major n x nk panel (coefficient image k is column k, ldx >= n), d a column-major nk x na dictionary (atom a is column
// a, ldd >= nk; the caller normalises).  For voxel i with c = x[i, :] and s_a = |d_a^H c|^2, idx[i] is the smallest a that attains
// max_a s_a as computed in float32 and ip[i] = d_a^H c for that a.  The n x na matrix of scores is never written: a (n x nk)(nk x na)
// complex product on the matrix cores with float32 inputs (v_mfma_f32_32x32x2_f32, the second use after ig_cc.hip: exact float32
// products, one rounding per product), fused with a running arg-max per voxel.  8 nk + 12 bytes per voxel.
//
// Real form.  An MFMA step sums over two reals: step k takes Re c[k] (lanes 0..31, k slot 0) and Im c[k] (lanes 32..63, k slot 1) of
// the lane's voxel as its B operand, and as its A operand, for the lane's atom,
//     (Re d[k, a],  Im d[k, a])   which accumulates  Re d_a^H c = sum_k Re d Re c + Im d Im c      (the Re tile)
//     (-Im d[k, a], Re d[k, a])   which accumulates  Im d_a^H c = sum_k Re d Im c - Im d Re c      (the Im tile)
// so each of Re and Im is a chain of 2 nk float32 fmas.  The voxels are on the accumulator's column side: lane (v, h) = (lane & 31,
// lane >> 5) owns voxel v of a group of 32 and, in a tile of 32 atoms, the 16 rows (r & 3) + 8 (r >> 2) + 4 h, r < 16 -- the same
// ones in the Re tile and in the Im tile, so s = re^2 + im^2 and the compare-and-select need no cross-lane traffic.  A lane keeps
// (best s, its atom) over all tiles; rows ascend with r and tiles with a, and only a strictly larger s replaces the best, so a lane
// holds the lowest index of its maximum.  At the very end the two lanes of a voxel exchange (s, index) once (larger s, then lower
// index), read the nk entries of the winning atom and form ip = d_a^H c from their halves of c (one more exchange).
//
// A wave keeps the operands of G groups of 32 voxels in registers (G KP floats per lane, KP = nk or nk rounded up to 16 or 32) for
// the whole sweep over the atoms: x is read once, and every A operand fetched serves 2 G MFMAs.  The dictionary goes through LDS
// in chunks of 64 / KP tiles (32 KB), already in operand form: one ds_read_b64 per lane, tile and step.  The workgroup is four
// waves, 128 G voxels.  Atoms >= na of the last tile and steps k >= nk are literal zeros (nothing is read there): a padded atom
// has s = 0 and an index >= na, and atom 0 -- seen by lane h = 0 before anything else -- has s >= 0, so under the lowest-index rule a
// padded atom never displaces a real one; tiles that lie wholly beyond na are skipped.  Voxels >= n load nothing and store nothing.
// No atomics and a fixed order throughout: two calls give the same bits.
#include "ig_common.h"

namespace {

constexpr int DICT_MAXK = 32;
constexpr int DICT_WAVES = 4;
constexpr int DICT_STEPS = 64;                  // (tiles of a chunk) x KP: 64 steps of 64 lanes x 8 bytes = 32 KB of LDS
constexpr int64_t DICT_MAXGRID = 1 << 20;       // workgroups; the voxel loop strides beyond that

typedef float f32x16_t __attribute__((ext_vector_type(16)));

template <int KP>
struct dict_cfg {
    static constexpr int G = KP <= 8 ? 4 : 2;               // groups of 32 voxels per wave: 32 G accumulators, G KP operands
    static constexpr int CT = DICT_STEPS / KP;              // tiles of a chunk
    static constexpr int VOX = 32 * G * DICT_WAVES;         // voxels of a workgroup
};

template <int KP>
__global__ void __launch_bounds__(64 * DICT_WAVES)
k_dict_match(int64_t n, int nk, int64_t na, const float2* __restrict__ x, int64_t ldx, const float2* __restrict__ d, int64_t ldd,
             int32_t* __restrict__ idx, float2* __restrict__ ip) {
    typedef dict_cfg<KP> cfg;
    __shared__ float2 sd[DICT_STEPS * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int v = lane & 31, h = lane >> 5;
    const int64_t nblocks = (n + cfg::VOX - 1) / cfg::VOX;
    const int64_t nchunks = (na + 32 * cfg::CT - 1) / (32 * cfg::CT);

    for (int64_t blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        const int64_t i0 = blk * cfg::VOX + wave * (32 * cfg::G) + v;       // the lane's voxel of group 0
        float b[cfg::G][KP], best[cfg::G];
        uint32_t arg[cfg::G];
#pragma unroll
        for (int g = 0; g < cfg::G; ++g) {
            const int64_t i = i0 + 32 * g;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                float2 c = make_float2(0.f, 0.f);
                if (i < n && k < nk) c = x[i + (int64_t)k * ldx];
                b[g][k] = h ? c.y : c.x;
            }
            best[g] = -1.f;
            arg[g] = 0u;
        }

        for (int64_t ch = 0; ch < nchunks; ++ch) {
            const int64_t a0 = ch * (32 * cfg::CT);
            __syncthreads();                                                // the previous chunk (or block) has been consumed
            for (int e = threadIdx.x; e < 32 * cfg::CT * KP; e += 64 * DICT_WAVES) {
                const int al = e / KP, k = e - al * KP;
                float2 w = make_float2(0.f, 0.f);
                if (a0 + al < na && k < nk) w = d[k + (a0 + al) * ldd];
                float2* slot = sd + ((al >> 5) * KP + k) * 64 + (al & 31);
                slot[0] = make_float2(w.x, -w.y);                           // k slot 0 meets Re c
                slot[32] = make_float2(w.y, w.x);                           // k slot 1 meets Im c
            }
            __syncthreads();
#pragma unroll 1
            for (int t = 0; t < cfg::CT; ++t) {
                if (a0 + 32 * t >= na) break;                               // (uniform) a tile of padding only
                f32x16_t re[cfg::G], im[cfg::G];
#pragma unroll
                for (int g = 0; g < cfg::G; ++g)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { re[g][r] = 0.f; im[g][r] = 0.f; }
#pragma unroll
                for (int k = 0; k < KP; ++k) {
                    const float2 a = sd[(t * KP + k) * 64 + lane];
#pragma unroll
                    for (int g = 0; g < cfg::G; ++g) {
                        re[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b[g][k], re[g], 0, 0, 0);
                        im[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b[g][k], im[g], 0, 0, 0);
                    }
                }
                const uint32_t row0 = (uint32_t)(a0 + 32 * t) + 4u * h;
#pragma unroll
                for (int g = 0; g < cfg::G; ++g)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float s = fmaf(im[g][r], im[g][r], re[g][r] * re[g][r]);
                        const bool up = s > best[g];
                        best[g] = up ? s : best[g];
                        arg[g] = up ? row0 + (uint32_t)((r & 3) + 8 * (r >> 2)) : arg[g];
                    }
            }
        }

        // the two lanes of a voxel agree on the atom, then each adds its half of d_a^H c
#pragma unroll
        for (int g = 0; g < cfg::G; ++g) {
            const float os = __shfl_xor(best[g], 32);
            const uint32_t oa = (uint32_t)__shfl_xor((int)arg[g], 32);
            uint32_t a = (os > best[g] || (os == best[g] && oa < arg[g])) ? oa : arg[g];
            a = a < (uint32_t)na ? a : (uint32_t)(na - 1);
            const float2* da = d + (int64_t)a * ldd;
            float pre = 0.f, pim = 0.f;
#pragma unroll
            for (int k = 0; k < KP; ++k) {
                if (k < nk) {
                    const float2 w = da[k];
                    pre = fmaf(h ? w.y : w.x, b[g][k], pre);
                    pim = fmaf(h ? w.x : -w.y, b[g][k], pim);
                }
            }
            pre += __shfl_xor(pre, 32);
            pim += __shfl_xor(pim, 32);
            const int64_t i = i0 + 32 * g;
            if (h == 0 && i < n) {
                idx[i] = (int32_t)a;
                ip[i] = make_float2(pre, pim);
            }
        }
    }
}

}  // namespace

int ig_dict_match_c64(ig_ctx* ctx, int64_t n, int64_t nk, int64_t na, const void* x, int64_t ldx, const void* d, int64_t ldd,
                      int32_t* idx, void* ip) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_dict_match_c64: ctx is NULL");
    if (nk < 1 || nk > DICT_MAXK)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_dict_match_c64: %lld coefficients, between 1 and %d are supported", (long long)nk, DICT_MAXK);
    if (na < 1 || na > INT32_MAX)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_dict_match_c64: %lld atoms, between 1 and 2^31 - 1 are supported", (long long)na);
    if (n < 1)
        return ig_fail(ctx, IG_ERR_UNSUPPORTED, "ig_dict_match_c64: %lld voxels, at least 1 is supported", (long long)n);
    IG_REQUIRE(ctx, ldx >= n, "ig_dict_match_c64: leading dimension %lld of x below n = %lld", (long long)ldx, (long long)n);
    IG_REQUIRE(ctx, ldd >= nk, "ig_dict_match_c64: leading dimension %lld of d below nk = %lld", (long long)ldd, (long long)nk);
    IG_REQUIRE(ctx, x && d && idx && ip, "ig_dict_match_c64: NULL pointer");
    const uintptr_t i0 = (uintptr_t)idx, i1 = i0 + (uintptr_t)n * sizeof(int32_t);
    const uintptr_t x0 = (uintptr_t)x, x1 = x0 + (uintptr_t)((nk - 1) * ldx + n) * sizeof(float2);
    const uintptr_t d0 = (uintptr_t)d, d1 = d0 + (uintptr_t)((na - 1) * ldd + nk) * sizeof(float2);
    IG_REQUIRE(ctx, !ig_panels_overlap(ip, n, n, 1, x, ldx, n, nk), "ig_dict_match_c64: ip overlaps x");
    IG_REQUIRE(ctx, !ig_panels_overlap(ip, n, n, 1, d, ldd, nk, na), "ig_dict_match_c64: ip overlaps d");
    IG_REQUIRE(ctx, !ig_bytes_overlap(i0, i1, x0, x1), "ig_dict_match_c64: idx overlaps x");
    IG_REQUIRE(ctx, !ig_bytes_overlap(i0, i1, d0, d1), "ig_dict_match_c64: idx overlaps d");
    IG_REQUIRE(ctx, !ig_bytes_overlap(i0, i1, (uintptr_t)ip, (uintptr_t)ip + (uintptr_t)n * sizeof(float2)), "ig_dict_match_c64: idx overlaps ip");
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, "dict_match", (double)n * (8.0 * (double)nk + 12.0));
#define IG_DICT_GO(KP) hipLaunchKernelGGL((k_dict_match<KP>), ig_grid_1d(n, dict_cfg<KP>::VOX, DICT_MAXGRID), dim3(64 * DICT_WAVES), 0, ctx->stream, \
                                          n, (int)nk, na, (const float2*)x, ldx, (const float2*)d, ldd, idx, (float2*)ip)
    switch (nk) {
        case 1: IG_DICT_GO(1); break;
        case 2: IG_DICT_GO(2); break;
        case 3: IG_DICT_GO(3); break;
        case 4: IG_DICT_GO(4); break;
        case 5: IG_DICT_GO(5); break;
        case 6: IG_DICT_GO(6); break;
        case 7: IG_DICT_GO(7); break;
        case 8: IG_DICT_GO(8); break;
        default: if (nk <= 16) IG_DICT_GO(16); else IG_DICT_GO(32);
    }
#undef IG_DICT_GO
    IG_LAUNCH_CHECK(ctx, "k_dict_match");
    return IG_OK;
}
