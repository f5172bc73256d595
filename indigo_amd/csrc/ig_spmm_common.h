// What the sparse-product units (ig_spmm.hip, ig_spmm_bricks.hip, ig_spmm_runs.hip) share.  No kernels here: a kernel template in a
// shared header would be instantiated, and compiled, once per unit.
#pragma once
#include "ig_common.h"
#include <functional>
#include <thread>
#include <type_traits>
#include <vector>

namespace {             // internal to each unit, as in the one file these came from (the kernels' mangled names keep naming it)

constexpr int BLK = 256;
constexpr int WAVES_PER_BLOCK = BLK / 64;

// Blocks are dealt round-robin to the 8 XCDs (each with a private L2).  Give
// each XCD a contiguous range of row blocks so neighbouring rows -- which in
// gridding matrices touch neighbouring panel rows -- share one L2.  Speed
// only; the map is a bijection for every grid size.
__device__ __forceinline__ int64_t xcd_block(int64_t b, int64_t nb) {
    const int64_t q = nb >> 3, rem = nb & 7;
    const int64_t xcd = b & 7, idx = b >> 3;
    return (xcd < rem) ? xcd * (q + 1) + idx : rem * (q + 1) + (xcd - rem) * q + idx;
}

// the brick formats (described above k_grid_bricks in ig_spmm.hip)
struct BrickTask { int32_t lo, hi, bt, nb_flags; };     // entries [lo, hi) = bricks table[bt .. bt + (nb_flags & 0xffff)); bit 16: shared
struct BrickRef { int32_t brick, end; };                  // a non-empty brick and where its entries end
struct BrickEntry { uint32_t cell; float re, im; };       // 12 bytes; cell == 0xffffffff: padding
inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline bool bricks_ok(int64_t n0, int64_t nm, int64_t ns, int bm, int bs, int unit) {
    return n0 > 0 && nm > 0 && ns > 0 && pow2(bm) && pow2(bs) && bm * bs <= 64 && n0 % 16 == 0 && nm % bm == 0 && ns % bs == 0 &&
           pow2(unit) && unit <= 64;
}

// host threads of the format builders: contiguous ranges of rows (or bricks, or runs) per thread
inline int brick_threads(int64_t M) {
    unsigned hw = std::thread::hardware_concurrency();
    int nt = (int)(hw ? hw : 4);
    if (nt > 16) nt = 16;
    if (M < 16384) nt = 1;
    return nt;
}
inline void run_threads(int nt, const std::function<void(int)>& body) {
    if (nt == 1) { body(0); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back([t, &body]() { body(t); });
    for (auto& x : th) x.join();
}

}  // namespace

// X(rows x N, column-major, leading dimension ldx; row k = panel row xperm[k] if given) -> *packed[rows][np], np = the power of two
// >= N (<= 64), in the context's repack scratch, which only grows.  may_decline: *packed = nullptr and IG_OK when the scratch would
// exceed a quarter of the free device memory or 16 GiB, or cannot be allocated; otherwise a failed allocation is an error.
int ig_pack_panel(ig_ctx* ctx, int64_t rows, int64_t N, int np, const float2* X, int64_t ldx, const int32_t* xperm,
                  bool may_decline, const float2** packed);
