// The y <-> z intermediate of the coil-interleaved grid layout (layout 2), stored z-contiguous per kx tile.
//
// Between its y and its z pass a zero-padded / cropped transform keeps an array nobody else sees: n0 x n1 x b2 points (full
// along x and y, the image box along z) times C interleaved coils.  In the grid's own order -- (c, kx) fastest, then kz, then
// ky -- a z-pass tile of `piece` columns reads (padded) or writes (cropped) b2 pieces that lie n0 * C elements apart, and the
// y pass steps n0 * n2 * C elements (16 MB on the 512^3 x 8 grid) from one ky to the next.  Stored as
//
//     [kx tile q][ky][z'][e]        k0 = c + C * kx = q * piece + e,   z' = z - box_lo[2]
//
// the dense side of a z tile is ONE run of b2 * piece elements, and the y pass steps b2 * piece elements per ky inside a region
// of n1 * b2 * piece elements per tile.  Every (kx, ky) column keeps its slot whether the support table flags it or not: the
// addresses are closed-form and the array is n0 * n1 * b2 * C elements, never more than the full-size array it replaces.
//
// Host code only, no dependency on the HIP headers: ig_fft_plan.hip builds the pass descriptors of the y and z passes from zc_side,
// ig_fft_zc_offset / ig_fft_zc_size export the map, and tools/zc_layout_check.cpp walks it under the sanitizers.
#pragma once
#include <cstdint>

struct ZcGeom {
    int64_t n0, n1, b2, C;       // grid points along x and y, image planes along z, interleaved coils
    int64_t piece;               // columns (c, kx) per piece = the tile width of the z pass (16 or 32); divides n0 * C
};

static inline bool zc_valid(const ZcGeom& z) {
    return z.n0 >= 1 && z.n1 >= 1 && z.b2 >= 1 && z.C >= 1 && z.piece >= 1 && (z.piece & (z.piece - 1)) == 0 && (z.n0 * z.C) % z.piece == 0;
}

static inline int64_t zc_size(const ZcGeom& z) { return z.n0 * z.C * z.n1 * z.b2; }                  // elements

// element offset of coil c of the point (kx, ky, z') -- z' counted from the box's first plane
static inline int64_t zc_offset(const ZcGeom& z, int64_t kx, int64_t ky, int64_t zb, int64_t c) {
    const int64_t k0 = c + z.C * kx, q = k0 / z.piece, e = k0 - q * z.piece;
    return ((q * z.n1 + ky) * z.b2 + zb) * z.piece + e;
}

// What a strided pass over the array takes (PassDesc, ig_fft_ab.h): the element steps along the transform axis (sj) and along
// the row axis k1 (s1: z' for the y pass, ky for the z pass), and from one piece to the next (zt); lanes run at unit stride
// inside a piece.  All of them differences of zc_offset.
struct ZcSide { int64_t sj, s1, zt; int piece_log2; };

static inline ZcSide zc_side(const ZcGeom& z, int axis /* 1: the y pass, 2: the z pass */) {
    const int64_t o = zc_offset(z, 0, 0, 0, 0), dy = zc_offset(z, 0, 1 % z.n1, 0, 0) - o, dz = zc_offset(z, 0, 0, 1 % z.b2, 0) - o;
    // (an axis of one point has no step: any value serves)
    const int64_t sy = z.n1 > 1 ? dy : z.b2 * z.piece, sz = z.b2 > 1 ? dz : z.piece;
    ZcSide s{};
    s.sj = axis == 1 ? sy : sz;
    s.s1 = axis == 1 ? sz : sy;
    s.zt = z.n1 * z.b2 * z.piece;
    s.piece_log2 = 0;
    while ((int64_t(1) << s.piece_log2) < z.piece) ++s.piece_log2;
    return s;
}

// the element offset of column k0 = tile * W + lane of a pass tile of W <= piece columns, as k_fft_2stage forms it: the
// workgroup's base (wave-uniform) plus the lane
static inline int64_t zc_tile_base(const ZcSide& s, int64_t k0u) {
    return (k0u >> s.piece_log2) * s.zt + (k0u & ((int64_t(1) << s.piece_log2) - 1));
}
