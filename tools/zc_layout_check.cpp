// Host check of the z-contiguous y <-> z intermediate (indigo_amd/csrc/ig_fft_zc.h), meant to be built with
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/zc_layout_check.cpp -o zc_layout_check
// and run on the host (tests/test_zc_layout_cpu.py does both).  No GPU, no HIP headers.
//
// For every geometry on the command line -- n0 n1 n2 b2 lo2 coils wy wz, the tile widths of the y and the z pass -- it takes the
// strides the pass descriptors get (zc_side) and walks the array the way the workgroups of k_fft_2stage do: tile origin
// (zc_tile_base) + row step + element step + lane.  Every address a pass forms is checked against the map (zc_offset) and
// written into a buffer of exactly zc_size elements, so an address outside the array is a sanitizer report, and the counts
// show that each pass touches every element exactly once; the z pass's tile must be one contiguous run.
#include "../indigo_amd/csrc/ig_fft_zc.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int fail(const char* what, long long a, long long b, long long c, long long d) {
    std::fprintf(stderr, "zc_layout_check: %s (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
    return 1;
}

static int check(int64_t n0, int64_t n1, int64_t n2, int64_t b2, int64_t lo2, int64_t C, int64_t wy, int64_t wz) {
    const ZcGeom g{n0, n1, b2, C, wz};
    if (!zc_valid(g) || wy > wz || (n0 * C) % wy || lo2 < 0 || lo2 + b2 > n2) return fail("bad geometry", n0, n1, b2, C);
    const int64_t size = zc_size(g), ext0 = n0 * C;
    if (size > n0 * n1 * n2 * C) return fail("larger than the full-size array", size, n0 * n1 * n2 * C, 0, 0);
    const ZcSide sy = zc_side(g, 1), sz = zc_side(g, 2);
    std::vector<unsigned char> hit((size_t)size, 0);
    // the y pass: tiles of wy columns, rows k1 = z', elements j = ky over the whole axis
    for (int64_t tr = 0; tr < ext0 / wy; ++tr)
        for (int64_t zb = 0; zb < b2; ++zb) {
            const int64_t base = zc_tile_base(sy, tr * wy) + zb * sy.s1;
            for (int64_t ky = 0; ky < n1; ++ky)
                for (int64_t w = 0; w < wy; ++w) {
                    const int64_t k0 = tr * wy + w, a = base + ky * sy.sj + w;
                    // (the map itself at a tile's two ends: inside a piece it is linear by construction)
                    if ((w == 0 || w == wy - 1) && a != zc_offset(g, k0 / C, ky, zb, k0 % C)) return fail("y pass address differs from the map", k0, ky, zb, a);
                    hit[(size_t)a] += 1;
                }
        }
    for (int64_t i = 0; i < size; ++i)
        if (hit[(size_t)i] != 1) return fail("y pass: element not touched exactly once", i, hit[(size_t)i], 0, 0);
    // the z pass: tiles of wz columns, rows k1 = ky, elements j = z in the box through a base pre-offset by the box's corner
    for (int64_t tr = 0; tr < ext0 / wz; ++tr)
        for (int64_t ky = 0; ky < n1; ++ky) {
            const int64_t base = -lo2 * sz.sj + zc_tile_base(sz, tr * wz) + ky * sz.s1;
            const int64_t first = base + lo2 * sz.sj;
            for (int64_t z = lo2; z < lo2 + b2; ++z)
                for (int64_t w = 0; w < wz; ++w) {
                    const int64_t k0 = tr * wz + w, a = base + z * sz.sj + w;
                    if ((w == 0 || w == wz - 1) && a != zc_offset(g, k0 / C, ky, z - lo2, k0 % C)) return fail("z pass address differs from the map", k0, ky, z, a);
                    if (a != first + (z - lo2) * wz + w) return fail("z tile is not one contiguous run", k0, ky, z, a);
                    hit[(size_t)a] += 1;
                }
        }
    for (int64_t i = 0; i < size; ++i)
        if (hit[(size_t)i] != 2) return fail("z pass: element not touched exactly once", i, hit[(size_t)i], 0, 0);
    std::printf("ok %lld x %lld x %lld box_z %lld coils %lld tiles %lld/%lld: %lld elements, run of %lld bytes per z tile\n", (long long)n0,
                (long long)n1, (long long)n2, (long long)b2, (long long)C, (long long)wy, (long long)wz, (long long)size, (long long)(b2 * wz * 8));
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 9 || (argc - 1) % 8) {
        std::fprintf(stderr, "usage: zc_layout_check n0 n1 n2 b2 lo2 coils wy wz [n0 n1 ...]\n");
        return 2;
    }
    for (int i = 1; i + 7 < argc; i += 8) {
        int64_t v[8];
        for (int k = 0; k < 8; ++k) v[k] = std::atoll(argv[i + k]);
        if (int rc = check(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7])) return rc;
    }
    return 0;
}
