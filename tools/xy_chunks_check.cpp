// Host check of the partition of the chunked x <-> y pair (indigo_amd/csrc/ig_fft_xy.h), meant to be built with
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/xy_chunks_check.cpp -o xy_chunks_check
// and run on the host (tests/test_xy_chunks_cpu.py does both).  No GPU, no HIP headers.
//
//   xy_chunks_check [max_planes]        (default 300)
//
// For every number of planes 1 ... max_planes, every K from 0 to planes + 1, every S from 1 to 3 and two origins z0 it walks the
// chunks the way exec_padded / exec_cropped do and marks every plane in a buffer of exactly `planes` bytes: a chunk outside the range
// is a sanitizer report, and the counts show that the chunks tile [z0, z1) exactly once, in order, none of them empty, the last one
// alone ragged, on streams below S that alternate.  K = 0 and K >= planes are one chunk on stream 0; an empty range has no chunk.
#include "../indigo_amd/csrc/ig_fft_xy.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int fail(const char* what, long long planes, long long K, long long S, long long i) {
    std::fprintf(stderr, "xy_chunks_check: %s (planes %lld, K %lld, S %lld, chunk %lld)\n", what, planes, K, S, i);
    return 1;
}

static int check(int64_t z0, int64_t planes, int64_t K, int S) {
    const int64_t z1 = z0 + planes;
    const XyChunks p = xy_chunks(z0, z1, K, S);
    if (p.count < 1) return fail("no chunk for a range that has planes", planes, K, S, 0);
    if (p.S < 1 || p.S > S || p.S > XY_MAX_STREAMS || p.S > p.count) return fail("streams in use outside [1, min(S, chunks)]", planes, K, S, p.S);
    if ((K <= 0 || K >= planes) && (p.count != 1 || p.S != 1)) return fail("K = 0 or K >= planes is not one chunk on one stream", planes, K, S, p.count);
    if (K > 0 && K < planes && p.count != (planes + K - 1) / K) return fail("chunk count is not ceil(planes / K)", planes, K, S, p.count);
    std::vector<unsigned char> hit((size_t)planes, 0);
    int64_t next = z0;
    for (int64_t i = 0; i < p.count; ++i) {
        const XyChunk c = xy_chunk(p, i);
        if (c.nz < 1) return fail("empty chunk", planes, K, S, i);
        if (c.z0 != next) return fail("chunk does not start where the last one ended", planes, K, S, i);
        if (i + 1 < p.count && K > 0 && c.nz != K) return fail("a chunk before the last is not K planes", planes, K, S, i);
        if (c.stream < 0 || c.stream >= S || c.stream >= p.S) return fail("stream index out of range", planes, K, S, i);
        if (c.stream != (int)(i % p.S)) return fail("chunk i is not on stream i mod S", planes, K, S, i);
        for (int64_t z = c.z0; z < c.z0 + c.nz; ++z) hit[(size_t)(z - z0)] += 1;          // (out of range: the sanitizer reports it)
        next = c.z0 + c.nz;
    }
    if (next != z1) return fail("chunks do not end at z1", planes, K, S, p.count);
    for (int64_t z = 0; z < planes; ++z)
        if (hit[(size_t)z] != 1) return fail("plane not covered exactly once", planes, K, S, z);
    return 0;
}

int main(int argc, char** argv) {
    const int64_t max_planes = argc > 1 ? std::atoll(argv[1]) : 300;
    if (max_planes < 1) { std::fprintf(stderr, "usage: xy_chunks_check [max_planes >= 1]\n"); return 2; }
    long long cases = 0;
    for (int64_t planes = 1; planes <= max_planes; ++planes)
        for (int64_t K = 0; K <= planes + 1; ++K)
            for (int S = 1; S <= 3; ++S)
                for (int64_t z0 : {int64_t(0), int64_t(7)}) {
                    if (int rc = check(z0, planes, K, S)) return rc;
                    ++cases;
                }
    // an empty or reversed range has no chunk at all; S beyond the limit is clamped
    for (int64_t K : {int64_t(0), int64_t(1), int64_t(5)}) {
        if (xy_chunks(4, 4, K, 2).count != 0 || xy_chunks(9, 4, K, 2).count != 0) return fail("an empty range has chunks", 0, K, 2, 0);
    }
    // the automatic chunk: the fewest planes that reach 128 MiB (16 of the 512^3 x 8 grid's 8 MiB planes), never zero for a real plane
    if (xy_auto_planes(int64_t(512) * 256 * 8 * 8) != 16 || xy_auto_planes(int64_t(256) * 128 * 8 * 8) != 64 || xy_auto_planes(int64_t(512) * 320 * 8 * 8) != 13)
        return fail("automatic planes per chunk", 0, 0, 0, 0);
    for (int64_t pb = 8; pb <= (int64_t(1) << 31); pb = pb * 3 + 8) {
        const int64_t K = xy_auto_planes(pb);
        if (K < 1 || K * pb < XY_AUTO_CHUNK_BYTES || (K - 1) * pb >= XY_AUTO_CHUNK_BYTES) return fail("automatic planes per chunk are not the fewest that reach the size", pb, K, 0, 0);
    }
    if (xy_auto_planes(0) != 0) return fail("a plane of no bytes has automatic planes", 0, 0, 0, 0);
    if (xy_chunks(0, 100, 1, 9).S != XY_MAX_STREAMS || xy_chunks(0, 100, 1, 0).S != 1) return fail("S is not clamped", 100, 1, 9, 0);
    std::printf("ok %lld partitions up to %lld planes\n", cases, (long long)max_planes);
    return 0;
}
