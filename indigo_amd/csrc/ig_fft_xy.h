// The x <-> y pair of the coil-interleaved grid layout (layout 2), run in chunks of image planes.
//
// Between its x and its y pass a zero-padded / cropped transform keeps `mid`: n0 x b1 x b2 points times C interleaved coils, stored
// plane by plane along z'.  Both passes are independent per image plane, so instead of x(all planes) then y(all planes) the pair can
// run as x(chunk) -> y(chunk) over chunks of K planes (cropped: y then x), chunk i on stream i mod S.  What a chunk's second pass
// reads was written a few launches earlier, while it may still sit in the last-level cache; nothing else changes -- the same kernels
// over the same addresses, ordered by stream order alone.  (plan options "fft.xy_chunk_planes" = K, "fft.xy_chunk_streams" = S)
//
// This header is the partition only: which planes a chunk covers and which stream it runs on.  Host code, no dependency on the HIP
// headers: ig_fft_plan.hip walks it to launch, tools/xy_chunks_check.cpp walks it under the sanitizers.
#pragma once
#include <cstdint>

constexpr int XY_MAX_STREAMS = 3;      // the context's own stream and two more: a process has four hardware queues

struct XyChunks {
    int64_t z0, z1;          // the image planes [z0, z1) the pair covers
    int64_t K;               // planes per chunk (the last one may be shorter); z1 - z0 where the pair runs unchunked
    int64_t count;           // chunks: 0 for an empty range
    int S;                   // streams in use: 1 ... min(XY_MAX_STREAMS, count)
};

struct XyChunk { int64_t z0, nz; int stream; };

// The planes per chunk of the automatic setting (option value -1): the fewest whose share of the intermediate reaches 128 MiB.
// Measured: chunks of about that size pay -- 16 planes of the 512^3 x 8 grid's 8 MiB planes, 64 of the
// 256^3 x 8 grid's 2 MiB planes -- smaller ones lose more to their launches than they gain, larger ones fall out of the cache.
constexpr int64_t XY_AUTO_CHUNK_BYTES = int64_t(128) << 20;
static inline int64_t xy_auto_planes(int64_t plane_bytes) {
    return plane_bytes <= 0 ? 0 : (XY_AUTO_CHUNK_BYTES + plane_bytes - 1) / plane_bytes;
}

// K <= 0 or K >= planes: one chunk, today's two launches.  S is clamped to [1, XY_MAX_STREAMS] and to the number of chunks.
static inline XyChunks xy_chunks(int64_t z0, int64_t z1, int64_t K, int S) {
    XyChunks p{z0, z1, 0, 0, 1};
    const int64_t planes = z1 - z0;
    if (planes <= 0) return p;
    p.K = (K <= 0 || K >= planes) ? planes : K;
    p.count = (planes + p.K - 1) / p.K;
    p.S = S < 1 ? 1 : S > XY_MAX_STREAMS ? XY_MAX_STREAMS : S;
    if (p.S > p.count) p.S = (int)p.count;
    return p;
}

// chunk i of 0 ... count - 1
static inline XyChunk xy_chunk(const XyChunks& p, int64_t i) {
    const int64_t lo = p.z0 + i * p.K, hi = lo + p.K < p.z1 ? lo + p.K : p.z1;
    return XyChunk{lo, hi - lo, (int)(i % p.S)};
}
