// Context, memory, copies, events.
// Counterpart of the bring-up + dndarray plumbing in the reference's CUDA
// backend (indigo/backends/cuda.py:28-38,126-181) -- written against the HIP
// runtime for gfx950, not translated from it.
#include "ig_common.h"
#include <cstring>

std::string& ig_tls_error() {
    static thread_local std::string e;
    return e;
}

int ig_fail(ig_ctx* ctx, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    ig_tls_error() = buf;
    if (ctx) ctx->err = buf;
    return code;
}

extern "C" {

int ig_abi_version(void) { return IG_ABI_VERSION; }

int ig_device_count(int* count) {
    if (!count) return ig_fail(nullptr, IG_ERR_ARG, "ig_device_count: count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { n = 0; (void)hipGetLastError(); }
    *count = n;
    return IG_OK;
}

static int ig_init_common(int device_id, bool adopt, void* ext_stream, ig_ctx** out) {
    if (!out) return ig_fail(nullptr, IG_ERR_ARG, "ig_init: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return ig_fail(nullptr, IG_ERR_NODEVICE,
                       "ig_init: no HIP device available (%s); this library has no CPU fallback",
                       e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    }
    if (device_id < 0 || device_id >= n)
        return ig_fail(nullptr, IG_ERR_ARG, "ig_init: device_id %d out of range [0,%d)", device_id, n);

    ig_ctx* ctx = new ig_ctx();
    ctx->device = device_id;
    auto bail = [&](const char* what, hipError_t err) {
        int rc = ig_fail(nullptr, IG_ERR_HIP, "ig_init: %s failed: %s", what, hipGetErrorString(err));
        if (ctx->d_partials) (void)hipFree(ctx->d_partials);
        if (ctx->h_result) (void)hipHostFree(ctx->h_result);
        if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
        delete ctx;
        return rc;
    };
    if ((e = hipSetDevice(device_id)) != hipSuccess) return bail("hipSetDevice", e);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) return bail("hipGetDeviceProperties", e);
    ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (adopt) {
        ctx->stream = (hipStream_t)ext_stream;
        ctx->own_stream = false;
    } else {
        if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess)
            return bail("hipStreamCreateWithFlags", e);
        ctx->own_stream = true;
    }
    ctx->partials_bytes = sizeof(double) * 2 * (IG_MAX_RED_BLOCKS + 1);
    if ((e = hipMalloc((void**)&ctx->d_partials, ctx->partials_bytes)) != hipSuccess)
        return bail("hipMalloc(partials)", e);
    if ((e = hipHostMalloc((void**)&ctx->h_result, sizeof(double) * 2, hipHostMallocDefault)) != hipSuccess)
        return bail("hipHostMalloc(result)", e);
    *out = ctx;
    return IG_OK;
}

int ig_init(int device_id, ig_ctx** out) { return ig_init_common(device_id, false, nullptr, out); }

int ig_init_on_stream(int device_id, void* hip_stream, ig_ctx** out) {
    return ig_init_common(device_id, true, hip_stream, out);
}

void ig_destroy(ig_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (ig_prof_rec& r : ctx->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (hipEvent_t e : ctx->prof_pool) (void)hipEventDestroy(e);
    if (ctx->d_partials) (void)hipFree(ctx->d_partials);
    if (ctx->d_scalars) (void)hipFree(ctx->d_scalars);
    if (ctx->d_worklist) (void)hipFree(ctx->d_worklist);
    if (ctx->d_xpack) (void)hipFree(ctx->d_xpack);
    if (ctx->d_epg) (void)hipFree(ctx->d_epg);
    if (ctx->h_result) (void)hipHostFree(ctx->h_result);
    for (int i = 0; i < 2; ++i) {          // (their work was joined into ctx->stream, which has been synchronised)
        if (ctx->xy_stream[i]) (void)hipStreamDestroy(ctx->xy_stream[i]);
        if (ctx->xy_join[i]) (void)hipEventDestroy(ctx->xy_join[i]);
    }
    if (ctx->xy_fork) (void)hipEventDestroy(ctx->xy_fork);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* ig_last_error(ig_ctx* ctx) {
    if (ctx) return ctx->err.c_str();
    return ig_tls_error().c_str();
}

int ig_sync(ig_ctx* ctx) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_sync: ctx is NULL");
    if (int rc = ig_set_device(ctx)) return rc;
    IG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return IG_OK;
}

void* ig_stream(ig_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

// ---- recorded launch sequences (HIP graphs) --------------------------------------------------------------------------
int ig_graph_begin(ig_ctx* ctx) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_graph_begin: ctx is NULL");
    IG_REQUIRE(ctx, !ctx->capturing, "ig_graph_begin: already recording");
    IG_REQUIRE(ctx, !ctx->prof_on, "ig_graph_begin: profile mode brackets launches with events of its own; switch it off");
    if (int rc = ig_set_device(ctx)) return rc;
    // thread-local mode: only this thread's unsafe calls (allocations, synchronisations) invalidate the recording
    IG_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    ctx->capturing = true;
    return IG_OK;
}

int ig_graph_end(ig_ctx* ctx, ig_graph** out) {
    IG_REQUIRE(ctx, ctx && out, "ig_graph_end: bad arguments");
    IG_REQUIRE(ctx, ctx->capturing, "ig_graph_end: not recording");
    *out = nullptr;
    ctx->capturing = false;
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamEndCapture(ctx->stream, &g);
    if (e != hipSuccess || !g) {
        (void)hipGetLastError();
        if (g) (void)hipGraphDestroy(g);
        return ig_fail(ctx, IG_ERR_HIP, "ig_graph_end: the recording is invalid (%s): a call inside it synchronised or allocated",
                       hipGetErrorString(e));
    }
    hipGraphExec_t x = nullptr;
    e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)hipGraphDestroy(g);
        return ig_fail(ctx, IG_ERR_HIP, "ig_graph_end: hipGraphInstantiate failed: %s", hipGetErrorString(e));
    }
    ig_graph* r = new ig_graph();
    r->ctx = ctx; r->graph = g; r->exec = x;
    *out = r;
    return IG_OK;
}

int ig_graph_abort(ig_ctx* ctx) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_graph_abort: ctx is NULL");
    if (!ctx->capturing) return IG_OK;
    ctx->capturing = false;
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture(ctx->stream, &g);
    (void)hipGetLastError();
    if (g) (void)hipGraphDestroy(g);
    return IG_OK;
}

int ig_graph_launch(ig_graph* graph) {
    IG_REQUIRE(nullptr, graph && graph->ctx && graph->exec, "ig_graph_launch: bad graph");
    ig_ctx* ctx = graph->ctx;
    IG_REQUIRE(ctx, !ctx->capturing, "ig_graph_launch: the context is recording");
    if (int rc = ig_set_device(ctx)) return rc;
    IG_HIP(ctx, hipGraphLaunch(graph->exec, ctx->stream));
    return IG_OK;
}

int ig_graph_destroy(ig_graph* graph) {
    if (!graph) return IG_OK;
    if (graph->exec) (void)hipGraphExecDestroy(graph->exec);
    if (graph->graph) (void)hipGraphDestroy(graph->graph);
    delete graph;
    return IG_OK;
}

int ig_device_name(ig_ctx* ctx, char* buf, size_t len) {
    IG_REQUIRE(ctx, ctx && buf && len > 0, "ig_device_name: bad arguments");
    hipDeviceProp_t prop;
    IG_HIP(ctx, hipGetDeviceProperties(&prop, ctx->device));
    snprintf(buf, len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return IG_OK;
}

int ig_set_option(ig_ctx* ctx, const char* name, int64_t value) {
    IG_REQUIRE(ctx, ctx && name, "ig_set_option: bad arguments");
    if (std::string(name) == "fft.kernels") {
        IG_REQUIRE(ctx, value >= 0 && value <= 2, "ig_set_option: fft.kernels is 0 (all), 1 (no A x B passes) or 2 (generic stages only)");
        ctx->opt_fft_kernels = (int)value;
        return IG_OK;
    }
    if (std::string(name) == "fft.zc_intermediate") {
        IG_REQUIRE(ctx, value == 0 || value == 1, "ig_set_option: fft.zc_intermediate is 0 (the grid's order) or 1 (z-contiguous per kx tile)");
        ctx->opt_fft_zc = (int)value;
        return IG_OK;
    }
    if (std::string(name) == "fft.xy_chunk_planes") {
        IG_REQUIRE(ctx, value >= -1 && value <= 0x7fffffffLL, "ig_set_option: fft.xy_chunk_planes is 0 (one launch per pass), the image planes per chunk of the x / y pair, or -1 (chunks of 128 MiB)");
        ctx->opt_fft_xy_planes = (int)value;
        return IG_OK;
    }
    if (std::string(name) == "fft.xy_chunk_streams") {
        IG_REQUIRE(ctx, value >= 1 && value <= 3, "ig_set_option: fft.xy_chunk_streams is 1, 2 or 3 (the context's stream and up to two more)");
        ctx->opt_fft_xy_streams = (int)value;
        return IG_OK;
    }
    return ig_fail(ctx, IG_ERR_ARG, "ig_set_option: unknown option '%s'", name);
}

int ig_library_bytes(ig_ctx* ctx, size_t* bytes) {
    IG_REQUIRE(ctx, ctx && bytes, "ig_library_bytes: bad arguments");
    // device memory the library itself holds for this context: the repacked-panel buffer of the SpMM kernels (grown on
    // demand), the pulse program of the EPG simulation, the deferred-row lists, the reduction scratch and the solver scalars
    // (the byte counts are recorded where the buffers are allocated)
    *bytes = ctx->xpack_bytes + ctx->epg_bytes + (ctx->d_worklist ? ctx->worklist_bytes : 0) + (ctx->d_partials ? ctx->partials_bytes : 0) +
             (ctx->d_scalars ? ctx->scalars_bytes : 0);
    return IG_OK;
}

int ig_mem_info(ig_ctx* ctx, size_t* free_bytes, size_t* total_bytes) {
    IG_REQUIRE(ctx, ctx && free_bytes && total_bytes, "ig_mem_info: bad arguments");
    if (int rc = ig_set_device(ctx)) return rc;
    IG_HIP(ctx, hipMemGetInfo(free_bytes, total_bytes));
    return IG_OK;
}

// ---- memory -----------------------------------------------------------------

int ig_malloc(ig_ctx* ctx, size_t nbytes, void** dptr) {
    IG_REQUIRE(ctx, ctx && dptr, "ig_malloc: bad arguments");
    if (int rc = ig_set_device(ctx)) return rc;
    *dptr = nullptr;
    // hipMalloc returns >=256-byte aligned memory; never hand out NULL for an empty array
    size_t n = nbytes ? nbytes : 256;
    hipError_t e = hipMalloc(dptr, n);
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return ig_fail(ctx, IG_ERR_NOMEM, "ig_malloc: out of device memory requesting %zu bytes", nbytes);
    }
    if (e != hipSuccess) return ig_fail(ctx, IG_ERR_HIP, "hipMalloc(%zu) failed: %s", nbytes, hipGetErrorString(e));
    return IG_OK;
}

// Placement probe (round 5): the passes that step megabytes per element (the y passes of the coil-interleaved grid:
// 512 rows of 256-byte segments 16 MB apart) run 3 ... 6 % slower on some allocations than on others of the same size made by the
// same process -- the same kernel on six hipMalloc'ed buffers: 1.61 ms on three, 1.66 ... 1.70 on the others, repeatably; two runs of
// the benchmark on one box differed by exactly that.  This writes zeros over the buffer in that pattern (512 rows of nbytes / 512,
// in tiles of 256-byte segments) and reports the time of the fastest of three passes; the backend allocates a few candidates for its
// large arrays and keeps the best (HipBackend.tuning['placement_candidates']).  The buffer's contents are destroyed.
namespace {
__global__ void __launch_bounds__(512)
k_probe_placement(float4* __restrict__ p, size_t pitch16 /* row pitch in float4 */) {
    const size_t tile = blockIdx.x;
    const int lane = threadIdx.x & 15, row0 = threadIdx.x >> 4;
#pragma unroll
    for (int s = 0; s < 16; ++s)
        p[(size_t)(row0 + 32 * s) * pitch16 + tile * 16 + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
}
}   // namespace

int ig_probe_placement(ig_ctx* ctx, void* dptr, size_t nbytes, double* ms) {
    IG_REQUIRE(ctx, ctx && ms, "ig_probe_placement: bad arguments");
    IG_REQUIRE(ctx, !ctx->capturing, "ig_probe_placement: not while a graph is being recorded (the probe synchronises the stream)");
    *ms = 0.0;
    const size_t pitch = (nbytes / 512) & ~(size_t)4095;
    if (!dptr || pitch == 0) return IG_OK;                     // too small to have such a pattern
    if (int rc = ig_set_device(ctx)) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    IG_HIP(ctx, hipEventCreate(&e0));
    hipError_t err = hipEventCreate(&e1);
    float best = 1e30f;
    for (int rep = 0; rep < 4 && err == hipSuccess; ++rep) {
        err = hipEventRecord(e0, ctx->stream);
        if (err != hipSuccess) break;
        hipLaunchKernelGGL(k_probe_placement, dim3((unsigned)(pitch / 256)), dim3(512), 0, ctx->stream, (float4*)dptr, pitch / 16);
        if ((err = hipGetLastError()) != hipSuccess) break;                                 // (the launch itself, checked on the spot)
        if ((err = hipEventRecord(e1, ctx->stream)) != hipSuccess) break;
        if ((err = hipEventSynchronize(e1)) != hipSuccess) break;
        float t = 0.f;
        if ((err = hipEventElapsedTime(&t, e0, e1)) != hipSuccess) break;
        if (rep && t < best) best = t;
    }
    (void)hipEventDestroy(e0);                                 // (on every path: the events do not outlive the call)
    if (e1) (void)hipEventDestroy(e1);
    if (err != hipSuccess) return ig_fail(ctx, IG_ERR_HIP, "ig_probe_placement: %s", hipGetErrorString(err));
    *ms = best;
    return IG_OK;
}

int ig_free(ig_ctx* ctx, void* dptr) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_free: ctx is NULL");
    if (!dptr) return IG_OK;
    if (int rc = ig_set_device(ctx)) return rc;
    // work queued on our (non-blocking) stream may still use the buffer
    IG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    IG_HIP(ctx, hipFree(dptr));
    return IG_OK;
}

int ig_memset0(ig_ctx* ctx, void* dptr, size_t nbytes) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_memset0: ctx is NULL");
    if (nbytes == 0) return IG_OK;
    IG_REQUIRE(ctx, dptr != nullptr, "ig_memset0: NULL pointer");
    if (int rc = ig_set_device(ctx)) return rc;
    IG_HIP(ctx, hipMemsetAsync(dptr, 0, nbytes, ctx->stream));
    return IG_OK;
}

int ig_copy2d(ig_ctx* ctx, void* dst, size_t dpitch, const void* src, size_t spitch,
              size_t width_bytes, size_t height, int kind) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_copy2d: ctx is NULL");
    if (width_bytes == 0 || height == 0) return IG_OK;
    IG_REQUIRE(ctx, dst && src, "ig_copy2d: NULL pointer");
    IG_REQUIRE(ctx, height == 1 || (dpitch >= width_bytes && spitch >= width_bytes),
               "ig_copy2d: pitch smaller than row width");
    hipMemcpyKind k;
    switch (kind) {
        case IG_H2D: k = hipMemcpyHostToDevice; break;
        case IG_D2H: k = hipMemcpyDeviceToHost; break;
        case IG_D2D: k = hipMemcpyDeviceToDevice; break;
        default: return ig_fail(ctx, IG_ERR_ARG, "ig_copy2d: unknown kind %d", kind);
    }
    if (int rc = ig_set_device(ctx)) return rc;
    const bool dense = (height == 1) || (dpitch == width_bytes && spitch == width_bytes);
    if (dense) {
        IG_HIP(ctx, hipMemcpyAsync(dst, src, width_bytes * height, k, ctx->stream));
    } else {
        IG_HIP(ctx, hipMemcpy2DAsync(dst, dpitch, src, spitch, width_bytes, height, k, ctx->stream));
    }
    if (kind != IG_D2D) IG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return IG_OK;
}

// ---- events -----------------------------------------------------------------

int ig_event_create(ig_ctx* ctx, ig_event** out) {
    IG_REQUIRE(ctx, ctx && out, "ig_event_create: bad arguments");
    if (int rc = ig_set_device(ctx)) return rc;
    ig_event* ev = new ig_event();
    ev->ctx = ctx;
    hipError_t e = hipEventCreate(&ev->ev);
    if (e != hipSuccess) { delete ev; return ig_fail(ctx, IG_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(e)); }
    *out = ev;
    return IG_OK;
}

int ig_event_record(ig_event* ev) {
    if (!ev) return ig_fail(nullptr, IG_ERR_ARG, "ig_event_record: NULL event");
    ig_ctx* ctx = ev->ctx;
    if (int rc = ig_set_device(ctx)) return rc;
    IG_HIP(ctx, hipEventRecord(ev->ev, ctx->stream));
    return IG_OK;
}

int ig_event_elapsed_ms(ig_event* start, ig_event* stop, float* ms) {
    if (!start || !stop || !ms) return ig_fail(nullptr, IG_ERR_ARG, "ig_event_elapsed_ms: bad arguments");
    ig_ctx* ctx = stop->ctx;
    if (int rc = ig_set_device(ctx)) return rc;
    IG_HIP(ctx, hipEventSynchronize(stop->ev));
    IG_HIP(ctx, hipEventElapsedTime(ms, start->ev, stop->ev));
    return IG_OK;
}

int ig_prof_enable(ig_ctx* ctx, int on) {
    IG_REQUIRE(ctx, ctx != nullptr, "ig_prof_enable: ctx is NULL");
    ctx->prof_on = on != 0;
    return IG_OK;
}

int ig_prof_report(ig_ctx* ctx, char* buf, size_t len) {
    IG_REQUIRE(ctx, ctx && buf && len > 0, "ig_prof_report: bad arguments");
    if (int rc = ig_set_device(ctx)) return rc;
    IG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    struct Acc { const char* name; long n; double ms; double bytes; };
    std::vector<Acc> acc;
    for (const ig_prof_rec& r : ctx->prof) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) { (void)hipGetLastError(); ms = 0.f; }
        Acc* a = nullptr;
        for (Acc& c : acc) if (strcmp(c.name, r.name) == 0) { a = &c; break; }
        if (!a) { acc.push_back(Acc{r.name, 0, 0.0, 0.0}); a = &acc.back(); }
        a->n += 1; a->ms += ms; a->bytes += r.bytes;
        ctx->prof_pool.push_back(r.e0);
        ctx->prof_pool.push_back(r.e1);
    }
    ctx->prof.clear();
    size_t off = 0;
    buf[0] = 0;
    for (const Acc& a : acc) {
        int w = snprintf(buf + off, len - off, "%s %ld %.6f %.0f\n", a.name, a.n, a.ms, a.bytes);
        if (w < 0 || (size_t)w >= len - off) break;
        off += (size_t)w;
    }
    return IG_OK;
}

int ig_event_destroy(ig_event* ev) {
    if (!ev) return IG_OK;
    (void)hipSetDevice(ev->ctx->device);
    (void)hipEventDestroy(ev->ev);
    delete ev;
    return IG_OK;
}

}  // extern "C"
