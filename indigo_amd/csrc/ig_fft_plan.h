// What the FFT units share: the plan structures, and the host functions that cross units.  No kernels here.
//   ig_fft.hip        k_fft_2stage (every pass of the SENSE path) and its launch
//   ig_fft_plain.hip  the kernels off that path (two-launch 256^3, LDS, generic stage, unfused chirp-z steps), one launch function each
//   ig_fft_plan.hip   planning, execution, the zero-padded / cropped pass schedule and the C ABI: host code only
//   ig_fft_regs.h     the register DFT building blocks of the kernels in the first two
#pragma once
#include "ig_common.h"
#include "ig_fft_ab.h"
#include <memory>
#include <string>
#include <vector>

namespace {             // internal to each unit, as in the one file these came from (k_fft_lds's mangled name keeps naming it)

constexpr int MAX_STAGES = 16;
constexpr int E = 8;                 // complex elements a thread holds per LDS stage
constexpr int LDS_NMAX = 4096;
constexpr size_t LDS_BUDGET = 150 * 1024;

struct Radices { int r[MAX_STAGES]; };

}  // namespace

// AxisPlan (and with it Chirp and ig_fft) holds a Radices, which is a type of its own in every unit: formally each unit defines its own
// AxisPlan, and they agree only because this header gives all of them the same layout.  Accepted knowingly, for k_fft_lds's name.  Define
// these structs nowhere else, keep them free of anything a unit could see differently (no #if, no unit-local types beyond Radices), and
// do not build the FFT units in a way that merges or compares types across units (LTO with ODR checking).
struct Chirp;
struct AxisPlan {
    int64_t n = 1, inner = 1, outer = 1;
    int kind = 2;                      // 0 LDS kernel, 1 generic stages, 2 nothing to do (n == 1), 3 two-stage (256, 512), 4 two-stage A x B,
                                       // 5 chirp-z (Bluestein) over a smooth length m >= 2 n - 1: lengths with a prime factor > 7
    std::shared_ptr<Chirp> chirp;      // kind 5
    int nstages = 0;
    int ab_A = 0, ab_B = 0;            // kind 4: n = A * B (ig_fft_ab.h)
    Radices rad{};
    std::vector<int64_t> gen_radices;  // generic path may carry large prime radices
    int W = 16, T = 1;
    size_t lds_bytes = 0;
    float2* d_tw = nullptr;
};

// Bluestein: X_k = b_k sum_j (x_j b_j) conj(b)_{k-j}, b_j = exp(-i pi j^2 / n) -- a cyclic convolution of length m >= 2 n - 1, done
// with two transforms of a length the fast kernels have.  Tables for both directions (the inverse's are the conjugates):
//   b[dir]    m entries: the chirp (input weights; only j < n is ever read)
//   bhat[dir] m entries: F_m of the wrapped conjugate chirp (the convolution kernel in the frequency domain)
//   bout[dir] m entries: b_k / m (output weights of the inverse sub-transform, which is unnormalised)
struct Chirp {
    int64_t m = 0;
    float2* d_b[2] = {nullptr, nullptr};
    float2* d_bhat[2] = {nullptr, nullptr};
    float2* d_bout[2] = {nullptr, nullptr};
    float2* d_hat_out[2] = {nullptr, nullptr};     // bhat then bout in one array (the one-launch kernel's second table)
    // (round 6) the tables of the one-launch kernel for a transform that carries a circular shift by `shift` points on its image side
    // (ig_fft_set_axis_shift): input weights, then [transformed kernel, output weights / m]
    int64_t shift = 0;
    float2* d_in_s[2] = {nullptr, nullptr};
    float2* d_hat_out_s[2] = {nullptr, nullptr};
    AxisPlan sub;                      // the length-m axis with this axis's inner / outer extents
    bool fused = false;                // ONE launch per pass (k_fft_chirp: both length-m transforms in registers / LDS; strided axes, m = A x B)
    ~Chirp() {
        for (int d = 0; d < 2; ++d) { if (d_b[d]) (void)hipFree(d_b[d]); if (d_bhat[d]) (void)hipFree(d_bhat[d]); if (d_bout[d]) (void)hipFree(d_bout[d]);
                                      if (d_hat_out[d]) (void)hipFree(d_hat_out[d]);
                                      if (d_in_s[d]) (void)hipFree(d_in_s[d]); if (d_hat_out_s[d]) (void)hipFree(d_hat_out_s[d]); }
        if (sub.d_tw) (void)hipFree(sub.d_tw);
    }
};

struct ig_fft {
    ig_ctx* ctx = nullptr;
    bool is_chirp_sub = false;       // a throw-away plan made to plan the length-m axis of a chirp-z axis (no nesting)
    int rank = 0;
    int64_t dims[3] = {1, 1, 1};
    int64_t batch = 1;
    int64_t total = 0;               // elements in all volumes
    AxisPlan axis[3];
    size_t workspace_bytes = 0;
    std::string desc;
    // zero-padded / cropped plans (ig_fft_plan_padded): the image occupies box_lo .. box_lo+box_dims of the grid
    bool two_launch = false;         // 256^3 volumes: k_fft3d_a + k_fft3d_b instead of three axis passes
    size_t inplace_workspace_bytes = 0;   // two-launch transform called in place: staging volumes in the CALLER's workspace (ig_fft_inplace_workspace)
    bool padded = false;
    bool has_ab_axis = false;        // a zero-padded plan with an A x B axis (160 ... 640)
    bool has_chirp_axis = false;     // ... with a chirp-z axis (y or z): no k-space support table
    int zw_in = 16, zw_out = 16;     // words per entry of the k-space support table's bitmaps on the z axis (ig_fft_support_words)
    int layout = 0;                  // memory order of the grid: 0 = (x, y, z), 1 = (x, z, y)
    int support_tile = 16;           // kx points per entry of the k-space support table (layout 2: ig_fft_set_support_tile)
    int64_t box_lo[3] = {0, 0, 0}, box_dims[3] = {1, 1, 1};
};

// ---- ig_fft.hip: one two-stage axis pass (n in {256, 512}); axis0 selects the lane mapping for contiguous columns; stream: the
// stream of the launch where it is not the context's, keep_out: stores of the default cache policy instead of streaming ones (the
// chunked x / y pair, ig_fft_xy.h)
int ig_launch_2stage(ig_ctx* ctx, const AxisPlan& ax, const PassDesc& d, bool axis0, int wmode, hipStream_t stream = nullptr, bool keep_out = false);
// which instantiation such a pass takes: whether it is boxed, its compile-time half box; returns whether it runs on 32-column tiles
bool ig_two_stage_variant(const AxisPlan& ax, const PassDesc& d, bool axis0, int wmode, bool& boxed, int& half);
// the launch grid of a pass kernel at cpt columns per tile, after the checks of the tile count and the 2 GB descriptor window
int ig_pass_tiles(ig_ctx* ctx, PassDesc& d, int64_t cpt, int64_t reach, bool weights, const char* kernel, dim3& grid);

// ---- ig_fft_plain.hip: one launch per kernel (each applies its kernel's dynamic-LDS opt-in where it needs one); blocks: the grid
// of the grid-stride kernels
int ig_launch_fft3d_a(ig_ctx* ctx, const float2* in, float2* out, const float2* tw, int64_t batch, int inverse);
int ig_launch_fft3d_b(ig_ctx* ctx, const float2* in, float2* out, const float2* tw, int64_t batch, int inverse);
int ig_launch_fft_lds(ig_ctx* ctx, const AxisPlan& ax, const float2* in, float2* out, int inverse);
int ig_launch_fft_generic_stage(ig_ctx* ctx, unsigned blocks, const float2* in, float2* out, const float2* tw, int64_t n, int64_t inner,
                                int64_t total, int R, int64_t Ns, int inverse);
int ig_launch_chirp_pre(ig_ctx* ctx, unsigned blocks, const float2* x, float2* W, const float2* b, int64_t n, int64_t m, int64_t inner, int64_t total_m);
int ig_launch_chirp_mul(ig_ctx* ctx, unsigned blocks, float2* W, const float2* bhat, int64_t m, int64_t inner, int64_t total_m);
int ig_launch_chirp_post(ig_ctx* ctx, unsigned blocks, const float2* W, float2* y, const float2* bout, int64_t n, int64_t m, int64_t inner, int64_t total_n);
