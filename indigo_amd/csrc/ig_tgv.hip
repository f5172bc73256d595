// Second-order total generalized variation of complex64 volumes: the symmetrised backward difference E of a 3-component field, its
// adjoint, and the two fused passes of the primal-dual iteration on (x; v) (operators.SymGradient, Backend.symgrad3 / tgv_adjoint /
// tgv_dual_step, pics --tgv).
//
// A column of x is an F-ordered n0 x n1 x n2 volume with N voxels (axis 0 fastest), a column of v or p three of them, component a
// in rows [aN, (a+1)N), a column of q six: xx, yy, zz, xy, xz, yz, component c in rows [cN, (c+1)N).  With e_a the step along axis
// a, D_a the forward difference of ig_tv.hip (zero on the far face) and B_a = -D_a^H the matching backward difference:
//   (B_a w)[i] = (i_a < n_a - 1 ? w[i] : 0) - (i_a > 0 ? w[i - e_a] : 0)
//   (E v)_aa = B_a v_a                                   (E v)_ab = (B_b v_a + B_a v_b) / sqrt(2),  a < b, stored once
//   (E^H q)_a = -D_a q_aa - sum_{b != a} D_b q_ab / sqrt(2)
// so that the 2-norm of the six components is the Frobenius norm of the symmetric 3 x 3 tensor.  D_b never reads past the far face
// and B_a never before the near one; E^H is the exact adjoint.  K (x; v) = (D x - v; E v), K^H (p; q) = (D^H p; E^H q - p).
//
// The four kernels are the streaming stencils of ig_tv.hip (ig_stencil.h: 256 / LX x-contiguous rows per workgroup, LX = 8 .. 64):
// the neighbours along x are in the same lines, those along y and z are rows that this or a nearby workgroup streams anyway, the
// caches serve them and nothing is staged in LDS.  Outputs must not overlap inputs.  Bytes per voxel and column:
//   k_symgrad   v 24 read, y 48 written                        =  72   (+ 48 when beta != 0)
//   k_symgradh  q 48 read, y 24 written                        =  72   (+ 24 when beta != 0)
//   k_tgv_kh    p 24, q 48 read, gx 8 + 8, gv 24 written       = 112
//   k_tgv_dual  xn, xo 16, vn, vo 48 read, p 24 + 24, q 48 + 48 = 208
#include "ig_stencil.h"

namespace {

constexpr float RSQRT2 = 0.70710678118654752440f;

// which neighbours the voxel has, and the strides to them
struct tgv_nb {
    bool fwd[3], bwd[3];
    int64_t s[3];
    __device__ __forceinline__ tgv_nb(const tv_dims& d, int64_t i0, int64_t i1, int64_t i2)
        : fwd{i0 < d.n0 - 1, i1 < d.n1 - 1, i2 < d.n2 - 1}, bwd{i0 > 0, i1 > 0, i2 > 0}, s{1, d.n0, d.n0 * d.n1} {}
};

// e = (E w)[i] and c_a = w_a[i], with w_a at offset `off` from the voxel given by val(a, off): 3 values and 9 backward neighbours
template <class V>
__device__ __forceinline__ void symgrad_at(const tgv_nb& nb, V val, float2 (&c)[3], float2 (&e)[6]) {
    const float2 zero = make_float2(0.f, 0.f);
    float2 b[3][3];                                        // b[a][k] = (B_k w_a)[i]
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        c[a] = val(a, 0);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float2 back = nb.bwd[k] ? val(a, -nb.s[k]) : zero;
            b[a][k] = csub(nb.fwd[k] ? c[a] : zero, back);
        }
    }
    e[0] = b[0][0]; e[1] = b[1][1]; e[2] = b[2][2];
    e[3] = make_float2((b[0][1].x + b[1][0].x) * RSQRT2, (b[0][1].y + b[1][0].y) * RSQRT2);
    e[4] = make_float2((b[0][2].x + b[2][0].x) * RSQRT2, (b[0][2].y + b[2][0].y) * RSQRT2);
    e[5] = make_float2((b[1][2].x + b[2][1].x) * RSQRT2, (b[1][2].y + b[2][1].y) * RSQRT2);
}

// g = (E^H q)[i], with q_c at offset `off` from the voxel given by val(c, off): 6 values and 9 forward neighbours
template <class V>
__device__ __forceinline__ void symgradh_at(const tgv_nb& nb, V val, float2 (&g)[3]) {
    const float2 zero = make_float2(0.f, 0.f);
    float2 c[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) c[k] = val(k, 0);
    auto D = [&](int k, int comp) { return nb.fwd[k] ? csub(val(comp, nb.s[k]), c[comp]) : zero; };   // (D_k q_comp)[i]
    const float2 d0 = D(0, 0), d1 = D(1, 1), d2 = D(2, 2);
    const float2 xy1 = D(1, 3), xy0 = D(0, 3), xz2 = D(2, 4), xz0 = D(0, 4), yz2 = D(2, 5), yz1 = D(1, 5);
    g[0] = make_float2(fmaf(-RSQRT2, xy1.x + xz2.x, -d0.x), fmaf(-RSQRT2, xy1.y + xz2.y, -d0.y));
    g[1] = make_float2(fmaf(-RSQRT2, xy0.x + yz2.x, -d1.x), fmaf(-RSQRT2, xy0.y + yz2.y, -d1.y));
    g[2] = make_float2(fmaf(-RSQRT2, xz0.x + yz1.x, -d2.x), fmaf(-RSQRT2, xz0.y + yz1.y, -d2.y));
}

// y[cN + i, j] = beta * y[cN + i, j] + alpha * (E v[:, j])_c[i], c < 6;  READ_Y false: y is not read
template <bool READ_Y>
__global__ void __launch_bounds__(TV_BLK)
k_symgrad(tv_dims d, int64_t ncols, const float2* __restrict__ v, int64_t ldv, float2 a, float2 b,
          float2* __restrict__ y, int64_t ldy) {
    for_each_voxel(d, ncols, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        const float2* vc = v + j * ldv + i;
        float2* yc = y + j * ldy + i;
        const tgv_nb nb(d, i0, i1, i2);
        float2 c[3], e[6];
        symgrad_at(nb, [&](int comp, int64_t off) { return vc[comp * d.vol + off]; }, c, e);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            float2 r = cmul(a, e[k]);
            if (READ_Y) cfma(r, b, yc[k * d.vol]);
            yc[k * d.vol] = r;
        }
    });
}

// y[aN + i, j] = beta * y[aN + i, j] + alpha * (E^H q[:, j])_a[i], a < 3
template <bool READ_Y>
__global__ void __launch_bounds__(TV_BLK)
k_symgradh(tv_dims d, int64_t ncols, const float2* __restrict__ q, int64_t ldq, float2 a, float2 b,
           float2* __restrict__ y, int64_t ldy) {
    for_each_voxel(d, ncols, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        const float2* qc = q + j * ldq + i;
        float2* yc = y + j * ldy + i;
        const tgv_nb nb(d, i0, i1, i2);
        float2 g[3];
        symgradh_at(nb, [&](int comp, int64_t off) { return qc[comp * d.vol + off]; }, g);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float2 r = cmul(a, g[k]);
            if (READ_Y) cfma(r, b, yc[k * d.vol]);
            yc[k * d.vol] = r;
        }
    });
}

// K^H in one pass: gx[i, j] += (D^H p[:, j])[i];  gv[aN + i, j] = (E^H q[:, j])_a[i] - p[aN + i, j]  (gv is not read)
__global__ void __launch_bounds__(TV_BLK)
k_tgv_kh(tv_dims d, int64_t ncols, const float2* __restrict__ p, int64_t ldp, const float2* __restrict__ q, int64_t ldq,
         float2* __restrict__ gx, int64_t ldgx, float2* __restrict__ gv, int64_t ldgv) {
    for_each_voxel(d, ncols, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        const float2* pc = p + j * ldp + i;
        const float2* qc = q + j * ldq + i;
        float2* gxp = gx + j * ldgx + i;
        float2* gvc = gv + j * ldgv + i;
        const tgv_nb nb(d, i0, i1, i2);
        float2 g[3];
        symgradh_at(nb, [&](int comp, int64_t off) { return qc[comp * d.vol + off]; }, g);
        *gxp = cadd(*gxp, grad_adjoint_at(d, pc, i0, i1, i2));
#pragma unroll
        for (int k = 0; k < 3; ++k) gvc[k * d.vol] = csub(g[k], pc[k * d.vol]);
    });
}

// The dual step in one pass, w = 2 (xn; vn) - (xo; vo):
//   p <- proj_{a1}(p + sigma (D w_x - w_v))  (3 components, the ball r^2 <= a1^2)
//   q <- proj_{a0}(q + sigma E w_v)          (6 components, the ball r^2 <= a0^2)
// both compared squared, as k_dual of ig_tv.hip compares.  w_x at the voxel and its three forward neighbours, w_v at the voxel and
// its nine backward neighbours: 8 + 24 loads, p and q read and written once.
__global__ void __launch_bounds__(TV_BLK)
k_tgv_dual(tv_dims d, int64_t ncols, const float2* __restrict__ xn, int64_t ldxn, const float2* __restrict__ xo, int64_t ldxo,
           const float2* __restrict__ vn, int64_t ldvn, const float2* __restrict__ vo, int64_t ldvo, float sigma, float a1, float a0,
           float2* __restrict__ p, int64_t ldp, float2* __restrict__ q, int64_t ldq) {
    const float a1sq = a1 * a1, a0sq = a0 * a0;
    for_each_voxel(d, ncols, [&](int64_t j, int64_t i0, int64_t i1, int64_t i2, int64_t i) {
        const float2* xnc = xn + j * ldxn + i;
        const float2* xoc = xo + j * ldxo + i;
        const float2* vnc = vn + j * ldvn + i;
        const float2* voc = vo + j * ldvo + i;
        float2* pc = p + j * ldp + i;
        float2* qc = q + j * ldq + i;
        const tgv_nb nb(d, i0, i1, i2);
        auto two_minus = [](float2 n, float2 o) { return make_float2(fmaf(2.f, n.x, -o.x), fmaf(2.f, n.y, -o.y)); };
        auto wx = [&](int64_t off) { return two_minus(xnc[off], xoc[off]); };
        const float2 zero = make_float2(0.f, 0.f);
        float2 c[3], e[6];
        symgrad_at(nb, [&](int comp, int64_t off) { return two_minus(vnc[comp * d.vol + off], voc[comp * d.vol + off]); }, c, e);
        const float2 w0 = wx(0);
        float2 t[3];
        float r2 = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float2 g = csub(nb.fwd[k] ? csub(wx(nb.s[k]), w0) : zero, c[k]);
            const float2 u = pc[k * d.vol];
            t[k] = make_float2(fmaf(sigma, g.x, u.x), fmaf(sigma, g.y, u.y));
            r2 = fmaf(t[k].x, t[k].x, r2);
            r2 = fmaf(t[k].y, t[k].y, r2);
        }
        const float f1 = r2 <= a1sq ? 1.f : a1 / sqrtf(r2);
#pragma unroll
        for (int k = 0; k < 3; ++k) pc[k * d.vol] = make_float2(t[k].x * f1, t[k].y * f1);
        float2 s[6];
        float rq2 = 0.f;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const float2 u = qc[k * d.vol];
            s[k] = make_float2(fmaf(sigma, e[k].x, u.x), fmaf(sigma, e[k].y, u.y));
            rq2 = fmaf(s[k].x, s[k].x, rq2);
            rq2 = fmaf(s[k].y, s[k].y, rq2);
        }
        const float f0 = rq2 <= a0sq ? 1.f : a0 / sqrtf(rq2);
#pragma unroll
        for (int k = 0; k < 6; ++k) qc[k * d.vol] = make_float2(s[k].x * f0, s[k].y * f0);
    });
}

// The body of ig_symgrad3_c64 (ADJ false: in = v with 3N rows per column, y with 6N) and of ig_symgrad3h_c64 (ADJ true: in = q with
// 6N rows, y with 3N).  72 bytes per voxel and column either way, and y once more where it is read.
template <bool ADJ>
int symgrad_launch(ig_ctx* ctx, const char* fn, const char* kname, int64_t n0, int64_t n1, int64_t n2, int64_t ncols,
                   const void* in, int64_t ldin, float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    IG_REQUIRE(ctx, ctx != nullptr, "%s: ctx is NULL", fn);
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && ncols >= 0, "%s: negative dimension", fn);
    const tv_dims d = make_dims(n0, n1, n2);
    const int64_t rows_in = (ADJ ? 6 : 3) * d.vol, rows_y = (ADJ ? 3 : 6) * d.vol;
    IG_REQUIRE(ctx, ldin >= rows_in && ldy >= rows_y, "%s: leading dimension (%lld, %lld) below (%s, %s) for N = %lld", fn,
               (long long)ldin, (long long)ldy, ADJ ? "6N" : "3N", ADJ ? "3N" : "6N", (long long)d.vol);
    if (d.vol == 0 || ncols == 0) return IG_OK;
    IG_REQUIRE(ctx, in && y, "%s: NULL pointer", fn);
    IG_REQUIRE(ctx, !ig_panels_overlap(in, ldin, rows_in, ncols, y, ldy, rows_y, ncols), "%s: y overlaps %s", fn, ADJ ? "q" : "v");
    if (int rc = ig_set_device(ctx)) return rc;
    const bool b0 = (br == 0.f && bi == 0.f);
    const float2 a = make_float2(ar, ai), b = make_float2(br, bi);
    const dim3 g = make_grid(d, ncols);
    ig_prof_scope prof(ctx, kname + 2, (double)d.vol * ncols * (72.0 + (b0 ? 0.0 : ADJ ? 24.0 : 48.0)));
#define IG_TGV_GO(KERNEL, READ_Y) hipLaunchKernelGGL((KERNEL<READ_Y>), g, dim3(TV_BLK), 0, ctx->stream, d, ncols, (const float2*)in, ldin, a, b, (float2*)y, ldy)
    if (ADJ) { if (b0) IG_TGV_GO(k_symgradh, false); else IG_TGV_GO(k_symgradh, true); }
    else     { if (b0) IG_TGV_GO(k_symgrad, false);  else IG_TGV_GO(k_symgrad, true); }
#undef IG_TGV_GO
    IG_LAUNCH_CHECK(ctx, kname);
    return IG_OK;
}

// whether the rows x ncols panel `out` shares a byte with any of the `count` input panels
struct tgv_panel { const void* p; int64_t ld, rows; };
bool overlaps_any(const tgv_panel& out, const tgv_panel* in, int count, int64_t ncols) {
    for (int k = 0; k < count; ++k)
        if (ig_panels_overlap(out.p, out.ld, out.rows, ncols, in[k].p, in[k].ld, in[k].rows, ncols)) return true;
    return false;
}

}  // namespace

int ig_symgrad3_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, const void* v, int64_t ldv,
                    float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    return symgrad_launch<false>(ctx, "ig_symgrad3_c64", "k_symgrad3", n0, n1, n2, ncols, v, ldv, ar, ai, br, bi, y, ldy);
}

int ig_symgrad3h_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, const void* q, int64_t ldq,
                     float ar, float ai, float br, float bi, void* y, int64_t ldy) {
    return symgrad_launch<true>(ctx, "ig_symgrad3h_c64", "k_symgrad3h", n0, n1, n2, ncols, q, ldq, ar, ai, br, bi, y, ldy);
}

int ig_tgv_kh_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, const void* p, int64_t ldp,
                  const void* q, int64_t ldq, void* gx, int64_t ldgx, void* gv, int64_t ldgv) {
    const char* fn = "ig_tgv_kh_c64";
    IG_REQUIRE(ctx, ctx != nullptr, "%s: ctx is NULL", fn);
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && ncols >= 0, "%s: negative dimension", fn);
    const tv_dims d = make_dims(n0, n1, n2);
    IG_REQUIRE(ctx, ldp >= 3 * d.vol && ldq >= 6 * d.vol && ldgx >= d.vol && ldgv >= 3 * d.vol,
               "%s: leading dimension (%lld, %lld, %lld, %lld) below (3N, 6N, N, 3N) for N = %lld", fn, (long long)ldp, (long long)ldq,
               (long long)ldgx, (long long)ldgv, (long long)d.vol);
    if (d.vol == 0 || ncols == 0) return IG_OK;
    IG_REQUIRE(ctx, p && q && gx && gv, "%s: NULL pointer", fn);
    const tgv_panel in[] = {{p, ldp, 3 * d.vol}, {q, ldq, 6 * d.vol}, {gv, ldgv, 3 * d.vol}};
    IG_REQUIRE(ctx, !overlaps_any({gx, ldgx, d.vol}, in, 3, ncols) && !overlaps_any({gv, ldgv, 3 * d.vol}, in, 2, ncols),
               "%s: gx or gv overlaps p, q or the other", fn);
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, "tgv_kh", (double)d.vol * ncols * 112.0);
    hipLaunchKernelGGL(k_tgv_kh, make_grid(d, ncols), dim3(TV_BLK), 0, ctx->stream, d, ncols, (const float2*)p, ldp,
                       (const float2*)q, ldq, (float2*)gx, ldgx, (float2*)gv, ldgv);
    IG_LAUNCH_CHECK(ctx, "k_tgv_kh");
    return IG_OK;
}

int ig_tgv_dual_c64(ig_ctx* ctx, int64_t n0, int64_t n1, int64_t n2, int64_t ncols, const void* xn, int64_t ldxn,
                    const void* xo, int64_t ldxo, const void* vn, int64_t ldvn, const void* vo, int64_t ldvo,
                    float sigma, float a1, float a0, void* p, int64_t ldp, void* q, int64_t ldq) {
    const char* fn = "ig_tgv_dual_c64";
    IG_REQUIRE(ctx, ctx != nullptr, "%s: ctx is NULL", fn);
    IG_REQUIRE(ctx, n0 >= 0 && n1 >= 0 && n2 >= 0 && ncols >= 0, "%s: negative dimension", fn);
    IG_REQUIRE(ctx, a1 >= 0.f && a0 >= 0.f, "%s: negative radius (%g, %g)", fn, (double)a1, (double)a0);
    const tv_dims d = make_dims(n0, n1, n2);
    IG_REQUIRE(ctx, ldxn >= d.vol && ldxo >= d.vol && ldvn >= 3 * d.vol && ldvo >= 3 * d.vol && ldp >= 3 * d.vol && ldq >= 6 * d.vol,
               "%s: leading dimension (%lld, %lld, %lld, %lld, %lld, %lld) below (N, N, 3N, 3N, 3N, 6N) for N = %lld", fn, (long long)ldxn,
               (long long)ldxo, (long long)ldvn, (long long)ldvo, (long long)ldp, (long long)ldq, (long long)d.vol);
    if (d.vol == 0 || ncols == 0) return IG_OK;
    IG_REQUIRE(ctx, xn && xo && vn && vo && p && q, "%s: NULL pointer", fn);
    const tgv_panel in[] = {{xn, ldxn, d.vol}, {xo, ldxo, d.vol}, {vn, ldvn, 3 * d.vol}, {vo, ldvo, 3 * d.vol}, {q, ldq, 6 * d.vol}};
    IG_REQUIRE(ctx, !overlaps_any({p, ldp, 3 * d.vol}, in, 5, ncols) && !overlaps_any({q, ldq, 6 * d.vol}, in, 4, ncols),
               "%s: p or q overlaps xn, xo, vn, vo or the other", fn);
    if (int rc = ig_set_device(ctx)) return rc;
    ig_prof_scope prof(ctx, "tgv_dual", (double)d.vol * ncols * 208.0);
    hipLaunchKernelGGL(k_tgv_dual, make_grid(d, ncols), dim3(TV_BLK), 0, ctx->stream, d, ncols, (const float2*)xn, ldxn,
                       (const float2*)xo, ldxo, (const float2*)vn, ldvn, (const float2*)vo, ldvo, sigma, a1, a0, (float2*)p, ldp,
                       (float2*)q, ldq);
    IG_LAUNCH_CHECK(ctx, "k_tgv_dual");
    return IG_OK;
}
