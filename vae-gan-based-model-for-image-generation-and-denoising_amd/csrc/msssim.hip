// Multi-scale SSIM reconstruction loss (Wang, Simoncelli & Bovik 2003), forward and backward: the contract of
// include/vaegan_hip.h (vg_msssim_loss_forward_backward).  a (reconstruction), b (target): NCHW f32 in [-1, 1]; level j + 1 of
// the pyramid is the 2 x 2 mean (stride 2, floor sizes, f32) of level j; at every level the maps of ssimloss.hip on
// u = (a_j + 1) / 2, v = (b_j + 1) / 2 over the interior [5, H_j - 5) x [5, W_j - 5):  cs = A2 / B2 for j < M - 1, S = (A1 / B1)
// (A2 / B2) at the last level; m_{b,j} their mean per IMAGE (channels and pixels), n_j = C (H_j - 10)(W_j - 10);
//   P_b = prod_j m_{b,j}^{w_j} if every m_{b,j} > 0 else 0,   loss[0] (+)= 1 - (1 / B) sum_b P_b
//   k_{b,j} = w_j P_b / (m_{b,j} B n_j) (0 on the clamp),     g_j = -k_{b,j} d(sum_p map_j(p)) / d a_j
//   d[q] += gscale sum_j 4^-j g_j[q >> j]                      over the levels whose plane contains q >> j
//
// The coefficient of every pixel's gradient hangs on P_b, a reduction over the whole image at every level, so forward and
// backward cannot share a launch.  The launches (their number does not grow with M):
//   1. pyramid   (M > 1)  a workgroup owns a 32 x 32 base block of a plane and writes its 16 x 16 ... 2 x 2 descendants of a and b
//   2. forward            one workgroup per 32 x 32 tile of every level (the level is found from the block index in a table
//                         that travels by value); an f32 partial of the tile's interior cs / S sum, summed in f64; only the
//                         row- and column-pass items that feed the tile's own pixels are computed
//   3. finalize           one workgroup: m (one thread per (image, level), its partials in index order), P, k in f64, the loss,
//                         per_scale, and the f32 coefficient -gscale k / 2 of every (image, level)
//   4. backward  (d)      the same tiles: the maps again, the three derivative maps, their transposed correlation with the
//                         window; g_j times the coefficient, WRITTEN into a gradient pyramid.  A workgroup of an image on
//                         the clamp (coefficient 0) writes zeros and computes nothing
//   5. collapse  (d)      one thread per element of d: the sum over the levels and the one read-modify-write (skipped
//                         where the sum is zero: d of a clamped image comes back bit for bit)
// Every element has one owner in every launch: no atomics, the same bits run to run and eager vs. replayed.  The tile pass --
// staging with the per-tile shift, the four separable passes, the pointwise step without fma contraction in its S and cs
// forms, the window -- is csrc/ssim_tile.hpp, shared with ssimloss.hip; the reasoning about cancellation and contraction
// (why identical images give cs = S = 1 exactly at every level) is there.  What is here: the level lookup, the clamp
// early-out, the forward launch's skip of the items outside the tile, the stores, and launches 1, 3 and 5.
// No host synchronisation.
#include "common.hpp"

#include <climits>
#include <cmath>

namespace {

#include "ssim_tile.hpp"                // NT, TS (also the pyramid's base block), KW, HW5, Gauss11 and the tile pass

constexpr int MAXM = 5;
constexpr int TIMING_FAMILY = 5;

struct Level {
    int H, W, tiles_x, tiles_per_plane;
    int tile_start;                     // first workgroup of this level in the forward / backward launches
    int is_cs;                          // 1: the contrast-structure map (every level but the last)
    int64_t in_off;                     // floats from the start of the a (or b) pyramid to this level (levels >= 1)
    int64_t g_off;                      // floats from the start of the gradient pyramid to this level (levels >= 0)
};

// Everything the launches need to know, by value.  Offsets are in floats from the workspace's start.
struct Plan {
    int M, B, C, tiles_total;
    Level l[MAXM];
    double w[MAXM];
    int64_t o_coef, o_partial, o_apyr, o_bpyr, o_gpyr;       // (f64 [B][1 + M] sits at the very start: P_b and the m_{b,j})
    int64_t total_floats;
};

inline int64_t round4(int64_t v) { return (v + 3) & ~(int64_t)3; }

// The geometry of (B, C, H, W, M); false for sizes outside the contract.
bool make_plan(int B, int C, int H, int W, int M, Plan& p) {
    if (B <= 0 || C <= 0 || M < 1 || M > MAXM || H < KW || W < KW) return false;
    if ((H >> (M - 1)) < KW || (W >> (M - 1)) < KW) return false;
    p.M = M, p.B = B, p.C = C;
    const int64_t planes = (int64_t)B * C;
    int64_t tiles = 0, n_in = 0, n_g = 0;
    for (int j = 0; j < M; ++j) {
        Level& l = p.l[j];
        l.H = H >> j, l.W = W >> j;
        l.tiles_x = (l.W + TS - 1) / TS;
        l.tiles_per_plane = l.tiles_x * ((l.H + TS - 1) / TS);
        if (tiles > INT_MAX) return false;
        l.tile_start = (int)tiles;
        l.is_cs = j < M - 1;
        tiles += planes * l.tiles_per_plane;
        const int64_t px = planes * l.H * l.W;
        if (px > ((int64_t)1 << 38)) return false;      // (the collapse launch: one thread per element, 2^30 workgroups)
        l.in_off = j ? n_in : 0;
        l.g_off = n_g;
        if (j) n_in += round4(px);
        n_g += round4(px);
    }
    for (int j = M; j < MAXM; ++j) p.l[j] = Level{0, 0, 0, 0, INT_MAX, 0, 0, 0};
    if (tiles > INT_MAX) return false;
    p.tiles_total = (int)tiles;
    int64_t o = round4(2 * (int64_t)B * (M + 1));
    p.o_coef = o, o += round4((int64_t)B * M);
    p.o_partial = o, o += round4(tiles);
    p.o_apyr = o, o += n_in;
    p.o_bpyr = o, o += n_in;
    p.o_gpyr = o, o += n_g;
    p.total_floats = o;
    return true;
}

// ---- 1. the pyramid: a 32 x 32 base block and all its descendants, a and b ------------------------------------------------
__global__ __launch_bounds__(NT) void msssim_pyramid_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            float* __restrict__ ws, Plan pl) {
    __shared__ float lv[2][TS * TS + 256 + 64 + 16 + 4];
    const int tid = threadIdx.x;
    const Level l0 = pl.l[0];
    const int tile = blockIdx.x % l0.tiles_per_plane;
    const int64_t plane = blockIdx.x / l0.tiles_per_plane;
    const int ty0 = (tile / l0.tiles_x) * TS, tx0 = (tile % l0.tiles_x) * TS;
    const float* src[2] = {a + plane * l0.H * l0.W, b + plane * l0.H * l0.W};
    for (int e = tid; e < 2 * TS * TS; e += NT) {
        const int which = e / (TS * TS), r = e % (TS * TS);
        const int y = ty0 + r / TS, x = tx0 + r % TS;
        lv[which][r] = (y < l0.H && x < l0.W) ? src[which][(int64_t)y * l0.W + x] : 0.f;
    }
    __syncthreads();
    int from = 0, to = TS * TS;
    for (int j = 1; j < pl.M; ++j) {
        const int s = TS >> j;
        const Level l = pl.l[j];
        const int by = ty0 >> j, bx = tx0 >> j;
        for (int e = tid; e < 2 * s * s; e += NT) {
            const int which = e / (s * s), r = e % (s * s);
            const int ly = r / s, lx = r % s;
            const float* p = &lv[which][from + (2 * ly) * (2 * s) + 2 * lx];
            float v;
            {
#pragma clang fp contract(off)
                v = ((p[0] + p[1]) + (p[2 * s] + p[2 * s + 1])) * 0.25f;
            }
            lv[which][to + r] = v;
            const int y = by + ly, x = bx + lx;
            if (y < l.H && x < l.W)         // then its four sources are pixels of level j - 1 (2 y + 1 < 2 H_j <= H_{j-1})
                ws[(which ? pl.o_bpyr : pl.o_apyr) + l.in_off + plane * l.H * l.W + (int64_t)y * l.W + x] = v;
        }
        __syncthreads();
        from = to;
        to += s * s;
    }
}

// ---- 2 and 4. the tile pass over every level ---------------------------------------------------------------------------------
template <bool BWD>
__global__ __launch_bounds__(NT) void msssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         float* __restrict__ ws, Plan pl, Gauss11 gw) {
    __shared__ float sin_[SSIM_LDS_IN];
    __shared__ float tmp[SSIM_LDS_TMP];
    __shared__ float redf[4][2];
    __shared__ double redd[4];
    float* su = sin_;
    float* sv = sin_ + RI * RIP;
    float* sD = sin_;                                   // the derivative maps take the staged inputs' place
    const int tid = threadIdx.x;
    int lev = 0;
    for (int j = 1; j < pl.M; ++j)
        if ((int)blockIdx.x >= pl.l[j].tile_start) lev = j;
    const Level l = pl.l[lev];
    const int H = l.H, W = l.W;
    const int local = (int)blockIdx.x - l.tile_start;
    const int tile = local % l.tiles_per_plane;
    const int64_t plane = local / l.tiles_per_plane;
    const int ty0 = (tile / l.tiles_x) * TS, tx0 = (tile % l.tiles_x) * TS;
    const float* pa = (lev ? ws + pl.o_apyr + l.in_off : a) + plane * H * W;
    const float* pb = (lev ? ws + pl.o_bpyr + l.in_off : b) + plane * H * W;
    const bool cs_only = l.is_cs != 0;

    float coef = 0.f;
    if (BWD) {
        coef = ws[pl.o_coef + (plane / pl.C) * pl.M + lev];
        if (coef == 0.f) {                      // an image on the clamp: gradient exactly 0 (uniform over the workgroup)
            float* pg = ws + pl.o_gpyr + l.g_off + plane * H * W;
            for (int e = tid; e < TS * TS; e += NT) {
                const int y = ty0 + e / TS, x = tx0 + e % TS;
                if (y < H && x < W) pg[(int64_t)y * W + x] = 0.f;
            }
            return;
        }
    }

    const SsimShift sh = ssim_stage_shift(pa, pb, H, W, ty0, tx0, su, sv, redf);
    const int qc = tid % TS, qr0 = (tid / TS) * 4;      // the thread's own four pixels of the level's gradient plane
    float uq[4], vq[4];
    if (BWD) ssim_own_pixels(su, sv, qc, qr0, uq, vq);
    // the forward launch sums the tile's own pixels only: it skips the row- and column-pass items that feed no such pixel
    // and never writes the derivative maps
    ssim_fwd_rows(su, sv, tmp, gw, !BWD);
    __syncthreads();                                    // su, sv are dead from here on
    const double acc = ssim_fwd_cols(tmp, sD, gw, H, W, ty0, tx0, sh, cs_only, BWD, !BWD);
    if (!BWD) {
        const float sum = ssim_tile_sum(acc, redd);
        if (tid == 0) ws[pl.o_partial + blockIdx.x] = sum;
        return;
    }
    __syncthreads();

    ssim_bwd_rows(sD, tmp, gw);
    __syncthreads();
    float wsum[3][4];
    ssim_bwd_cols(tmp, gw, qc, qr0, wsum);
    float* pg = ws + pl.o_gpyr + l.g_off + plane * H * W;
    const int x = tx0 + qc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = ty0 + qr0 + j;
        if (y < H && x < W) pg[(int64_t)y * W + x] = ssim_grad_pixel(coef, wsum, uq, vq, j);      // WRITTEN, not added
    }
}

// ---- 3. m, P, k, the loss ---------------------------------------------------------------------------------------------------
// One workgroup, three phases.  A: one THREAD per (image, level) sums that pair's tile partials in f64, in index order (its
// loads are independent, so they overlap; a wave per pair would pay one memory round trip per pair, in sequence).  B: one
// thread per image forms P_b and the coefficients.  C: one wave sums the P_b.  All in a fixed order.
__global__ __launch_bounds__(NT) void msssim_final_kernel(float* __restrict__ ws, Plan pl, float gscale,
                                                          float* __restrict__ loss, int accumulate,
                                                          float* __restrict__ per_scale) {
    double* dbl = reinterpret_cast<double*>(ws);            // [B][1 + M]: P_b, m_{b,0} .. m_{b,M-1}
    const float* partial = ws + pl.o_partial;
    const int M = pl.M, stride = pl.M + 1;
    for (int pair = threadIdx.x; pair < pl.B * M; pair += NT) {
        const int img = pair / M, j = pair % M;
        const Level l = pl.l[j];
        const int cnt = pl.C * l.tiles_per_plane;
        const float* p = partial + l.tile_start + (int64_t)img * cnt;
        double s = 0.0;
        for (int i = 0; i < cnt; ++i) s += (double)p[i];
        dbl[(int64_t)img * stride + 1 + j] = s / ((double)pl.C * (l.H - 2 * HW5) * (double)(l.W - 2 * HW5));
    }
    __syncthreads();
    for (int img = threadIdx.x; img < pl.B; img += NT) {
        double* row = dbl + (int64_t)img * stride;
        bool ok = true;
        for (int j = 0; j < M; ++j) ok = ok && row[1 + j] > 0.0;
        double prod = 0.0;
        if (ok) {
            prod = 1.0;
            for (int j = 0; j < M; ++j) prod *= pow(row[1 + j], pl.w[j]);
        }
        row[0] = prod;
        for (int j = 0; j < M; ++j) {
            const Level l = pl.l[j];
            const double n = (double)pl.C * (l.H - 2 * HW5) * (double)(l.W - 2 * HW5);
            const double k = ok ? pl.w[j] * prod / (row[1 + j] * (double)pl.B * n) : 0.0;
            ws[pl.o_coef + (int64_t)img * M + j] = (float)(-0.5 * (double)gscale * k);
            if (per_scale) per_scale[(int64_t)img * M + j] = (float)row[1 + j];
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        double s = 0.0;
        for (int i = threadIdx.x; i < pl.B; i += 64) s += dbl[(int64_t)i * stride];
        s = wave_sum_d(s);
        if (threadIdx.x == 0) {
            const float v = (float)(1.0 - s / (double)pl.B);
            loss[0] = accumulate ? loss[0] + v : v;
        }
    }
}

// ---- 5. the adjoint of the pooling chain and the one read-modify-write of d ----------------------------------------------------
__global__ __launch_bounds__(NT) void msssim_collapse_kernel(float* __restrict__ d, const float* __restrict__ ws, Plan pl,
                                                             int64_t total) {
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const int H = pl.l[0].H, W = pl.l[0].W;
    const int64_t plane = e / ((int64_t)H * W);
    const int r = (int)(e % ((int64_t)H * W));
    const int y = r / W, x = r % W;
    const float* g = ws + pl.o_gpyr;
    float s = g[e];                                      // level 0 sits at the pyramid's start in d's own layout
    float scale = 1.f;
    for (int j = 1; j < pl.M; ++j) {
        const Level l = pl.l[j];
        scale *= 0.25f;
        const int yj = y >> j, xj = x >> j;
        if (yj < l.H && xj < l.W) s += scale * g[l.g_off + plane * l.H * l.W + (int64_t)yj * l.W + xj];
    }
    if (s != 0.f) d[e] += s;                             // a clamped image: every level wrote 0 and d keeps its bits
}

}  // namespace

extern "C" int64_t vg_msssim_ws_bytes(int B, int C, int H, int W, int M) {
    Plan p;
    VG_CHECK_ARG(make_plan(B, C, H, W, M, p), VG_EINVAL);
    return p.total_floats * 4;
}

extern "C" int vg_msssim_loss_forward_backward(const float* a, const float* b, float* d, int B, int C, int H, int W, int M,
                                               const float* weights_host, float gscale, float* loss, int accumulate_loss,
                                               float* per_scale, void* ws, int64_t ws_bytes, void* stream) {
    VG_CHECK_ARG(a && b && loss && weights_host, VG_EINVAL);
    Plan p;
    VG_CHECK_ARG(make_plan(B, C, H, W, M, p), VG_EINVAL);
    for (int j = 0; j < MAXM; ++j) {
        p.w[j] = j < M ? (double)weights_host[j] : 0.0;
        VG_CHECK_ARG(j >= M || (std::isfinite(weights_host[j]) && weights_host[j] > 0.f), VG_EINVAL);
    }
    VG_CHECK_ARG(ws && ws_bytes >= p.total_floats * 4, VG_EINVAL);
    VG_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, VG_EALIGN);
    const Gauss11 gw = ssim_window();
    float* wsf = static_cast<float*>(ws);
    hipStream_t s = vg_stream(stream);
    int rc;
    if (M > 1) {
        const int64_t blocks = (int64_t)B * C * p.l[0].tiles_per_plane;
        vg_launch_timed(TIMING_FAMILY, msssim_pyramid_kernel, dim3((unsigned)blocks), dim3(NT), 0, s, a, b, wsf, p);
        if ((rc = VG_LAUNCH_RC())) return rc;
    }
    vg_launch_timed(TIMING_FAMILY, msssim_tile_kernel<false>, dim3((unsigned)p.tiles_total), dim3(NT), 0, s, a, b, wsf, p, gw);
    if ((rc = VG_LAUNCH_RC())) return rc;
    vg_launch_timed(TIMING_FAMILY, msssim_final_kernel, dim3(1), dim3(NT), 0, s, wsf, p, gscale, loss, accumulate_loss,
                    per_scale);
    if ((rc = VG_LAUNCH_RC()) || !d) return rc;
    vg_launch_timed(TIMING_FAMILY, msssim_tile_kernel<true>, dim3((unsigned)p.tiles_total), dim3(NT), 0, s, a, b, wsf, p, gw);
    if ((rc = VG_LAUNCH_RC())) return rc;
    const int64_t total = (int64_t)B * C * H * W;
    const int64_t blocks = (total + NT - 1) / NT;
    vg_launch_timed(TIMING_FAMILY, msssim_collapse_kernel, dim3((unsigned)blocks), dim3(NT), 0, s, d, (const float*)wsf, p,
                    total);
    return VG_LAUNCH_RC();
}
