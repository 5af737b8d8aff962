// SSIM reconstruction loss, forward AND backward in one launch: the metric's contract (vg_ssim, pointwise.hip) made
// differentiable.  a (reconstruction), b (target): NCHW f32 in [-1, 1], u = (a + 1) / 2, v = (b + 1) / 2; g the normalised
// 11-tap Gaussian (sigma 1.5), w = g (x) g; interior pixels p in [5, H - 5) x [5, W - 5):
//
//   mu_u = sum w u, mu_v = sum w v, s_uu = sum w u^2 - mu_u^2, s_vv likewise, s_uv = sum w u v - mu_u mu_v
//   A1 = 2 mu_u mu_v + c1, A2 = 2 s_uv + c2, B1 = mu_u^2 + mu_v^2 + c1, B2 = s_uu + s_vv + c2, S = A1 A2 / (B1 B2)
//   loss[0] (+)= 1 - (1 / n) sum_p S(p),   n = B C (H - 10)(W - 10)
//   Du = -A1 A2 / (B1 B2^2), Dc = 2 A1 / (B1 B2), Dm = 2 mu_v A2 / (B1 B2) - 2 mu_u A1 A2 / (B1^2 B2) - 2 mu_u Du - mu_v Dc
//   d[q] += -gscale / (2 n) [ (w * Dm)(q) + 2 u(q) (w * Du)(q) + v(q) (w * Dc)(q) ]        for EVERY pixel q of the plane
//
// (* = the transposed, full correlation with w; the D maps are zero outside the interior.)
//
// Shape: a workgroup of 256 threads owns a 32 x 32 tile of d of one (image, channel) plane.  It stages the tile and its
// 10-pixel halo of u and v (52 x 52 each) in LDS, runs the five forward maps as a row pass (52 x 42, three columns per
// thread) and a column pass (42 x 42, three rows per thread), forms S and the three derivative maps of the 42 x 42 pixels
// within 5 of its tile -- over the staged inputs, which only the tile's own pixels are read from again, and those are in
// registers by then -- runs them through a row pass (42 x 32) and a column pass (32 x 32, four rows per thread) and does
// ONE read-modify-write of its own d pixels.  Every d element has exactly one owner: no atomics, the same bits run to
// run.  S is summed over the interior pixels INSIDE the tile (each belongs to one tile) in f64, one f32 partial per
// workgroup; one wave sums the partials in f64 in a fixed order (the second launch).
//
// Cancellation: sum w u^2 - mu^2 of the raw values loses ~1e-7 against c2 = 9e-4 on flat windows (pointwise.hip's
// ssim_kernel centres per output pixel, which is not separable).  A variance does not move with the origin: the workgroup
// subtracts ONE constant per tile and input (the mean of the staged pixels) before the moments, so a flat tile has
// exactly zero variance, and the gradient is evaluated in the shifted variables too:
//   Dm' = 2 mu_v A2 / (B1 B2) - 2 mu_u A1 A2 / (B1^2 B2) - 2 (mu_u - cu) Du - (mu_v - cv) Dc,   u(q) - cu, v(q) - cv for u(q), v(q)
// -- the same sum, with products of small numbers where the raw form cancels products of large ones.  S is formed as
// (A1 / B1)(A2 / B2) and the pointwise step runs without fma contraction, so that identical images give S = 1 exactly and
// a gradient of zero or rounding residue (see the comment there; DESIGN.md section 4.4f has what was measured).
//
// LDS: 2 x 52 x 53 + 5 x 52 x 43 floats = 66.8 KB -> two workgroups per CU.  No host synchronisation: capturable.
#include "common.hpp"

#include <climits>
#include <cmath>

namespace {

constexpr int NT = 256;                 // threads per workgroup
constexpr int TS = 32;                  // tile of d pixels (TS x TS)
constexpr int KW = 11, HW5 = 5;         // window, half window
constexpr int RI = TS + 4 * HW5;        // 52: staged inputs (tile + 10 each side)
constexpr int RS = TS + 2 * HW5;        // 42: SSIM / derivative maps (tile + 5 each side)
constexpr int RIP = RI + 1, RSP = RS + 1, TSP = TS + 1;      // padded LDS rows
static_assert(RS % 3 == 0 && TS % 4 == 0 && (TS / 4) * TS == NT, "thread maps below");
static_assert(3 * RS * RSP <= 2 * RI * RIP && 3 * RS * TSP <= 5 * RI * RSP, "aliased LDS regions");

struct Gauss11 { float g[KW]; };

__global__ __launch_bounds__(NT) void ssim_loss_tile_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            float* __restrict__ d, int H, int W, int tiles_x,
                                                            int tiles_per_plane, Gauss11 gw, float coef,
                                                            float* __restrict__ partial) {
    __shared__ float sin_[2 * RI * RIP];        // u - cu, v - cv; later the three derivative maps [3][RS][RSP]
    __shared__ float tmp[5 * RI * RSP];         // row-pass results [5][RI][RSP]; later the backward's [3][RS][TSP]
    __shared__ float redf[4][2];
    __shared__ double redd[4];
    float* su = sin_;
    float* sv = sin_ + RI * RIP;
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % tiles_per_plane;
    const int64_t plane = blockIdx.x / tiles_per_plane;
    const int ty0 = (tile / tiles_x) * TS, tx0 = (tile % tiles_x) * TS;
    const float* pa = a + plane * H * W;
    const float* pb = b + plane * H * W;

    // ---- stage the tile and its halo; pixels outside the plane read 0 and are never used by an interior window
    float tu = 0.f, tv = 0.f;
    for (int e = tid; e < RI * RI; e += NT) {
        const int i = e / RI, j = e % RI;
        const int y = ty0 - 2 * HW5 + i, x = tx0 - 2 * HW5 + j;
        float u = 0.f, v = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            u = (pa[(int64_t)y * W + x] + 1.f) * 0.5f;
            v = (pb[(int64_t)y * W + x] + 1.f) * 0.5f;
            tu += u;
            tv += v;
        }
        su[i * RIP + j] = u;
        sv[i * RIP + j] = v;
    }
    tu = wave_sum(tu);
    tv = wave_sum(tv);
    if ((tid & 63) == 0) { redf[tid >> 6][0] = tu; redf[tid >> 6][1] = tv; }
    __syncthreads();
    const int ny = min(ty0 + TS + 2 * HW5, H) - max(ty0 - 2 * HW5, 0), nx = min(tx0 + TS + 2 * HW5, W) - max(tx0 - 2 * HW5, 0);
    const float inv_cnt = 1.f / (float)(ny * nx);
    const float cu = (redf[0][0] + redf[1][0] + redf[2][0] + redf[3][0]) * inv_cnt;
    const float cv = (redf[0][1] + redf[1][1] + redf[2][1] + redf[3][1]) * inv_cnt;
    for (int e = tid; e < RI * RI; e += NT) {          // the elements this thread wrote itself
        const int i = e / RI, j = e % RI;
        su[i * RIP + j] -= cu;
        sv[i * RIP + j] -= cv;
    }
    __syncthreads();

    // the thread's own four d pixels (column qc, rows qr0 .. qr0 + 3 of the tile): u - cu, v - cv, kept for the last step
    const int qc = tid % TS, qr0 = (tid / TS) * 4;
    float uq[4], vq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uq[j] = su[(qr0 + j + 2 * HW5) * RIP + qc + 2 * HW5];
        vq[j] = sv[(qr0 + j + 2 * HW5) * RIP + qc + 2 * HW5];
    }

    // ---- forward row pass: [RI rows][RS columns], three adjacent columns per thread
    for (int it = tid; it < RI * (RS / 3); it += NT) {
        const int r = it / (RS / 3), c0 = (it % (RS / 3)) * 3;
        float xu[KW + 2], xv[KW + 2];
#pragma unroll
        for (int k = 0; k < KW + 2; ++k) {
            xu[k] = su[r * RIP + c0 + k];
            xv[k] = sv[r * RIP + c0 + k];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                const float wu = gw.g[k] * xu[j + k], wv = gw.g[k] * xv[j + k];
                m0 += wu;
                m1 += wv;
                m2 += wu * xu[j + k];
                m3 += wv * xv[j + k];
                m4 += wu * xv[j + k];
            }
            const int o = r * RSP + c0 + j;
            tmp[o] = m0;
            tmp[RI * RSP + o] = m1;
            tmp[2 * RI * RSP + o] = m2;
            tmp[3 * RI * RSP + o] = m3;
            tmp[4 * RI * RSP + o] = m4;
        }
    }
    __syncthreads();                                   // sin_ is dead from here on: the derivative maps take its place

    // ---- forward column pass, S and the derivative maps: [RS][RS], three adjacent rows per thread
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    float* sD = sin_;
    double acc = 0.0;
    for (int it = tid; it < (RS / 3) * RS; it += NT) {
        const int c = it % RS, r0 = (it / RS) * 3;
        float m[5][3];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            float x[KW + 2];
#pragma unroll
            for (int k = 0; k < KW + 2; ++k) x[k] = tmp[(q * RI + r0 + k) * RSP + c];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < KW; ++k) s += gw.g[k] * x[j + k];
                m[q][j] = s;
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i = r0 + j;
            const int y = ty0 - HW5 + i, x = tx0 - HW5 + c;
            float dm = 0.f, du = 0.f, dc = 0.f;
            if (y >= HW5 && y < H - HW5 && x >= HW5 && x < W - HW5) {
                // Contraction OFF and the ratios A1 / B1, A2 / B2 formed first: for a == b (a perfect reconstruction) A1 and
                // B1, A2 and B2 are then the same roundings of the same numbers, S is exactly 1, dc = -2 du and dm = 0 --
                // the gradient of identical images stays at zero or rounding residue, and that of nearly identical
                // ones cancels what it should.  (An fma in one of two matching expressions leaves half an ulp of each
                // behind.)
#pragma clang fp contract(off)
                const float mus = m[0][j], mvs = m[1][j];              // shifted means
                const float suu = m[2][j] - mus * mus, svv = m[3][j] - mvs * mvs, suv = m[4][j] - mus * mvs;
                const float mu = mus + cu, mv = mvs + cv;
                const float A1 = 2.f * (mu * mv) + c1, A2 = 2.f * suv + c2;
                const float B1 = (mu * mu + mv * mv) + c1, B2 = (suu + svv) + c2;
                const float r1 = A1 / B1, r2 = A2 / B2;
                const float S = r1 * r2;
                if (i >= HW5 && i < HW5 + TS && c >= HW5 && c < HW5 + TS) acc += (double)S;      // the tile's own pixel
                du = -S / B2;
                dc = 2.f * r1 / B2;
                dm = (2.f * mv * r2 - 2.f * mu * S) / B1 - (2.f * mus * du + mvs * dc);
            }
            if (d) {
                sD[i * RSP + c] = dm;
                sD[RS * RSP + i * RSP + c] = du;
                sD[2 * RS * RSP + i * RSP + c] = dc;
            }
        }
    }
    acc = wave_sum_d(acc);
    if ((tid & 63) == 0) redd[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) partial[blockIdx.x] = (float)(redd[0] + redd[1] + redd[2] + redd[3]);
    if (!d) return;                                    // forward only (uniform over the workgroup)

    // ---- backward row pass: [RS rows][TS tile columns] of the three maps, four adjacent columns per thread
    for (int it = tid; it < RS * (TS / 4); it += NT) {
        const int r = it / (TS / 4), c0 = (it % (TS / 4)) * 4;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float x[KW + 3];
#pragma unroll
            for (int k = 0; k < KW + 3; ++k) x[k] = sD[q * RS * RSP + r * RSP + c0 + k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < KW; ++k) s += gw.g[k] * x[j + k];
                tmp[(q * RS + r) * TSP + c0 + j] = s;
            }
        }
    }
    __syncthreads();

    // ---- backward column pass and the one read-modify-write of the thread's own four d pixels
    float wsum[3][4];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        float x[KW + 3];
#pragma unroll
        for (int k = 0; k < KW + 3; ++k) x[k] = tmp[(q * RS + qr0 + k) * TSP + qc];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < KW; ++k) s += gw.g[k] * x[j + k];
            wsum[q][j] = s;
        }
    }
    float* pd = d + plane * H * W;
    const int x = tx0 + qc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = ty0 + qr0 + j;
        if (y < H && x < W) {
#pragma clang fp contract(off)
            const int64_t o = (int64_t)y * W + x;                      // (w * Dc = -2 w * Du exactly where a == b)
            pd[o] += coef * (wsum[0][j] + (2.f * uq[j] * wsum[1][j] + vq[j] * wsum[2][j]));
        }
    }
}

__global__ __launch_bounds__(64) void ssim_loss_final_kernel(const float* __restrict__ ws, int nparts, double n,
                                                             float* __restrict__ loss, int accumulate) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) s += (double)ws[i];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) {
        const float v = (float)(1.0 - s / n);
        loss[0] = accumulate ? loss[0] + v : v;
    }
}

inline int64_t ssim_loss_tiles(int B, int C, int H, int W) {
    return (int64_t)B * C * ((H + TS - 1) / TS) * ((W + TS - 1) / TS);
}

}  // namespace

extern "C" int64_t vg_ssim_loss_ws_floats(int B, int C, int H, int W) {
    VG_CHECK_ARG(B > 0 && C > 0 && H >= KW && W >= KW, VG_EINVAL);
    const int64_t t = ssim_loss_tiles(B, C, H, W);
    VG_CHECK_ARG(t <= INT_MAX, VG_EINVAL);
    return t;
}

extern "C" int vg_ssim_loss_forward_backward(const float* a, const float* b, float* d, int B, int C, int H, int W, float gscale,
                                             float* loss, int accumulate_loss, float* ws, int ws_capacity, void* stream) {
    VG_CHECK_ARG(a && b && loss && B > 0 && C > 0 && H >= KW && W >= KW, VG_EINVAL);
    const int64_t tiles = vg_ssim_loss_ws_floats(B, C, H, W);
    VG_CHECK_ARG(tiles > 0 && ws && (int64_t)ws_capacity >= tiles, VG_EINVAL);
    Gauss11 gw;
    double g[KW], gs = 0.0;
    for (int k = 0; k < KW; ++k) gs += (g[k] = std::exp(-((k - HW5) * (k - HW5)) / (2.0 * 1.5 * 1.5)));
    for (int k = 0; k < KW; ++k) gw.g[k] = (float)(g[k] / gs);
    const double n = (double)B * C * (H - 2 * HW5) * (double)(W - 2 * HW5);
    const float coef = (float)(-(double)gscale / (2.0 * n));
    const int tiles_x = (W + TS - 1) / TS, tiles_per_plane = tiles_x * ((H + TS - 1) / TS);
    hipLaunchKernelGGL(ssim_loss_tile_kernel, dim3((unsigned)tiles), dim3(NT), 0, vg_stream(stream), a, b, d, H, W, tiles_x,
                       tiles_per_plane, gw, coef, ws);
    int rc = VG_LAUNCH_RC();
    if (rc) return rc;
    hipLaunchKernelGGL(ssim_loss_final_kernel, dim3(1), dim3(64), 0, vg_stream(stream), ws, (int)tiles, n, loss,
                       accumulate_loss);
    return VG_LAUNCH_RC();
}
