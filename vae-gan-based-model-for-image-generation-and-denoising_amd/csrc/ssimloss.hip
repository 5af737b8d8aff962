// SSIM reconstruction loss, forward AND backward in one launch: the metric's contract (vg_ssim, pointwise.hip) made
// differentiable.  a (reconstruction), b (target): NCHW f32 in [-1, 1], u = (a + 1) / 2, v = (b + 1) / 2; with the maps of
// ssim_tile.hpp (S and its derivative maps Dm, Du, Dc over the interior pixels p in [5, H - 5) x [5, W - 5), w the window):
//
//   loss[0] (+)= 1 - (1 / n) sum_p S(p),   n = B C (H - 10)(W - 10)
//   d[q] += -gscale / (2 n) [ (w * Dm)(q) + 2 u(q) (w * Du)(q) + v(q) (w * Dc)(q) ]        for EVERY pixel q of the plane
//
// The tile pass -- staging with the per-tile shift, the four separable passes, the pointwise step without fma contraction,
// the window -- is csrc/ssim_tile.hpp, shared with msssim.hip; the reasoning about cancellation and contraction (why
// identical images give S = 1 exactly and a flat tile zero variance) is there.  What is here: a workgroup of 256 threads
// owns a 32 x 32 tile of d of one (image, channel) plane, found from blockIdx; a null d ends the workgroup after the
// forward sum, so forward and backward share one launch (the forward-only call still computes every item of the forward
// passes); ONE read-modify-write of the tile's own d pixels; one f32 partial of the tile's S sum per workgroup, which one
// wave sums in f64 in a fixed order (the second launch).  No host synchronisation: capturable.
#include "common.hpp"

#include <climits>
#include <cmath>

namespace {

#include "ssim_tile.hpp"

__global__ __launch_bounds__(NT) void ssim_loss_tile_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            float* __restrict__ d, int H, int W, int tiles_x,
                                                            int tiles_per_plane, Gauss11 gw, float coef,
                                                            float* __restrict__ partial) {
    __shared__ float sin_[SSIM_LDS_IN];
    __shared__ float tmp[SSIM_LDS_TMP];
    __shared__ float redf[4][2];
    __shared__ double redd[4];
    float* su = sin_;
    float* sv = sin_ + RI * RIP;
    float* sD = sin_;                                   // the derivative maps take the staged inputs' place
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % tiles_per_plane;
    const int64_t plane = blockIdx.x / tiles_per_plane;
    const int ty0 = (tile / tiles_x) * TS, tx0 = (tile % tiles_x) * TS;

    const SsimShift sh = ssim_stage_shift(a + plane * H * W, b + plane * H * W, H, W, ty0, tx0, su, sv, redf);
    const int qc = tid % TS, qr0 = (tid / TS) * 4;      // the thread's own four d pixels
    float uq[4], vq[4];
    ssim_own_pixels(su, sv, qc, qr0, uq, vq);
    ssim_fwd_rows(su, sv, tmp, gw, false);
    __syncthreads();                                    // su, sv are dead from here on
    const double acc = ssim_fwd_cols(tmp, sD, gw, H, W, ty0, tx0, sh, false, d != nullptr, false);
    const float sum = ssim_tile_sum(acc, redd);
    if (tid == 0) partial[blockIdx.x] = sum;
    if (!d) return;                                     // forward only (uniform over the workgroup)

    ssim_bwd_rows(sD, tmp, gw);
    __syncthreads();
    float wsum[3][4];
    ssim_bwd_cols(tmp, gw, qc, qr0, wsum);
    float* pd = d + plane * H * W;
    const int x = tx0 + qc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = ty0 + qr0 + j;
        if (y < H && x < W) pd[(int64_t)y * W + x] += ssim_grad_pixel(coef, wsum, uq, vq, j);
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
    const Gauss11 gw = ssim_window();
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
