// Radial power spectra (include/vaegan_hip.h "Spectral generation metric"): a separable complex transform of every channel
// plane by two dense matrix products on v_mfma_f64_16x16x4_f64, the squared modulus summed over the channels, and a
// table-driven (CSR) weighted bin sum.  The transform matrices, the weight and the bins are the CALLER's tables
// (spectrum.py builds windowed DFT tables and radial bins), so integer tables and integer images give integer results.
//   spectrum_mean_kernel    m = (sum of a plane) / (H W), one workgroup per plane (center = 1 only)
//   spectrum_power_kernel   Y = (x - m) tw, Z = th Y, P = sum_c |Z|^2 for one image and 16 output columns v
//   spectrum_bins_*_kernel  prof[b][k] = sum over the bin's CSR entries, ascending
//   spectrum_accum_kernel   running sum and sum of squares of the profiles, one thread per bin
// A workgroup of the power kernel (4 waves) keeps the H x 16 complex Y block of one channel in LDS (2 * 16 * 8 bytes a row,
// 64 KB at H = 256) and the |Z|^2 sums in registers over the channel loop.  Stage 1 streams the plane straight from global
// memory into the A operand: with k = 4 q + j for MFMA j of a 16-wide step a lane's four values are adjacent in the row.
// Stage 2 reads th from global (L2) as A and Y from LDS as B with k = q + 4 j: lanes 0 .. 31 then read two adjacent LDS rows,
// 64 distinct banks of ds_read_b64.  Rows >= H, columns >= W or >= Wh are staged as zeros and never multiplied in.
#include "common.hpp"

typedef __attribute__((ext_vector_type(4))) double f64x4;

namespace {

constexpr int kSpMax = 256;        // largest H, W
constexpr int kSpVB = 16;          // output columns v per workgroup
constexpr int kSpThreads = 256;
constexpr int kSpTilesPerWave = kSpMax / 16 / (kSpThreads / 64);      // 16-row tiles of u a wave owns at H = 256

// partial[t] = sum of plane[i], i = t, t + 256, ... ascending; then partial[t] += partial[t + s] for s = 128, 64, ..., 1.
__global__ __launch_bounds__(kSpThreads) void spectrum_mean_kernel(const float* __restrict__ x, int HW,
                                                                   double* __restrict__ mean) {
    __shared__ double part[kSpThreads];
    const int t = threadIdx.x;
    const float* __restrict__ p = x + (int64_t)blockIdx.x * HW;
    double a = 0.0;
    for (int i = t; i < HW; i += kSpThreads) a += (double)p[i];
    part[t] = a;
    __syncthreads();
    for (int s = kSpThreads / 2; s > 0; s >>= 1) {
        if (t < s) part[t] += part[t + s];
        __syncthreads();
    }
    if (t == 0) mean[blockIdx.x] = part[0] / (double)HW;
}

// grid (images, ceil(Wh / 16)); dynamic LDS: 2 * Hp * 16 doubles, Hp = H rounded up to 16.
__global__ __launch_bounds__(kSpThreads) void spectrum_power_kernel(const float* __restrict__ x, int C, int H, int W, int Wh,
                                                                    const double* __restrict__ mean,
                                                                    const double* __restrict__ tw_re,
                                                                    const double* __restrict__ tw_im,
                                                                    const double* __restrict__ th_re,
                                                                    const double* __restrict__ th_im,
                                                                    double* __restrict__ power) {
    extern __shared__ __attribute__((aligned(16))) double ylds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int b = blockIdx.x, v0 = blockIdx.y * kSpVB;
    const int ntiles = (H + 15) >> 4, Hp = ntiles << 4;
    double* __restrict__ yre = ylds;
    double* __restrict__ yim = ylds + Hp * kSpVB;
    const int v = v0 + r;
    const bool vin = v < Wh;

    f64x4 P[kSpTilesPerWave];
#pragma unroll
    for (int t = 0; t < kSpTilesPerWave; ++t) P[t] = f64x4{0.0, 0.0, 0.0, 0.0};

    for (int c = 0; c < C; ++c) {
        const int64_t pl = (int64_t)b * C + c;
        const float* __restrict__ plane = x + pl * H * W;
        const double m = mean ? mean[pl] : 0.0;

        // ---- stage 1: Y[y][v] = sum_x (x[y][x] - m) tw[x][v] ----
        for (int rt = wave; rt < ntiles; rt += kSpThreads / 64) {
            const int y = rt * 16 + r;
            const bool yin = y < H;
            const float* __restrict__ row = plane + (int64_t)(yin ? y : 0) * W;
            f64x4 are = {0.0, 0.0, 0.0, 0.0}, aim = {0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < W; k0 += 16) {
                double a[4], br[4], bi[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int kx = k0 + 4 * q + j;
                    const bool kin = kx < W;
                    a[j] = (yin && kin) ? (double)row[kx] - m : 0.0;
                    br[j] = (kin && vin) ? tw_re[kx * Wh + v] : 0.0;
                    bi[j] = (kin && vin) ? tw_im[kx * Wh + v] : 0.0;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    are = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], br[j], are, 0, 0, 0);
                    aim = __builtin_amdgcn_mfma_f64_16x16x4f64(a[j], bi[j], aim, 0, 0, 0);
                }
            }
            // f64 C/D layout: col = lane & 15 (v), row = (lane >> 4) + 4 * reg (y inside the tile)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int yy = rt * 16 + q + 4 * g;
                yre[yy * kSpVB + r] = are[g];
                yim[yy * kSpVB + r] = aim[g];
            }
        }
        __syncthreads();

        // ---- stage 2: Z[u][v] = sum_y th[u][y] Y[y][v] (complex), P += |Z|^2 ----
#pragma unroll
        for (int t = 0; t < kSpTilesPerWave; ++t) {
            const int ut = wave + (kSpThreads / 64) * t;
            if (ut < ntiles) {
                const int u = ut * 16 + r;
                const bool uin = u < H;
                const double* __restrict__ tr = th_re + (int64_t)(uin ? u : 0) * H;
                const double* __restrict__ ti = th_im + (int64_t)(uin ? u : 0) * H;
                f64x4 zre = {0.0, 0.0, 0.0, 0.0}, zim = {0.0, 0.0, 0.0, 0.0};
                for (int k0 = 0; k0 < Hp; k0 += 4) {
                    const int y = k0 + q;
                    const bool in = uin && y < H;
                    const double ar = in ? tr[y] : 0.0, ai = in ? ti[y] : 0.0;
                    const double yr = yre[y * kSpVB + r], yi = yim[y * kSpVB + r];
                    zre = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, yr, zre, 0, 0, 0);
                    zre = __builtin_amdgcn_mfma_f64_16x16x4f64(-ai, yi, zre, 0, 0, 0);     // negating an operand is exact
                    zim = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, yi, zim, 0, 0, 0);
                    zim = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, yr, zim, 0, 0, 0);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) P[t][g] += zre[g] * zre[g] + zim[g] * zim[g];
            }
        }
        __syncthreads();                                   // the next channel overwrites Y
    }

    // row u = tile * 16 + (lane >> 4) + 4 * reg, column v = v0 + (lane & 15)
    double* __restrict__ dst = power + (int64_t)b * H * Wh;
#pragma unroll
    for (int t = 0; t < kSpTilesPerWave; ++t) {
        const int ut = wave + (kSpThreads / 64) * t;
        if (ut < ntiles) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int u = ut * 16 + q + 4 * g;
                if (u < H && vin) dst[(int64_t)u * Wh + v] = P[t][g];
            }
        }
    }
}

// The CSR range of bin k, or an empty one: nnz = bin_start[n_bins] clamped into [0, H Wh]; a bin whose bounds are not
// 0 <= s <= e <= nnz contributes nothing, so no entry of `order` beyond the table's own length is read.
__device__ __forceinline__ void spectrum_bin_range(const int32_t* __restrict__ bin_start, int n_bins, int k, int HWh, int& s,
                                                   int& e) {
    int nnz = bin_start[n_bins];
    nnz = nnz < 0 ? 0 : (nnz > HWh ? HWh : nnz);
    s = bin_start[k];
    e = bin_start[k + 1];
    if (s < 0 || e < s || e > nnz) s = e = 0;
}

// A wavefront per (image, bin): 64 entries at a time, one per lane (an entry outside [0, H Wh) is never dereferenced and
// adds nothing), added in ascending j by every lane alike.
__global__ __launch_bounds__(kSpThreads) void spectrum_bins_wave_kernel(const double* __restrict__ power,
                                                                        const double* __restrict__ weight,
                                                                        const int32_t* __restrict__ order,
                                                                        const int32_t* __restrict__ bin_start, int n_bins,
                                                                        int HWh, int64_t total, double* __restrict__ prof) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (kSpThreads / 64) + (threadIdx.x >> 6);
    if (w >= total) return;
    const int64_t b = w / n_bins;
    const int k = (int)(w - b * n_bins);
    int s, e;
    spectrum_bin_range(bin_start, n_bins, k, HWh, s, e);
    const double* __restrict__ P = power + b * HWh;
    double acc = 0.0;
    for (int j0 = s; j0 < e; j0 += 64) {
        const int j = j0 + lane;
        double term = 0.0;
        bool ok = false;
        if (j < e) {
            const int o = order[j];
            if (o >= 0 && o < HWh) { term = weight[o] * P[o]; ok = true; }
        }
        const int n = e - j0 < 64 ? e - j0 : 64;
        for (int i = 0; i < n; ++i) {
            const double ti = __shfl(term, i);
            const int oki = __shfl((int)ok, i);
            if (oki) acc += ti;
        }
    }
    if (lane == 0) prof[w] = acc;
}

// One thread per (image, bin): the form for short bins (the identity table of the mean 2-D spectrum).
__global__ __launch_bounds__(kSpThreads) void spectrum_bins_thread_kernel(const double* __restrict__ power,
                                                                          const double* __restrict__ weight,
                                                                          const int32_t* __restrict__ order,
                                                                          const int32_t* __restrict__ bin_start, int n_bins,
                                                                          int HWh, int64_t total, double* __restrict__ prof) {
    const int64_t w = (int64_t)blockIdx.x * kSpThreads + threadIdx.x;
    if (w >= total) return;
    const int64_t b = w / n_bins;
    const int k = (int)(w - b * n_bins);
    int s, e;
    spectrum_bin_range(bin_start, n_bins, k, HWh, s, e);
    const double* __restrict__ P = power + b * HWh;
    double acc = 0.0;
    for (int j = s; j < e; ++j) {
        const int o = order[j];
        if (o >= 0 && o < HWh) acc += weight[o] * P[o];
    }
    prof[w] = acc;
}

__global__ __launch_bounds__(kSpThreads) void spectrum_accum_kernel(const double* __restrict__ prof, int B, int n_bins,
                                                                    double* __restrict__ sum, double* __restrict__ sumsq) {
    const int k = blockIdx.x * kSpThreads + threadIdx.x;
    if (k >= n_bins) return;
    double s = sum[k], ss = sumsq[k];
    for (int b = 0; b < B; ++b) {
        const double p = prof[(int64_t)b * n_bins + k];
        s += p;
        ss = fma(p, p, ss);                                 // one rounding, whatever the compiler's contraction setting
    }
    sum[k] = s;
    sumsq[k] = ss;
}

bool sp_aligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1u)) == 0; }

struct SpBuf { const void* p; int64_t bytes; };
bool sp_overlap(const SpBuf& a, const SpBuf& b) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a.p), pb = reinterpret_cast<uintptr_t>(b.p);
    return pa < pb + (uintptr_t)b.bytes && pb < pa + (uintptr_t)a.bytes;
}

bool sp_shape_ok(int B, int C, int H, int W) {
    if (B < 1 || C < 1 || C > 4 || H < 2 || H > kSpMax || W < 2 || W > kSpMax) return false;
    return (int64_t)B * C * H * W <= 2147483647ll;
}

}  // namespace

extern "C" int vg_spectrum_ws_bytes(int B, int C, int H, int W, int64_t* bytes) {
    VG_CHECK_ARG(bytes && sp_shape_ok(B, C, H, W), VG_EINVAL);
    *bytes = 8 * ((int64_t)B * C + (int64_t)B * H * (W / 2 + 1));
    return 0;
}

extern "C" int vg_spectrum_profiles(const float* x, int B, int C, int H, int W, int center, const double* tw_re,
                                    const double* tw_im, const double* th_re, const double* th_im, const double* weight,
                                    const int32_t* order, const int32_t* bin_start, int n_bins, double* power, double* prof,
                                    void* ws, int64_t ws_bytes, void* stream) {
    VG_CHECK_ARG(x && tw_re && tw_im && th_re && th_im && weight && order && bin_start && prof && ws, VG_EINVAL);
    VG_CHECK_ARG(sp_shape_ok(B, C, H, W) && (center == 0 || center == 1), VG_EINVAL);
    const int Wh = W / 2 + 1, HWh = H * Wh;
    VG_CHECK_ARG(n_bins >= 1 && n_bins <= HWh && (int64_t)B * n_bins <= 2147483647ll, VG_EINVAL);
    int64_t need = 0;
    VG_CHECK_ARG(vg_spectrum_ws_bytes(B, C, H, W, &need) == 0 && ws_bytes >= need, VG_EINVAL);
    {   // aliasing: no output may overlap an input or another output (order's length is a device value: its first entry stands for it)
        const SpBuf in[] = {{x, 4ll * B * C * H * W}, {tw_re, 8ll * W * Wh}, {tw_im, 8ll * W * Wh}, {th_re, 8ll * H * H},
                            {th_im, 8ll * H * H}, {weight, 8ll * HWh}, {order, 4}, {bin_start, 4ll * (n_bins + 1)}};
        const SpBuf out[] = {{prof, 8ll * B * n_bins}, {ws, need}, {power, power ? 8ll * B * HWh : 0}};
        for (const SpBuf& o : out) {
            if (!o.p) continue;
            for (const SpBuf& i : in) VG_CHECK_ARG(!sp_overlap(o, i), VG_EINVAL);
            for (const SpBuf& o2 : out) VG_CHECK_ARG(&o == &o2 || !o2.p || !sp_overlap(o, o2), VG_EINVAL);
        }
    }
    VG_CHECK_ARG(sp_aligned(x, 4) && sp_aligned(order, 4) && sp_aligned(bin_start, 4) && sp_aligned(tw_re, 8) &&
                 sp_aligned(tw_im, 8) && sp_aligned(th_re, 8) && sp_aligned(th_im, 8) && sp_aligned(weight, 8) &&
                 sp_aligned(prof, 8) && sp_aligned(ws, 8) && (!power || sp_aligned(power, 8)), VG_EALIGN);
    hipStream_t st = vg_stream(stream);
    double* mean = static_cast<double*>(ws);
    double* pmap = power ? power : mean + (int64_t)B * C;
    if (center)
        hipLaunchKernelGGL(spectrum_mean_kernel, dim3((unsigned)(B * C)), dim3(kSpThreads), 0, st, x, H * W, mean);
    const int Hp = (H + 15) / 16 * 16;
    hipLaunchKernelGGL(spectrum_power_kernel, dim3((unsigned)B, (unsigned)((Wh + kSpVB - 1) / kSpVB)), dim3(kSpThreads),
                       (size_t)2 * Hp * kSpVB * sizeof(double), st, x, C, H, W, Wh, center ? mean : (const double*)nullptr,
                       tw_re, tw_im, th_re, th_im, pmap);
    const int64_t total = (int64_t)B * n_bins;
    if (HWh / n_bins >= 16)
        hipLaunchKernelGGL(spectrum_bins_wave_kernel, dim3((unsigned)((total + 3) / 4)), dim3(kSpThreads), 0, st, pmap, weight,
                           order, bin_start, n_bins, HWh, total, prof);
    else
        hipLaunchKernelGGL(spectrum_bins_thread_kernel, dim3((unsigned)((total + kSpThreads - 1) / kSpThreads)),
                           dim3(kSpThreads), 0, st, pmap, weight, order, bin_start, n_bins, HWh, total, prof);
    return VG_LAUNCH_RC();
}

extern "C" int vg_spectrum_accum(const double* prof, int B, int n_bins, double* sum, double* sumsq, void* stream) {
    VG_CHECK_ARG(prof && sum && sumsq, VG_EINVAL);
    VG_CHECK_ARG(B >= 1 && n_bins >= 1 && n_bins <= kSpMax * (kSpMax / 2 + 1) && (int64_t)B * n_bins <= 2147483647ll, VG_EINVAL);
    {
        const SpBuf p = {prof, 8ll * B * n_bins}, s = {sum, 8ll * n_bins}, q = {sumsq, 8ll * n_bins};
        VG_CHECK_ARG(!sp_overlap(p, s) && !sp_overlap(p, q) && !sp_overlap(s, q), VG_EINVAL);
    }
    VG_CHECK_ARG(sp_aligned(prof, 8) && sp_aligned(sum, 8) && sp_aligned(sumsq, 8), VG_EALIGN);
    hipLaunchKernelGGL(spectrum_accum_kernel, dim3((unsigned)((n_bins + kSpThreads - 1) / kSpThreads)), dim3(kSpThreads), 0,
                       vg_stream(stream), prof, B, n_bins, sum, sumsq);
    return VG_LAUNCH_RC();
}
