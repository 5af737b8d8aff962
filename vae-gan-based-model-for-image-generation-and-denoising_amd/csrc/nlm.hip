// Classical-denoiser baseline (include/vaegan_hip.h "Non-local means baseline and blind noise estimate"): pixelwise non-local
// means with a uniform patch kernel (Buades, Coll & Morel 2005) and Immerkaer's (1996) noise-level estimate.  No MFMA: the
// filter is VALU / LDS work, (2R+1)^2 window offsets per output pixel.
//
// vg_nlm_denoise.  One workgroup of 256 threads owns one 16 x 16 output tile of one image.  It stages the tile plus its P + R
// halo of all C channels in LDS once (reflection resolved while loading; 16-byte loads where a group of four columns lies
// inside the row and on the 16-byte grid, single floats elsewhere), then walks the K = (2R+1)^2 offsets.  Per offset:
//   A  the channel-summed squared-difference map over the tile plus its P halo, (16+2P)^2 values, ONCE -> LDS
//   B  row box sums of it, (16+2P) x 16 values, 2P adds each                                              -> LDS
//   C  every thread: the column box sum of its pixel (2P adds), the weight, and w, w * x~ into registers
// so a pixel-offset costs 2(2P+1) LDS reads for the patch sum instead of C (2P+1)^2 differences.  Two barriers per offset
// (after A, after B): step A of the next offset may overwrite the map because every thread finished reading it before the
// second barrier, and step B of the next offset is behind the next first barrier, which a thread reaches only after its step C.
// P = 0 needs neither map nor barrier.  The pass-through decision is per image, hence per workgroup: no divergence inside
// the offset loop.  Rows of every LDS array are 48 floats apart (48 mod 32 = 16): the two 16-float row pieces a half-wave
// touches fall on disjoint banks.
//
// Arithmetic of one pixel-offset, all f32, in this order (tests/_nlm_ref.py counts its bound from it):
//   d = a - b; s = fma(d, d, s) over the channels; box sums by plain adds; d2 = S * inv_n; e = max(d2 - two_sigma2, 0);
//   arg = e * nscale, nscale = -log2(e) / h^2 per image; w = v_exp_f32(arg); den += w; num_c = fma(w, x~_c, num_c).
// The exponential is the hardware base-2 exponential (__builtin_amdgcn_exp2f -> v_exp_f32), one per pixel-offset: 1 ulp
// (2^-23 relative) by the ISA manual, results below 2^-126 flushed to 0 -- an absolute error the centre weight 1 dwarfs.
// The quotient num_c / den is one IEEE division (v_div_scale / v_div_fmas / v_div_fixup), not a reciprocal multiply.
//
// vg_noise_sigma.  One workgroup per image; waves take rows, lanes take columns (coalesced), the 3 x 3 mask is evaluated
// in f64 (every product by 1, 2, 4 and every sum of nine f32 is far inside f64), |.| accumulated in f64 per thread and combined in
// a fixed order: xor butterfly in the wave, the waves through LDS in wave order (the pattern of gradclip.hip).
#include <cmath>
#include "common.hpp"

namespace {

constexpr int NLM_T = 16;                  // output tile edge; NLM_T * NLM_T threads
constexpr int NLM_THREADS = NLM_T * NLM_T;
constexpr int NLM_PITCH = 48;              // floats between LDS rows: >= 16 + 2 * (3 + 10) = 42, and 48 mod 32 = 16
constexpr int NLM_MAX_P = 3, NLM_MAX_R = 10, NLM_MAX_C = 4;

__device__ __forceinline__ int nlm_reflect(int g, int n) {
    g = g < 0 ? -g : g;
    g = g > n - 1 ? 2 * (n - 1) - g : g;
    return g < 0 ? 0 : (g > n - 1 ? n - 1 : g);       // only coordinates no existing output reads need the clamp
}

struct NlmArgs {
    const float* x;
    float* y;
    const float* sigma;
    int C, H, W, R, sigma_stride;
    float h_factor, h_const;
};

template <int C, int P>
__global__ __launch_bounds__(NLM_THREADS) void nlm_kernel(const NlmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int DW = NLM_T + 2 * P;                 // edge of the squared-difference map
    const int H = a.H, W = a.W, R = a.R;
    const int HALO = P + R, LW = NLM_T + 2 * HALO;
    float* __restrict__ pix = lds;                                        // [C][LW][NLM_PITCH]
    float* __restrict__ dmap = lds + C * LW * NLM_PITCH;                  // [DW][NLM_PITCH]
    float* __restrict__ rsum = dmap + DW * NLM_PITCH;                     // [DW][NLM_T]
    const int tid = threadIdx.x, lx = tid & (NLM_T - 1), ly = tid >> 4;
    const int b = blockIdx.z, x0 = blockIdx.x * NLM_T, y0 = blockIdx.y * NLM_T;
    const int px = x0 + lx, py = y0 + ly;
    const bool live = px < W && py < H;
    const size_t plane = (size_t)H * W;
    const float* __restrict__ xb = a.x + (size_t)b * C * plane;
    float* __restrict__ yb = a.y + (size_t)b * C * plane;

    // per-image parameters; the decision is uniform over the workgroup
    const float sg = a.sigma ? a.sigma[(size_t)b * a.sigma_stride] : 0.f;
    const float h = a.h_factor * sg + a.h_const;
    if (!(h > 0.f) || !(fabsf(h) < INFINITY) || !(fabsf(sg) < INFINITY)) {
        if (live) {
#pragma unroll
            for (int c = 0; c < C; ++c) yb[c * plane + (size_t)py * W + px] = xb[c * plane + (size_t)py * W + px];
        }
        return;
    }
    const float two_s2 = 2.f * (sg * sg);
    const float nscale = fmaxf(-1.4426950408889634f / (h * h), -3.402823466e38f);    // h^2 underflowing to 0: no 0 * inf at e = 0
    constexpr float inv_n = 1.f / (float)(C * (2 * P + 1) * (2 * P + 1));

    // ---- stage the tile + halo, reflection resolved here ----
    {
        const int xs = x0 - HALO, ys = y0 - HALO;
        const int NG = (LW + 3) / 4 + 1;                                  // groups of four columns per row, any phase
        const int items = C * LW * NG;
        for (int e = tid; e < items; e += NLM_THREADS) {
            const int g = e % NG, row = e / NG, r = row % LW, c = row / LW;
            const int gy = nlm_reflect(ys + r, H);
            const float* __restrict__ src = xb + c * plane + (size_t)gy * W;
            const int m = (int)((reinterpret_cast<uintptr_t>(src) >> 2) & 3);       // src's phase on the 16-byte grid
            const int cs = xs - ((m + xs) & 3) + 4 * g;                   // (m + cs) % 4 == 0: src + cs is 16-byte aligned
            float* __restrict__ dst = pix + (c * LW + r) * NLM_PITCH;
            float v[4];
            if (cs >= 0 && cs + 3 <= W - 1) {
                const float4 q = *reinterpret_cast<const float4*>(src + cs);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = src[nlm_reflect(cs + k, W)];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int l = cs + k - xs;
                if (l >= 0 && l < LW) dst[l] = v[k];
            }
        }
    }
    __syncthreads();

    float den = 0.f, num[C];
#pragma unroll
    for (int c = 0; c < C; ++c) num[c] = 0.f;
    const float* __restrict__ ctr = pix + (HALO + ly) * NLM_PITCH + HALO + lx;      // this thread's pixel, channel 0

    for (int ty = -R; ty <= R; ++ty) {
        for (int tx = -R; tx <= R; ++tx) {
            const int shift = ty * NLM_PITCH + tx;
            float S;
            if constexpr (P == 0) {
                S = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float d = ctr[c * LW * NLM_PITCH] - ctr[c * LW * NLM_PITCH + shift];
                    S = fmaf(d, d, S);
                }
            } else {
                // A: squared differences, channel-summed, over the tile + P halo
                for (int e = tid; e < DW * DW; e += NLM_THREADS) {
                    const int i = e / DW, j = e - i * DW;
                    const float* __restrict__ q = pix + (R + i) * NLM_PITCH + R + j;
                    float s = 0.f;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const float d = q[c * LW * NLM_PITCH] - q[c * LW * NLM_PITCH + shift];
                        s = fmaf(d, d, s);
                    }
                    dmap[i * NLM_PITCH + j] = s;
                }
                __syncthreads();
                // B: row box sums
                for (int e = tid; e < DW * NLM_T; e += NLM_THREADS) {
                    const int i = e >> 4, j = e & (NLM_T - 1);
                    const float* __restrict__ q = dmap + i * NLM_PITCH + j;
                    float s = q[0];
#pragma unroll
                    for (int k = 1; k <= 2 * P; ++k) s += q[k];
                    rsum[e] = s;
                }
                __syncthreads();
                // C: column box sum of this thread's pixel
                S = rsum[tid];
#pragma unroll
                for (int k = 1; k <= 2 * P; ++k) S += rsum[tid + k * NLM_T];
            }
            const float d2 = S * inv_n;
            const float ee = fmaxf(d2 - two_s2, 0.f);
            const float w = __builtin_amdgcn_exp2f(ee * nscale);
            den += w;
#pragma unroll
            for (int c = 0; c < C; ++c) num[c] = fmaf(w, ctr[c * LW * NLM_PITCH + shift], num[c]);
        }
    }
    if (live) {
#pragma unroll
        for (int c = 0; c < C; ++c) yb[c * plane + (size_t)py * W + px] = __fdiv_rn(num[c], den);
    }
}

size_t nlm_lds_bytes(int C, int P, int R) {
    const int LW = NLM_T + 2 * (P + R), DW = NLM_T + 2 * P;
    return sizeof(float) * ((size_t)C * LW * NLM_PITCH + (P ? (size_t)DW * NLM_PITCH + (size_t)DW * NLM_T : 0));
}

template <int C>
void nlm_launch(int P, dim3 grid, size_t shm, hipStream_t s, const NlmArgs& a) {
    switch (P) {
    case 0: hipLaunchKernelGGL((nlm_kernel<C, 0>), grid, dim3(NLM_THREADS), shm, s, a); break;
    case 1: hipLaunchKernelGGL((nlm_kernel<C, 1>), grid, dim3(NLM_THREADS), shm, s, a); break;
    case 2: hipLaunchKernelGGL((nlm_kernel<C, 2>), grid, dim3(NLM_THREADS), shm, s, a); break;
    default: hipLaunchKernelGGL((nlm_kernel<C, 3>), grid, dim3(NLM_THREADS), shm, s, a); break;
    }
}

// ---- Immerkaer's noise estimate ----
constexpr int NS_THREADS = 1024;

__global__ __launch_bounds__(NS_THREADS) void noise_sigma_kernel(const float* __restrict__ x, int C, int H, int W,
                                                                 float* __restrict__ sigma, int sigma_stride, double k) {
    __shared__ double part[NS_THREADS / 64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* __restrict__ xb = x + (size_t)b * C * H * W;
    const int rows = C * (H - 2);
    double acc = 0.0;
    for (int row = wave; row < rows; row += NS_THREADS / 64) {
        const int c = row / (H - 2), i = row - c * (H - 2) + 1;
        const float* __restrict__ r1 = xb + ((size_t)c * H + i) * W;
        const float* __restrict__ r0 = r1 - W;
        const float* __restrict__ r2 = r1 + W;
        for (int j = 1 + lane; j <= W - 2; j += 64) {
            const double corners = ((double)r0[j - 1] + (double)r0[j + 1]) + ((double)r2[j - 1] + (double)r2[j + 1]);
            const double edges = ((double)r0[j] + (double)r2[j]) + ((double)r1[j - 1] + (double)r1[j + 1]);
            acc += fabs(corners - 2.0 * edges + 4.0 * (double)r1[j]);
        }
    }
    acc = wave_sum_d(acc);
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double S = part[0];
#pragma unroll
        for (int w = 1; w < NS_THREADS / 64; ++w) S += part[w];
        sigma[(size_t)b * sigma_stride] = (float)(S * k);
    }
}

}  // namespace

extern "C" int vg_nlm_denoise(const float* x, float* y, int B, int C, int H, int W, int patch_radius, int search_radius,
                              const float* sigma, int sigma_stride, float h_factor, float h_const, void* stream) {
    VG_CHECK_ARG(x && y, VG_EINVAL);
    VG_CHECK_ARG(B >= 1 && C >= 1 && C <= NLM_MAX_C && H >= 1 && W >= 1, VG_EINVAL);
    VG_CHECK_ARG(patch_radius >= 0 && patch_radius <= NLM_MAX_P && search_radius >= 1 && search_radius <= NLM_MAX_R, VG_EINVAL);
    VG_CHECK_ARG((H < W ? H : W) >= patch_radius + search_radius + 1, VG_EINVAL);
    VG_CHECK_ARG(!sigma || sigma_stride >= 1, VG_EINVAL);
    VG_CHECK_ARG(std::isfinite(h_factor) && std::isfinite(h_const) && h_factor >= 0.f && h_const >= 0.f, VG_EINVAL);
    VG_CHECK_ARG(h_factor > 0.f || h_const > 0.f, VG_EINVAL);
    // limits: the grid (B and the tile rows in its z / y dimensions) and int32 element counts
    const int64_t total = (int64_t)B * C * H * W;
    VG_CHECK_ARG(total <= 0x7fffffffLL && B <= 65535 && (H + NLM_T - 1) / NLM_T <= 65535, VG_EINVAL);
    VG_CHECK_ARG(!sigma || (int64_t)(B - 1) * sigma_stride <= 0x7fffffffLL, VG_EINVAL);
    {   // aliasing: any overlap of the two buffers (y == x included)
        const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(y);
        const uintptr_t bytes = (uintptr_t)total * sizeof(float);
        VG_CHECK_ARG(xa + bytes <= ya || ya + bytes <= xa, VG_EINVAL);
    }
    VG_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3u) == 0 && (reinterpret_cast<uintptr_t>(y) & 3u) == 0 &&
                 (reinterpret_cast<uintptr_t>(sigma) & 3u) == 0, VG_EALIGN);
    NlmArgs a{x, y, sigma, C, H, W, search_radius, sigma ? sigma_stride : 0, h_factor, h_const};
    const dim3 grid((W + NLM_T - 1) / NLM_T, (H + NLM_T - 1) / NLM_T, B);
    const size_t shm = nlm_lds_bytes(C, patch_radius, search_radius);
    hipStream_t s = vg_stream(stream);
    switch (C) {
    case 1: nlm_launch<1>(patch_radius, grid, shm, s, a); break;
    case 2: nlm_launch<2>(patch_radius, grid, shm, s, a); break;
    case 3: nlm_launch<3>(patch_radius, grid, shm, s, a); break;
    default: nlm_launch<4>(patch_radius, grid, shm, s, a); break;
    }
    return VG_LAUNCH_RC();
}

extern "C" int vg_noise_sigma(const float* x, int B, int C, int H, int W, float* sigma, int sigma_stride, void* stream) {
    VG_CHECK_ARG(x && sigma, VG_EINVAL);
    VG_CHECK_ARG(B >= 1 && C >= 1 && H >= 3 && W >= 3 && sigma_stride >= 1, VG_EINVAL);
    // limits: one workgroup per image in grid.x; the row counter C * (H - 2) and the strided output index are int32
    VG_CHECK_ARG((int64_t)C * (H - 2) <= 0x7fffffffLL && (int64_t)(B - 1) * sigma_stride <= 0x7fffffffLL, VG_EINVAL);
    VG_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3u) == 0 && (reinterpret_cast<uintptr_t>(sigma) & 3u) == 0, VG_EALIGN);
    const double k = std::sqrt(3.14159265358979323846 / 2.0) / (6.0 * (double)C * (double)(H - 2) * (double)(W - 2));
    hipLaunchKernelGGL(noise_sigma_kernel, dim3(B), dim3(NS_THREADS), 0, vg_stream(stream), x, C, H, W, sigma, sigma_stride, k);
    return VG_LAUNCH_RC();
}
