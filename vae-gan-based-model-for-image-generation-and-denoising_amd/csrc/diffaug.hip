// Differentiable augmentation of the Discriminator's inputs (Zhao et al., NeurIPS 2020, "DiffAugment"; not in the reference):
// a per-image colour change, translation and cutout applied to everything D sees, and its exact adjoint.  The contract --
// formula, operation order, partition of the two sums, parameter safety -- is stated in include/vaegan_hip.h, "Differentiable
// augmentation".  Streaming, HBM-bound: a pixel is a whole number of 16-byte units, a thread owns DA_LOADS pixels of a part
// and issues their loads before it consumes any; the parameter row and the slab's parts are uniform per workgroup.
#include "common.hpp"
#include "noise.hpp"

namespace {

constexpr int DA_THREADS = 256;
constexpr int DA_LOADS = 4;                              // independent 16-byte loads in flight per thread
constexpr int DA_PART = DA_THREADS * DA_LOADS;           // pixels per part (= per workgroup): fixed, not a launch choice
constexpr float DA_BIG = 1073741824.0f;                  // 2^30: an integer slot at or beyond it (or NaN) counts as 0

struct DaGeom { int N, PB, H, W, C, U, cut_h, cut_w, parts; };   // U: 16-byte units per pixel; parts: ceil(H W / DA_PART)

struct DaRow { float beta, s, k; int ty, tx, cy, cx, cut; };     // cut: 1 when this image has a cutout

// u01 / rint of include/vaegan_hip.h "Degraded pairs" (the forms degrade.hip uses for its own draws)
__device__ __forceinline__ float da_u01(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }
__device__ __forceinline__ int da_rint(uint32_t w, int lo, int hi) {
    return lo + (int)(((unsigned long long)(w >> 8) * (unsigned long long)(uint32_t)(hi - lo)) >> 24);
}
// an integer carried in f32: NaN or |v| >= 2^30 -> ok = false (the caller takes 0 / no cutout); else truncated toward zero
__device__ __forceinline__ int da_int(float v, bool& ok) {
    ok = fabsf(v) < DA_BIG;                              // false for NaN
    return ok ? (int)v : 0;
}

// The row of image n (row n % PB), uniform over the workgroup: every address derives from blockIdx and kernel arguments.
__device__ __forceinline__ DaRow da_row(const float* __restrict__ params, int n, const DaGeom& g) {
    const float* r = params + (int64_t)(n % g.PB) * 8;
    DaRow p;
    p.beta = r[0]; p.s = r[1]; p.k = r[2];
    bool oky, okx, okcy, okcx;
    p.ty = da_int(r[3], oky);
    p.tx = da_int(r[4], okx);
    p.cy = da_int(r[5], okcy);
    p.cx = da_int(r[6], okcx);
    p.cut = (g.cut_h > 0 && g.cut_w > 0 && okcy && okcx) ? 1 : 0;
    return p;
}

__device__ __forceinline__ bool da_in_cut(const DaRow& p, const DaGeom& g, int h, int w) {
    return p.cut && h >= p.cy && h < p.cy + g.cut_h && w >= p.cx && w < p.cx + g.cut_w;
}

// Source pixel of destination pixel (h, w), or -1 where the destination reads zeros.
//   forward : source (h + ty, w + tx), the cutout tested at the DESTINATION (h, w)
//   backward: source (h - ty, w - tx), the cutout tested at the SOURCE
template <bool BWD>
__device__ __forceinline__ int da_source(const DaRow& p, const DaGeom& g, int h, int w) {
    const int hs = BWD ? h - p.ty : h + p.ty;            // |ty| < 2^30, h < 2^30: no overflow
    const int ws = BWD ? w - p.tx : w + p.tx;
    if (hs < 0 || hs >= g.H || ws < 0 || ws >= g.W) return -1;
    if (BWD ? da_in_cut(p, g, hs, ws) : da_in_cut(p, g, h, w)) return -1;
    return hs * g.W + ws;
}

template <int DT> struct DaUnit { float v[ElemT<DT>::per16]; };

template <int DT> __device__ __forceinline__ DaUnit<DT> da_load(const void* base, int64_t unit);
template <> __device__ __forceinline__ DaUnit<VG_F32> da_load<VG_F32>(const void* base, int64_t unit) {
    const float4 r = reinterpret_cast<const float4*>(base)[unit];
    return DaUnit<VG_F32>{{r.x, r.y, r.z, r.w}};
}
template <> __device__ __forceinline__ DaUnit<VG_BF16> da_load<VG_BF16>(const void* base, int64_t unit) {
    const u32x4 r = reinterpret_cast<const u32x4*>(base)[unit];
    DaUnit<VG_BF16> o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o.v[2 * j] = __uint_as_float(r[j] << 16);
        o.v[2 * j + 1] = __uint_as_float(r[j] & 0xffff0000u);
    }
    return o;
}
template <int DT> __device__ __forceinline__ void da_store(void* base, int64_t unit, const DaUnit<DT>& u);
template <> __device__ __forceinline__ void da_store<VG_F32>(void* base, int64_t unit, const DaUnit<VG_F32>& u) {
    reinterpret_cast<float4*>(base)[unit] = float4{u.v[0], u.v[1], u.v[2], u.v[3]};
}
template <> __device__ __forceinline__ void da_store<VG_BF16>(void* base, int64_t unit, const DaUnit<VG_BF16>& u) {
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        r[j] = (uint32_t)ElemT<VG_BF16>::from_f32(u.v[2 * j]) | ((uint32_t)ElemT<VG_BF16>::from_f32(u.v[2 * j + 1]) << 16);
    reinterpret_cast<u32x4*>(base)[unit] = r;
}
template <int DT> __device__ __forceinline__ DaUnit<DT> da_zero_unit() {
    DaUnit<DT> z;
#pragma unroll
    for (int j = 0; j < ElemT<DT>::per16; ++j) z.v[j] = 0.f;
    return z;
}

// real channels of unit u of a pixel, added in ascending channel order onto acc
template <int DT> __device__ __forceinline__ float da_chan_sum(float acc, const DaUnit<DT>& x, int u, int C) {
#pragma clang fp contract(off)
    constexpr int E = ElemT<DT>::per16;
#pragma unroll
    for (int j = 0; j < E; ++j)
        if (u * E + j < C) acc = acc + x.v[j];
    return acc;
}

// out_c = (ks * v_c + b * m) + e on the real channels, zero on the pad channels
template <int DT> __device__ __forceinline__ DaUnit<DT> da_apply_unit(const DaUnit<DT>& x, int u, int C, float ks, float bm, float e) {
#pragma clang fp contract(off)
    constexpr int E = ElemT<DT>::per16;
    DaUnit<DT> o;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const float t = ks * x.v[j];
        const float r = (t + bm) + e;
        o.v[j] = (u * E + j < C) ? r : 0.f;
    }
    return o;
}

// Sum of one value per thread over the workgroup in a fixed order: xor butterfly (32, 16, .., 1) inside each wave, then the
// four wave sums in wave order.  Valid in every thread.
__device__ __forceinline__ float da_block_sum(float v) {
#pragma clang fp contract(off)
    __shared__ float part[DA_THREADS / 64];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = part[0];
#pragma unroll
    for (int w = 1; w < DA_THREADS / 64; ++w) s = s + part[w];
    return s;
}

// Launch 1: ws[n * parts + q] = sum over the pixels of part q of image n of the channel sum of the (forward: plain;
// backward: shifted and masked) input.  grid N * parts, image-major.
template <int DT, bool BWD>
__global__ __launch_bounds__(DA_THREADS) void diffaug_reduce_kernel(const void* __restrict__ in, const float* __restrict__ params,
                                                                    const DaGeom g, float* __restrict__ ws) {
#pragma clang fp contract(off)
    const int n = (int)(blockIdx.x / (unsigned)g.parts), q = (int)(blockIdx.x - (unsigned)n * (unsigned)g.parts);
    const int HW = g.H * g.W;
    const int64_t img = (int64_t)n * HW;
    DaRow p{};
    if (BWD) p = da_row(params, n, g);
    int src[DA_LOADS];
#pragma unroll
    for (int k = 0; k < DA_LOADS; ++k) {
        const int pix = q * DA_PART + k * DA_THREADS + (int)threadIdx.x;
        src[k] = -1;
        if (pix < HW) {
            if (BWD) {
                const int h = pix / g.W;
                src[k] = da_source<true>(p, g, h, pix - h * g.W);
            } else {
                src[k] = pix;
            }
        }
    }
    float s[DA_LOADS];
    if (g.U == 1) {
        DaUnit<DT> x[DA_LOADS];
#pragma unroll
        for (int k = 0; k < DA_LOADS; ++k) x[k] = da_load<DT>(in, img + (src[k] >= 0 ? src[k] : 0));   // all issued, unconditionally:
#pragma unroll
        for (int k = 0; k < DA_LOADS; ++k)                                                             // a pixel without a source
            if (src[k] < 0) x[k] = da_zero_unit<DT>();                                                 // reads pixel 0, discarded
#pragma unroll
        for (int k = 0; k < DA_LOADS; ++k) s[k] = da_chan_sum<DT>(0.f, x[k], 0, g.C);
    } else {
#pragma unroll
        for (int k = 0; k < DA_LOADS; ++k) {
            s[k] = 0.f;
            if (src[k] >= 0)
                for (int u = 0; u < g.U; ++u) s[k] = da_chan_sum<DT>(s[k], da_load<DT>(in, (img + src[k]) * g.U + u), u, g.C);
        }
    }
    const float total = da_block_sum((s[0] + s[1]) + (s[2] + s[3]));
    if (threadIdx.x == 0) ws[(int64_t)n * g.parts + q] = total;
}

// Launch 2: the transform (or its adjoint) of part q of image n.  grid N * parts, image-major.
template <int DT, bool BWD>
__global__ __launch_bounds__(DA_THREADS) void diffaug_apply_kernel(const void* __restrict__ in, void* __restrict__ out,
                                                                   const float* __restrict__ params, const DaGeom g,
                                                                   const float* __restrict__ ws) {
#pragma clang fp contract(off)
    const int n = (int)(blockIdx.x / (unsigned)g.parts), q = (int)(blockIdx.x - (unsigned)n * (unsigned)g.parts);
    const int HW = g.H * g.W;
    const int64_t img = (int64_t)n * HW;
    const DaRow p = da_row(params, n, g);
    // uniform coefficients: ks = k s, b = k - ks, c = 1 - k, e = c * (S / (C H W)) (+ beta, forward)
    const float ks = p.k * p.s;
    const float b = p.k - ks;
    const float c = 1.0f - p.k;
    float S = 0.f;
    if (ws != nullptr)
        for (int i = 0; i < g.parts; ++i) S = S + ws[(int64_t)n * g.parts + i];
    const float mean = S / (float)((int64_t)g.C * HW);
    const float cm = c * mean;
    const float e = BWD ? cm : cm + p.beta;
    const float fC = (float)g.C;

    int pix[DA_LOADS], src[DA_LOADS];
#pragma unroll
    for (int k = 0; k < DA_LOADS; ++k) {
        pix[k] = q * DA_PART + k * DA_THREADS + (int)threadIdx.x;
        src[k] = -1;
        if (pix[k] < HW) {
            const int h = pix[k] / g.W;
            src[k] = da_source<BWD>(p, g, h, pix[k] - h * g.W);
        }
    }
    if (g.U == 1) {
        DaUnit<DT> x[DA_LOADS];
#pragma unroll
        for (int k = 0; k < DA_LOADS; ++k) x[k] = da_load<DT>(in, img + (src[k] >= 0 ? src[k] : 0));   // all issued, unconditionally:
#pragma unroll
        for (int k = 0; k < DA_LOADS; ++k)                                                             // a pixel without a source
            if (src[k] < 0) x[k] = da_zero_unit<DT>();                                                 // reads pixel 0, discarded
#pragma unroll
        for (int k = 0; k < DA_LOADS; ++k) {
            if (pix[k] >= HW) continue;
            DaUnit<DT> y = da_zero_unit<DT>();
            if (BWD || src[k] >= 0) {                          // forward: a destination without a source is zero
                const float m = da_chan_sum<DT>(0.f, x[k], 0, g.C) / fC;
                y = da_apply_unit<DT>(x[k], 0, g.C, ks, b * m, e);
            }
            da_store<DT>(out, img + pix[k], y);
        }
    } else {
#pragma unroll
        for (int k = 0; k < DA_LOADS; ++k) {
            if (pix[k] >= HW) continue;
            const bool live = src[k] >= 0;
            float m = 0.f;
            if (live)
                for (int u = 0; u < g.U; ++u) m = da_chan_sum<DT>(m, da_load<DT>(in, (img + src[k]) * g.U + u), u, g.C);
            const float bm = b * (m / fC);
            for (int u = 0; u < g.U; ++u) {
                DaUnit<DT> y = da_zero_unit<DT>();
                if (BWD || live) {
                    const DaUnit<DT> x = live ? da_load<DT>(in, (img + src[k]) * g.U + u) : da_zero_unit<DT>();
                    y = da_apply_unit<DT>(x, u, g.C, ks, bm, e);
                }
                da_store<DT>(out, (img + pix[k]) * g.U + u, y);
            }
        }
    }
}

__global__ __launch_bounds__(256) void diffaug_params_kernel(const unsigned long long* __restrict__ rng, int B, int policy,
                                                             int H, int W, int sh_h, int sh_w, int cut_h, int cut_w,
                                                             float* __restrict__ out) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const unsigned long long seed = rng[0], step = rng[1];
    uint32_t w[8];                                         // word(draw, 8 b + i) = word i & 3 of block (8 b + i) >> 2
    uint32_t lo[4], hi[4];
    philox4x32_10(seed, step, VG_DRAW_AUGMENT, 2ull * (unsigned long long)b, lo);
    philox4x32_10(seed, step, VG_DRAW_AUGMENT, 2ull * (unsigned long long)b + 1ull, hi);
#pragma unroll
    for (int i = 0; i < 4; ++i) { w[i] = lo[i]; w[4 + i] = hi[i]; }
    float* o = out + (int64_t)b * 8;
    o[0] = (policy & 1) ? da_u01(w[0]) - 0.5f : 0.f;
    o[1] = (policy & 2) ? 2.0f * da_u01(w[1]) : 1.f;
    o[2] = (policy & 4) ? da_u01(w[2]) + 0.5f : 1.f;
    o[3] = (policy & 8) ? (float)da_rint(w[3], -sh_h, sh_h + 1) : 0.f;
    o[4] = (policy & 8) ? (float)da_rint(w[4], -sh_w, sh_w + 1) : 0.f;
    o[5] = (policy & 16) ? (float)(da_rint(w[5], 0, H + 1 - cut_h % 2) - cut_h / 2) : 0.f;
    o[6] = (policy & 16) ? (float)(da_rint(w[6], 0, W + 1 - cut_w % 2) - cut_w / 2) : 0.f;
    o[7] = 0.f;
}

int64_t da_parts(int H, int W) { return ((int64_t)H * W + DA_PART - 1) / DA_PART; }

template <bool BWD>
int da_launch(const void* in, void* out, const float* params, int N, int PB, int H, int W, int C, int CP, int cut_h,
              int cut_w, float* ws, int64_t ws_capacity, int dtype, void* stream) {
    VG_CHECK_ARG(in && out && params && in != out, VG_EINVAL);
    VG_CHECK_ARG(N >= 1 && PB >= 1 && H >= 1 && W >= 1 && C >= 1 && CP >= 1 && N % PB == 0 && C <= CP, VG_EINVAL);
    VG_CHECK_ARG(cut_h >= 0 && cut_w >= 0 && cut_h <= H && cut_w <= W, VG_EINVAL);
    VG_CHECK_ARG((int64_t)H * W < (1ll << 30), VG_EINVAL);                              // pixel indices are ints
    VG_CHECK_ARG(dtype == VG_F32 || dtype == VG_BF16, VG_ENOSUP);
    const int per16 = dtype == VG_F32 ? 4 : 8;
    VG_CHECK_ARG(CP % per16 == 0, VG_EALIGN);                                          // a pixel is whole 16-byte units
    const int64_t parts = da_parts(H, W);
    VG_CHECK_ARG((int64_t)N * parts < (1ll << 31), VG_EINVAL);                          // one workgroup per part
    VG_CHECK_ARG(ws == nullptr || ws_capacity >= (int64_t)N * parts, VG_EINVAL);
    VG_CHECK_ARG(vg_aligned16(in) && vg_aligned16(out) && vg_aligned16(params) && vg_aligned16(ws), VG_EALIGN);
    const DaGeom g{N, PB, H, W, C, CP / per16, cut_h, cut_w, (int)parts};
    const dim3 grid((unsigned)((int64_t)N * parts)), block(DA_THREADS);
    hipStream_t st = vg_stream(stream);
    if (ws != nullptr) {
        if (dtype == VG_F32)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(diffaug_reduce_kernel<VG_F32, BWD>), grid, block, 0, st, in, params, g, ws);
        else
            hipLaunchKernelGGL(HIP_KERNEL_NAME(diffaug_reduce_kernel<VG_BF16, BWD>), grid, block, 0, st, in, params, g, ws);
        const int rc = VG_LAUNCH_RC();
        if (rc) return rc;
    }
    if (dtype == VG_F32)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(diffaug_apply_kernel<VG_F32, BWD>), grid, block, 0, st, in, out, params, g,
                           (const float*)ws);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(diffaug_apply_kernel<VG_BF16, BWD>), grid, block, 0, st, in, out, params, g,
                           (const float*)ws);
    return VG_LAUNCH_RC();
}

}  // namespace

extern "C" int64_t vg_diffaug_ws_floats(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || (int64_t)H * W >= (1ll << 30)) return VG_EINVAL;
    return (int64_t)N * da_parts(H, W);
}

extern "C" int vg_diffaug_params(const uint64_t* rng, int B, int policy, int H, int W, float* out, void* stream) {
    VG_CHECK_ARG(rng && out && B >= 1 && H >= 1 && W >= 1 && H < (1 << 24) && W < (1 << 24), VG_EINVAL);
    VG_CHECK_ARG(policy >= 0 && policy < 32, VG_EINVAL);
    // floor(size / 8 + 0.5) and floor(size / 2 + 0.5) in integer arithmetic
    const int sh_h = (H + 4) / 8, sh_w = (W + 4) / 8, cut_h = (H + 1) / 2, cut_w = (W + 1) / 2;
    hipLaunchKernelGGL(diffaug_params_kernel, dim3((B + 255) / 256), dim3(256), 0, vg_stream(stream),
                       (const unsigned long long*)rng, B, policy, H, W, sh_h, sh_w, cut_h, cut_w, out);
    return VG_LAUNCH_RC();
}

extern "C" int vg_diffaug_forward(const void* in, void* out, const float* params, int N, int PB, int H, int W, int C, int CP,
                                  int cut_h, int cut_w, float* ws, int64_t ws_capacity, int dtype, void* stream) {
    return da_launch<false>(in, out, params, N, PB, H, W, C, CP, cut_h, cut_w, ws, ws_capacity, dtype, stream);
}

extern "C" int vg_diffaug_backward(const void* in, void* out, const float* params, int N, int PB, int H, int W, int C, int CP,
                                   int cut_h, int cut_w, float* ws, int64_t ws_capacity, int dtype, void* stream) {
    return da_launch<true>(in, out, params, N, PB, H, W, C, CP, cut_h, cut_w, ws, ws_capacity, dtype, stream);
}
