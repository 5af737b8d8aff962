// Weight averaging: the exponential moving average of up to VG_EMA_MAX flat f32 parameter buffers in one launch
// (include/vaegan_hip.h "Weight averaging").  A pure stream: per element 4 bytes of p and 4 of ema are read and 4 of ema
// written, 16 bytes per lane and instruction, the grid capped at 2048 workgroups per buffer with a grid-stride loop.
#include <cmath>
#include "common.hpp"

namespace {

struct EmaArgs {
    float* ema[VG_EMA_MAX];
    const float* p[VG_EMA_MAX];
    const float* state[VG_EMA_MAX];
    int64_t n[VG_EMA_MAX];
    double decay[VG_EMA_MAX];
    int warmup[VG_EMA_MAX];
    int nb_end[VG_EMA_MAX];               // buffer i owns the workgroups [nb_end[i - 1], nb_end[i])
};

// e + w (p - e) as three rounded f32 operations.  Contraction off (the pragma binds lexically, see adam_grad in
// pack_adam.hip): hipcc would otherwise fold the product into an fma with the addition.
__device__ __forceinline__ float ema_lerp(float e, float p, float w) {
#pragma clang fp contract(off)
    const float d = p - e;
    const float s = w * d;
    return e + s;
}

__global__ __launch_bounds__(256) void ema_kernel(const EmaArgs a) {
    // owner of this workgroup: at most three scalar compares
    int which = 0;
#pragma unroll
    for (int i = 0; i < VG_EMA_MAX - 1; ++i) which += ((int)blockIdx.x >= a.nb_end[i]) ? 1 : 0;
    const int first = which == 0 ? 0 : a.nb_end[which - 1];
    const int bid = (int)blockIdx.x - first;
    const int nb = a.nb_end[which] - first;
    float* __restrict__ ema = a.ema[which];
    const float* __restrict__ p = a.p[which];
    double d = a.decay[which];
    if (a.warmup[which]) {
        const double t = (double)a.state[which][0];
        d = fmin(d, (1.0 + t) / (10.0 + t));
    }
    const float w = 1.0f - (float)d;
    const int64_t n = a.n[which], n4 = n / 4;
    for (int64_t i = (int64_t)bid * blockDim.x + threadIdx.x; i < n4; i += (int64_t)nb * blockDim.x) {
        float4 ee = reinterpret_cast<float4*>(ema)[i];
        const float4 pp = reinterpret_cast<const float4*>(p)[i];
        ee.x = ema_lerp(ee.x, pp.x, w);
        ee.y = ema_lerp(ee.y, pp.y, w);
        ee.z = ema_lerp(ee.z, pp.z, w);
        ee.w = ema_lerp(ee.w, pp.w, w);
        reinterpret_cast<float4*>(ema)[i] = ee;
    }
    // tail (n not a multiple of 4)
    if (bid == 0) {
        for (int64_t i = n4 * 4 + threadIdx.x; i < n; i += blockDim.x) ema[i] = ema_lerp(ema[i], p[i], w);
    }
}

}  // namespace

extern "C" int vg_ema_update(float* const* ema, const float* const* p, const int64_t* n, const float* const* state,
                             const double* decay, const int* warmup, int count, void* stream) {
    VG_CHECK_ARG(count >= 1 && count <= VG_EMA_MAX, VG_EINVAL);
    VG_CHECK_ARG(ema && p && n && state && decay && warmup, VG_EINVAL);
    EmaArgs a{};
    int end = 0;
    for (int i = 0; i < count; ++i) {
        VG_CHECK_ARG(ema[i] && p[i] && n[i] > 0, VG_EINVAL);
        VG_CHECK_ARG(std::isfinite(decay[i]) && decay[i] >= 0.0 && decay[i] <= 1.0, VG_EINVAL);
        VG_CHECK_ARG(warmup[i] == 0 || state[i] != nullptr, VG_EINVAL);
        VG_CHECK_ARG(n[i] <= (int64_t)(UINTPTR_MAX / 4), VG_EINVAL);
        const uintptr_t e0 = reinterpret_cast<uintptr_t>(ema[i]), p0 = reinterpret_cast<uintptr_t>(p[i]);
        const uintptr_t bytes = (uintptr_t)n[i] * 4u;
        VG_CHECK_ARG(!(e0 < p0 + bytes && p0 < e0 + bytes), VG_EINVAL);         // the two ranges are disjoint
        a.ema[i] = ema[i]; a.p[i] = p[i]; a.state[i] = state[i]; a.n[i] = n[i]; a.decay[i] = decay[i];
        a.warmup[i] = warmup[i] != 0;
        const int64_t b = (n[i] / 4 + 255) / 256;
        end += (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));        // adam_launch's grid: same elements per thread
        a.nb_end[i] = end;
    }
    for (int i = count; i < VG_EMA_MAX; ++i) a.nb_end[i] = 0x7fffffff;      // never the owner of a workgroup
    for (int i = 0; i < count; ++i) VG_CHECK_ARG(vg_aligned16(ema[i]) && vg_aligned16(p[i]), VG_EALIGN);
    hipLaunchKernelGGL(ema_kernel, dim3(end), dim3(256), 0, vg_stream(stream), a);
    return VG_LAUNCH_RC();
}
