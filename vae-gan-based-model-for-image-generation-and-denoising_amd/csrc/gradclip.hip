// Gradient-norm clipping (include/vaegan_hip.h "Gradient-norm clipping"): the global L2 norm of up to VG_GNORM_MAX flat f32
// gradient buffers and torch's clip coefficient for each, left ON THE DEVICE for vg_adam_apply_clip (pack_adam.hip).  Two
// launches: f64 partial sums per workgroup (a pure 4 B/element read stream), then one workgroup per buffer that adds the
// partials in a fixed order and evaluates the coefficient.  The kernel boundary is the hand-off: no atomics, no fences.
#include <cmath>
#include "common.hpp"

namespace {

constexpr int GN_THREADS = 256;
constexpr int GN_LOADS = 4;                                   // independent 16-byte loads in flight per thread and sweep
constexpr int GN_SWEEP = GN_THREADS * GN_LOADS;               // float4 per workgroup and sweep (1024)
static_assert(VG_GNORM_PARTS % GN_THREADS == 0, "the finalize walks the partials in rounds of one workgroup");

struct GnormArgs {
    const float* g[VG_GNORM_MAX];
    int64_t n[VG_GNORM_MAX];
    int nb_end[VG_GNORM_MAX];             // buffer i owns the workgroups [nb_end[i - 1], nb_end[i])
    double* ws;
};

struct GnormFinalArgs {
    float* out[VG_GNORM_MAX];
    double max_norm[VG_GNORM_MAX];
    float gscale[VG_GNORM_MAX];
    int nb[VG_GNORM_MAX];
    const double* ws;
};

__device__ __forceinline__ double gn_sq4(double acc, const float4 v) {
    acc += (double)v.x * (double)v.x;     // every product of two f32 is exact in f64
    acc += (double)v.y * (double)v.y;
    acc += (double)v.z * (double)v.z;
    acc += (double)v.w * (double)v.w;
    return acc;
}

// Sum of one value per thread over the workgroup, in a fixed order: xor butterfly inside each wave, then the four waves'
// sums through LDS added in wave order.  Valid in thread 0.
__device__ __forceinline__ double gn_block_sum(double v) {
    __shared__ double part[GN_THREADS / 64];
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = part[0];
#pragma unroll
    for (int w = 1; w < GN_THREADS / 64; ++w) s += part[w];
    return s;
}

__global__ __launch_bounds__(GN_THREADS) void gnorm_partial_kernel(const GnormArgs a) {
    int which = 0;
#pragma unroll
    for (int i = 0; i < VG_GNORM_MAX - 1; ++i) which += ((int)blockIdx.x >= a.nb_end[i]) ? 1 : 0;
    const int first = which == 0 ? 0 : a.nb_end[which - 1];
    const int bid = (int)blockIdx.x - first;
    const int nb = a.nb_end[which] - first;
    const float* __restrict__ g = a.g[which];
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    const int64_t n = a.n[which], n4 = n / 4;
    const int64_t full = n4 / GN_SWEEP;                       // sweeps in which every thread has all of its loads
    double acc[GN_LOADS] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t s = bid; s < full; s += nb) {
        const int64_t base = s * GN_SWEEP + threadIdx.x;
        float4 v[GN_LOADS];
#pragma unroll
        for (int k = 0; k < GN_LOADS; ++k) v[k] = g4[base + k * GN_THREADS];        // four loads issued, then consumed
#pragma unroll
        for (int k = 0; k < GN_LOADS; ++k) acc[k] = gn_sq4(acc[k], v[k]);
    }
    // the last, partial sweep belongs to the workgroup whose turn it is
    if (full * GN_SWEEP < n4 && (int)(full % nb) == bid) {
        const int64_t base = full * GN_SWEEP + threadIdx.x;
        float4 v[GN_LOADS];
#pragma unroll
        for (int k = 0; k < GN_LOADS; ++k) {
            const int64_t idx = base + k * GN_THREADS;
            v[k] = idx < n4 ? g4[idx] : float4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int k = 0; k < GN_LOADS; ++k) acc[k] = gn_sq4(acc[k], v[k]);
    }
    // tail (n not a multiple of 4), element by element in the buffer's first workgroup
    if (bid == 0) {
        const int64_t i = n4 * 4 + threadIdx.x;
        if (i < n) acc[0] += (double)g[i] * (double)g[i];
    }
    const double s = gn_block_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if (threadIdx.x == 0) a.ws[which * VG_GNORM_PARTS + bid] = s;
}

__global__ __launch_bounds__(GN_THREADS) void gnorm_final_kernel(const GnormFinalArgs a) {
    const int i = blockIdx.x;
    const double* __restrict__ part = a.ws + i * VG_GNORM_PARTS;
    const int nb = a.nb[i];
    double v = 0.0;
#pragma unroll
    for (int r = 0; r < VG_GNORM_PARTS / GN_THREADS; ++r) {
        const int b = r * GN_THREADS + (int)threadIdx.x;
        if (b < nb) v += part[b];
    }
    const double S = gn_block_sum(v);
    if (threadIdx.x == 0) {
        const double norm = fabs((double)a.gscale[i]) * sqrt(S);
        const double c = a.max_norm[i] / (norm + 1e-6);
        a.out[i][0] = (float)norm;
        a.out[i][1] = (float)(c < 1.0 ? c : (c != c ? c : 1.0));   // torch.clamp(max=1): NaN stays NaN
    }
}

}  // namespace

extern "C" int vg_grad_norm_clip(const float* const* g, const int64_t* n, const float* grad_scale, const double* max_norm,
                                 int count, float* const* out, double* ws, void* stream) {
    VG_CHECK_ARG(count >= 1 && count <= VG_GNORM_MAX, VG_EINVAL);
    VG_CHECK_ARG(g && n && grad_scale && max_norm && out && ws, VG_EINVAL);
    GnormArgs a{};
    GnormFinalArgs f{};
    int end = 0;
    for (int i = 0; i < count; ++i) {
        VG_CHECK_ARG(g[i] && out[i] && n[i] > 0, VG_EINVAL);
        VG_CHECK_ARG(!(max_norm[i] != max_norm[i]) && max_norm[i] >= 0.0, VG_EINVAL);      // +inf: norm monitor
        VG_CHECK_ARG(std::isfinite(grad_scale[i]), VG_EINVAL);
        const int64_t b = (n[i] / 4 + GN_SWEEP - 1) / GN_SWEEP;
        const int nb = (int)(b < 1 ? 1 : (b > VG_GNORM_PARTS ? VG_GNORM_PARTS : b));
        end += nb;
        a.g[i] = g[i]; a.n[i] = n[i]; a.nb_end[i] = end;
        f.out[i] = out[i]; f.max_norm[i] = max_norm[i]; f.gscale[i] = grad_scale[i]; f.nb[i] = nb;
    }
    for (int i = count; i < VG_GNORM_MAX; ++i) a.nb_end[i] = 0x7fffffff;    // never the owner of a workgroup
    for (int i = 0; i < count; ++i) VG_CHECK_ARG(vg_aligned16(g[i]), VG_EALIGN);
    a.ws = ws;
    f.ws = ws;
    hipStream_t s = vg_stream(stream);
    hipLaunchKernelGGL(gnorm_partial_kernel, dim3(end), dim3(GN_THREADS), 0, s, a);
    int rc = VG_LAUNCH_RC();
    if (rc) return rc;
    hipLaunchKernelGGL(gnorm_final_kernel, dim3(count), dim3(GN_THREADS), 0, s, f);
    return VG_LAUNCH_RC();
}
