// Discriminator-feature reconstruction loss (Larsen et al., "Autoencoding beyond pixels", eq. 2 / Dis_l): the squared
// error between two activations of one Discriminator stage, and its gradient ADDED onto the gradient that already
// arrives at that activation from the layers above.  One streaming pass reads a, b and d once and writes d once; no
// 2 (a - b) / n tensor is ever materialised.  HBM-bound: 16-byte vectors, a grid sized to the machine, not to n.
//
//   loss[0] (+)= (1 / n) sum_i (a_i - b_i)^2
//   d[i]      = round_dtype( float(d[i]) + f32(gscale 2 / n) (a_i - b_i) )          (d == NULL: loss only)
//
// Summation order is fixed by n alone (per-thread grid-stride order in f64 -> wave -> workgroup -> one f32 partial per
// workgroup -> one wave sums the partials in f64), so the loss has the same bits run to run and eager vs. replay.  No atomics,
// no host synchronisation: both launches are capturable.
#include "common.hpp"

namespace {

// 256 CUs x 4 resident 256-thread workgroups; also the workspace the Python side keeps for the partial sums
constexpr int FEAT_MAX_BLOCKS = 1024;

template <int DT> struct Vec16;
template <> struct Vec16<VG_F32> {
    static constexpr int N = 4;
    __device__ static __forceinline__ void load(const void* p, int64_t v, float* o) {
        const float4 r = reinterpret_cast<const float4*>(p)[v];
        o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
    }
    __device__ static __forceinline__ void store(void* p, int64_t v, const float* o) {
        reinterpret_cast<float4*>(p)[v] = make_float4(o[0], o[1], o[2], o[3]);
    }
};
template <> struct Vec16<VG_BF16> {
    static constexpr int N = 8;
    __device__ static __forceinline__ void load(const void* p, int64_t v, float* o) {
        const uint4 r = reinterpret_cast<const uint4*>(p)[v];
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o[2 * k] = __uint_as_float(w[k] << 16);
            o[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
        }
    }
    __device__ static __forceinline__ void store(void* p, int64_t v, const float* o) {
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            w[k] = (uint32_t)ElemT<VG_BF16>::from_f32(o[2 * k]) | ((uint32_t)ElemT<VG_BF16>::from_f32(o[2 * k + 1]) << 16);
        reinterpret_cast<uint4*>(p)[v] = make_uint4(w[0], w[1], w[2], w[3]);
    }
};

template <int DT>
__global__ __launch_bounds__(256) void feat_mse_partial_kernel(const void* __restrict__ a, const void* __restrict__ b,
                                                               void* __restrict__ d, int64_t n, float gcoef,
                                                               float* __restrict__ ws) {
    constexpr int N = Vec16<DT>::N;
    __shared__ double red[4];
    double s = 0.0;
    const int64_t nv = n / N;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x) {
        float x[N], y[N];
        Vec16<DT>::load(a, v, x);
        Vec16<DT>::load(b, v, y);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            x[k] -= y[k];
            s += (double)(x[k] * x[k]);
        }
        if (d) {
            Vec16<DT>::load(d, v, y);
#pragma unroll
            for (int k = 0; k < N; ++k) y[k] = fmaf(gcoef, x[k], y[k]);
            Vec16<DT>::store(d, v, y);
        }
    }
    if (blockIdx.x == 0) {                      // n is no multiple of a 16-byte vector: the last few elements, one by one
        for (int64_t i = nv * N + threadIdx.x; i < n; i += blockDim.x) {
            const float df = load1<DT>(a, i) - load1<DT>(b, i);
            s += (double)(df * df);
            if (d) store1<DT>(d, i, fmaf(gcoef, df, load1<DT>(d, i)));
        }
    }
    s = wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) ws[blockIdx.x] = (float)(red[0] + red[1] + red[2] + red[3]);
}

__global__ __launch_bounds__(64) void feat_mse_final_kernel(const float* __restrict__ ws, int nparts, double n,
                                                            float* __restrict__ loss, int accumulate) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) s += (double)ws[i];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) {
        const float v = (float)(s / n);
        loss[0] = accumulate ? loss[0] + v : v;
    }
}

}  // namespace

extern "C" int vg_feat_mse_forward_backward(const void* f_fake, const void* f_real, void* d_inout, int64_t n, float gscale,
                                            float* loss, int accumulate_loss, float* ws, int ws_capacity, int dtype,
                                            void* stream) {
    VG_CHECK_ARG(dtype == VG_F32 || dtype == VG_BF16, VG_ENOSUP);
    VG_CHECK_ARG(f_fake && f_real && loss && ws && n > 0 && ws_capacity >= 1, VG_EINVAL);
    VG_CHECK_ARG(vg_aligned16(f_fake) && vg_aligned16(f_real) && (d_inout == nullptr || vg_aligned16(d_inout)), VG_EALIGN);
    const int64_t nv = n / (dtype == VG_F32 ? 4 : 8);
    int64_t blocks = (nv + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > FEAT_MAX_BLOCKS) blocks = FEAT_MAX_BLOCKS;
    if (blocks > ws_capacity) blocks = ws_capacity;
    const float gcoef = (float)((double)gscale * 2.0 / (double)n);
    if (dtype == VG_F32)
        hipLaunchKernelGGL(feat_mse_partial_kernel<VG_F32>, dim3((int)blocks), dim3(256), 0, vg_stream(stream), f_fake, f_real,
                           d_inout, n, gcoef, ws);
    else
        hipLaunchKernelGGL(feat_mse_partial_kernel<VG_BF16>, dim3((int)blocks), dim3(256), 0, vg_stream(stream), f_fake, f_real,
                           d_inout, n, gcoef, ws);
    int rc = VG_LAUNCH_RC();
    if (rc) return rc;
    hipLaunchKernelGGL(feat_mse_final_kernel, dim3(1), dim3(64), 0, vg_stream(stream), ws, (int)blocks, (double)n, loss,
                       accumulate_loss);
    return VG_LAUNCH_RC();
}
