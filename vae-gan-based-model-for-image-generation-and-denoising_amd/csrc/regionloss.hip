// Region-weighted reconstruction MSE for training on degraded (occluded) pairs: the squared error of a reconstruction
// against the clean image, split into the image's occlusion rectangle ("hole") and the rest ("valid"), the hole weighed by
// w_hole; its gradient; and the region sums an evaluation pass accumulates.  One streaming pass reads a and b once and
// writes d_a once (12 B per element with the gradient, 8 B without): HBM-bound, 16-byte vectors along W, a grid sized to
// the machine, not to n.
//
//   d = a - b (f32), q = d d (f32); S_hole, S_valid = f64 sums of q over the two regions; n = B C H W
//   loss[0]     = (float)((S_valid + (double)w_hole S_hole) / n)
//   hole_mse[0] = (float)(S_hole / n_hole)            (0 when n_hole == 0)
//   d_a[e]      = d * (hole ? (float)(2 gscale w_hole / n) : (float)(2 gscale / n))
//   stats[0..3] += {S_hole, S_valid, n_hole, n_valid}
//
// Pixel (h, w) of image i is in the hole iff y <= h < y + rect_h and x <= w < x + rect_w with {rect_h, rect_w, x, y} =
// rects[i][2..5] (the layout vg_degrade_params writes), compared as f32.  The rectangle enters comparisons only: no address
// is formed from it.  A NaN makes every comparison false (no hole); a rectangle past the image is clipped by the image.
//
// Summation order is fixed by the shape alone (per-thread grid-stride order in f64 -> wave -> workgroup -> three f64
// partials per workgroup -> one wave sums the partials in f64): the same bits run to run and eager vs. replay.  No atomics,
// no host synchronisation: both launches are capturable.
#include "common.hpp"

namespace {

// 256 CUs x 4 resident 256-thread workgroups, as the MSE launch (pointwise.hip)
constexpr int REGION_MAX_BLOCKS = 1024;

struct Rect {              // half-open f32 bounds; row_lo > row_hi etc. are simply empty
    float y0, y1, x0, x1;
};

__device__ __forceinline__ Rect load_rect(const float* __restrict__ rects, int64_t img) {
    Rect r;
    const float2* p = reinterpret_cast<const float2*>(rects + img * 8);     // rows of 32 bytes: entries 2..5 as two 8-byte loads
    const float2 hw = p[1], xy = p[2];                                       // {rect_h, rect_w}, {x, y}
    r.y0 = xy.y; r.y1 = xy.y + hw.x; r.x0 = xy.x; r.x1 = xy.x + hw.y;
    return r;
}

// n / d for a divisor fixed at launch.  The GPU has no integer divider (a 32-bit division is some tens of instructions, and
// a step needs three: the row of the vector, the image of the row, h of the row): for 32-bit indices the quotient comes from
// one multiply-high and two shifts with constants made on the host (Granlund & Montgomery, "Division by invariant integers
// using multiplication", round-up form: exact for every 32-bit n and every d >= 1); 64-bit indices divide.
template <typename IDX> struct Div;
template <> struct Div<uint32_t> {
    uint32_t d, m, s1, s2;
    explicit Div(uint64_t div) : d((uint32_t)div) {
        uint32_t l = 0;
        while (l < 32 && ((uint64_t)1 << l) < div) ++l;                      // ceil(log2 d)
        m = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << l) - div)) / div + 1);
        s1 = l < 1 ? l : 1;
        s2 = l < 1 ? 0 : l - 1;
    }
    __device__ __forceinline__ uint32_t operator()(uint32_t n) const {
        const uint32_t t = __umulhi(m, n);
        return (t + ((n - t) >> s1)) >> s2;
    }
};
template <> struct Div<uint64_t> {
    uint64_t d;
    explicit Div(uint64_t div) : d(div) {}
    __device__ __forceinline__ uint64_t operator()(uint64_t n) const { return n / d; }
};

// VEC: one 16-byte vector of a row per step (W % 4 == 0, pointers 16-byte aligned); else one element per step.
// IDX: uint32_t where every index fits (the divisions that find the row are then multiply-shifts, Div), else uint64_t.
template <bool VEC, typename IDX>
__global__ __launch_bounds__(256) void region_mse_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const float* __restrict__ rects, IDX nsteps,
                                                                 Div<IDX> by_steps_per_row, Div<IDX> by_H, Div<IDX> by_CH,
                                                                 float coef_valid, float coef_hole,
                                                                 float* __restrict__ d_a, double* __restrict__ ws) {
    constexpr int N = VEC ? 4 : 1;
    __shared__ double red[3][4];
    double s_hole = 0.0, s_valid = 0.0;
    uint32_t c_hole = 0;               // at most 4 per step of a grid-stride loop: far below 2^32
    const IDX stride = (IDX)gridDim.x * (IDX)blockDim.x;
    for (IDX v = (IDX)blockIdx.x * (IDX)blockDim.x + (IDX)threadIdx.x; v < nsteps; v += stride) {
        const IDX row = by_steps_per_row(v);            // (image, channel, h): the row test is one per step
        const IDX w0 = (v - row * by_steps_per_row.d) * (IDX)N;
        bool in_row = false;
        Rect r = {0.f, 0.f, 0.f, 0.f};
        if (rects) {
            r = load_rect(rects, (int64_t)by_CH(row));
            const float hf = (float)(row - by_H(row) * by_H.d);
            in_row = hf >= r.y0 && hf < r.y1;
        }
        float x[N], y[N];
        if constexpr (VEC) {
            const float4 xa = reinterpret_cast<const float4*>(a)[v];
            const float4 yb = reinterpret_cast<const float4*>(b)[v];
            x[0] = xa.x; x[1] = xa.y; x[2] = xa.z; x[3] = xa.w;
            y[0] = yb.x; y[1] = yb.y; y[2] = yb.z; y[3] = yb.w;
        } else {
            x[0] = a[v]; y[0] = b[v];
        }
        float g[N];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float wf = (float)(w0 + (IDX)k);
            const bool hole = in_row && wf >= r.x0 && wf < r.x1;
            const float d = x[k] - y[k];
            const double q = (double)(d * d);
            s_hole += hole ? q : 0.0;
            s_valid += hole ? 0.0 : q;
            c_hole += hole ? 1u : 0u;
            g[k] = d * (hole ? coef_hole : coef_valid);
        }
        if (d_a) {
            if constexpr (VEC) reinterpret_cast<float4*>(d_a)[v] = make_float4(g[0], g[1], g[2], g[3]);
            else d_a[v] = g[0];
        }
    }
    s_hole = wave_sum_d(s_hole);
    s_valid = wave_sum_d(s_valid);
    const double n_hole = wave_sum_d((double)c_hole);   // exact: integers far below 2^53
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s_hole;
        red[1][threadIdx.x >> 6] = s_valid;
        red[2][threadIdx.x >> 6] = n_hole;
    }
    __syncthreads();
    if (threadIdx.x < 3)
        ws[(size_t)blockIdx.x * 3 + threadIdx.x] = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
}

__global__ __launch_bounds__(64) void region_mse_final_kernel(const double* __restrict__ ws, int nparts, double n, double w_hole,
                                                              float* __restrict__ loss, float* __restrict__ hole_mse,
                                                              double* __restrict__ stats) {
    double s_hole = 0.0, s_valid = 0.0, n_hole = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) {
        s_hole += ws[(size_t)i * 3];
        s_valid += ws[(size_t)i * 3 + 1];
        n_hole += ws[(size_t)i * 3 + 2];
    }
    s_hole = wave_sum_d(s_hole);
    s_valid = wave_sum_d(s_valid);
    n_hole = wave_sum_d(n_hole);
    if (threadIdx.x == 0) {
        if (loss) loss[0] = (float)((s_valid + w_hole * s_hole) / n);
        if (hole_mse) hole_mse[0] = n_hole > 0.0 ? (float)(s_hole / n_hole) : 0.f;
        if (stats) {
            stats[0] += s_hole;
            stats[1] += s_valid;
            stats[2] += n_hole;
            stats[3] += n - n_hole;
        }
    }
}

inline int region_blocks(int64_t nsteps) {
    int64_t b = (nsteps + 255) / 256;
    if (b > REGION_MAX_BLOCKS) b = REGION_MAX_BLOCKS;
    if (b < 1) b = 1;
    return (int)b;
}

inline bool region_sizes_ok(int B, int C, int H, int W) { return B >= 1 && C >= 1 && H >= 1 && W >= 1; }

}  // namespace

extern "C" int vg_region_mse_ws_doubles(int B, int C, int H, int W) {
    if (!region_sizes_ok(B, C, H, W)) return VG_EINVAL;
    const int64_t n = (int64_t)B * C * H * W;
    // sized for the scalar path's grid (one element per lane), which is never smaller than the vector path's: the pointers'
    // alignment selects the path at launch
    return 3 * region_blocks(n);
}

extern "C" int vg_region_mse_forward_backward(const float* a, const float* b, const float* rects, int B, int C, int H, int W,
                                              float w_hole, float gscale, float* loss, float* hole_mse, float* d_a,
                                              double* stats, double* ws, int ws_doubles, void* stream) {
    VG_CHECK_ARG(a && b && region_sizes_ok(B, C, H, W), VG_EINVAL);
    VG_CHECK_ARG(__builtin_isfinite(w_hole) && w_hole >= 0.f, VG_EINVAL);
    VG_CHECK_ARG(loss || hole_mse || d_a || stats, VG_EINVAL);
    VG_CHECK_ARG((reinterpret_cast<uintptr_t>(rects) & 7u) == 0, VG_EALIGN);      // its rows are read as 8-byte pairs
    const int64_t n = (int64_t)B * C * H * W;
    const bool vec = (W % 4 == 0) && vg_aligned16(a) && vg_aligned16(b) && (d_a == nullptr || vg_aligned16(d_a));
    const int64_t nsteps = vec ? n / 4 : n;
    const int64_t per_row = vec ? W / 4 : W;
    const int blocks = region_blocks(nsteps);
    VG_CHECK_ARG(ws && ws_doubles >= vg_region_mse_ws_doubles(B, C, H, W), VG_EINVAL);   // >= 3 * blocks on either path
    const float coef_valid = (float)(2.0 * (double)gscale / (double)n);
    const float coef_hole = (float)(2.0 * (double)gscale * (double)w_hole / (double)n);
    const int64_t CH = (int64_t)C * H;
    // 32-bit indices while a grid-stride step past the end cannot wrap: nsteps + one whole grid < 2^32
    const bool idx32 = nsteps + (int64_t)REGION_MAX_BLOCKS * 256 < ((int64_t)1 << 32);
    hipStream_t s = vg_stream(stream);
#define REGION_LAUNCH(VEC, IDX)                                                                                              \
    hipLaunchKernelGGL((region_mse_partial_kernel<VEC, IDX>), dim3(blocks), dim3(256), 0, s, a, b, rects, (IDX)nsteps,        \
                       Div<IDX>((uint64_t)per_row), Div<IDX>((uint64_t)H), Div<IDX>((uint64_t)CH), coef_valid, coef_hole, d_a, ws)
    if (vec && idx32) REGION_LAUNCH(true, uint32_t);
    else if (vec) REGION_LAUNCH(true, uint64_t);
    else if (idx32) REGION_LAUNCH(false, uint32_t);
    else REGION_LAUNCH(false, uint64_t);
#undef REGION_LAUNCH
    int rc = VG_LAUNCH_RC();
    if (rc) return rc;
    if (!(loss || hole_mse || stats)) return 0;        // gradient only: the partial sums are not needed
    hipLaunchKernelGGL(region_mse_final_kernel, dim3(1), dim3(64), 0, s, ws, blocks, (double)n, (double)w_hole, loss, hole_mse,
                       stats);
    return VG_LAUNCH_RC();
}
