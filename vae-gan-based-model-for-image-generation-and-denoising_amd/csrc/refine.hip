// Test-time latent refinement (GAN-inversion denoising / inpainting; Yeh et al. 2017): the three kernels that the frozen
// networks' forward and data-gradient chains lack when the unknown is the latent z, not a weight.  Contracts in
// include/vaegan_hip.h.
//
//   vg_bn_act_backward_eval   backward of y = act(scale[c] x + shift[c]) with CONSTANT coefficients (eval-mode BatchNorm):
//                             dx = dy act'(z) scale[c].  No statistics, no reduction: one streaming pass, three tensor-sized
//                             streams (12 B per element f32, 6 B bf16), HBM-bound.
//   vg_masked_mse_rows        per-image mean squared error outside the image's occlusion rectangle and its gradient: two
//                             reads and one write of an NCHW f32 image batch (12 B per element), HBM-bound; f64 partials per
//                             workgroup, a workgroup never leaves its image.
//   vg_latent_adam            objective, keep-best and Adam over the latent rows: one wave per row, everything a row needs in
//                             that wave (the step count too), a few hundred bytes per row: launch-latency-bound.
//
// No atomics, no host synchronisation, no allocation: every launch is capturable and gives the same bits eagerly and replayed.
#include "common.hpp"

namespace {

// ---- (a) eval-mode BatchNorm + activation backward -------------------------------------------------------------------
// The thread -> (row slot, channel column) mapping of bn_act.hip's streaming passes: min(C / VW, 256) threads per row,
// 256 / that rows per pass, blockIdx.y the block of 256 columns (the last one may be ragged); the two coefficient vectors
// are loaded once, before the row loop; four rows (4 x 16 bytes per tensor) in flight per thread.
constexpr int EV_UNROLL = 4;
constexpr int EV_MAX_WGS = 1024;     // 4 resident 256-thread workgroups on each of the 256 CUs (two coefficient vectors only)

template <int DT, int VW> struct RawVec { typedef __attribute__((ext_vector_type(VW / 2))) uint32_t type; };
template <int VW> struct RawVec<VG_F32, VW> { typedef float4 type; };
template <int DT, int VW>
__device__ __forceinline__ typename RawVec<DT, VW>::type loadv(const void* base, int64_t idx) {
    typedef typename RawVec<DT, VW>::type W;
    return *reinterpret_cast<const W*>(reinterpret_cast<const typename ElemT<DT>::type*>(base) + idx);
}
template <int DT, int VW>
__device__ __forceinline__ void unpackv(const typename RawVec<DT, VW>::type& r, float (&v)[VW]) {
    if constexpr (DT == VG_F32) {
        static_assert(VW == 4, "f32: one 16-byte vector");
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    } else {
#pragma unroll
        for (int k = 0; k < VW / 2; ++k) {
            v[2 * k] = __uint_as_float(r[k] << 16);
            v[2 * k + 1] = __uint_as_float(r[k] & 0xffff0000u);
        }
    }
}
template <int DT, int VW> __device__ __forceinline__ void storev(void* base, int64_t idx, const float (&v)[VW]) {
    typename RawVec<DT, VW>::type r;
    if constexpr (DT == VG_F32) {
        r = float4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int k = 0; k < VW / 2; ++k)
            r[k] = (uint32_t)ElemT<VG_BF16>::from_f32(v[2 * k]) | ((uint32_t)ElemT<VG_BF16>::from_f32(v[2 * k + 1]) << 16);
    }
    *reinterpret_cast<typename RawVec<DT, VW>::type*>(reinterpret_cast<typename ElemT<DT>::type*>(base) + idx) = r;
}
template <int V> struct IntC { static constexpr int value = V; };

template <int VW> __device__ __forceinline__ void load_coef(const float* __restrict__ p, float (&c)[VW]) {
#pragma unroll
    for (int k = 0; k < VW; k += 4) {
        const float4 r = *reinterpret_cast<const float4*>(p + k);
        c[k] = r.x; c[k + 1] = r.y; c[k + 2] = r.z; c[k + 3] = r.w;
    }
}

struct EvalPlan { int vec, rows_per_block, blocks, col_blocks; };

inline EvalPlan eval_plan(int dtype, int64_t rows, int C, bool aligned16) {
    EvalPlan p;
    p.vec = (dtype == VG_BF16 && C % 8 == 0 && aligned16) ? 8 : 4;
    const int cols = C / p.vec;
    const int ncol = cols < 256 ? cols : 256;
    const int rpp = 256 / ncol;
    p.col_blocks = (cols + 255) / 256;
    const int64_t passes = (rows + rpp - 1) / rpp;
    int64_t cap = EV_MAX_WGS / p.col_blocks;
    if (cap < 1) cap = 1;
    const int64_t blocks = passes < cap ? passes : cap;
    const int64_t rpb = (passes + blocks - 1) / blocks * rpp;
    p.rows_per_block = (int)rpb;
    p.blocks = (int)((rows + rpb - 1) / rpb);
    return p;
}

template <int DT, int VW>
__global__ __launch_bounds__(256) void bn_act_bwd_eval_kernel(const void* __restrict__ x, const void* __restrict__ dy,
                                                              void* __restrict__ dx, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, int64_t rows, int C, int act,
                                                              float slope, int rows_per_block) {
    typedef typename RawVec<DT, VW>::type Raw;
    const int cols = C / VW;
    const int cb = blockIdx.y * 256;
    const int ncol = min(256, cols - cb);
    const int rpp = 256 / ncol;
    const int tr = threadIdx.x / ncol, tc = threadIdx.x - tr * ncol;
    const int c = (cb + tc) * VW;                       // tc < ncol: c + VW <= C for every thread, idle ones included
    const int64_t b0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(rows, b0 + (int64_t)rows_per_block);
    int64_t r = tr < rpp ? b0 + tr : r1;                // an idle thread gets an empty range
    const int64_t step = (int64_t)rpp * C;
    int64_t off = r * C + c;
    float sc[VW], sh[VW];
    load_coef<VW>(scale + c, sc);
    load_coef<VW>(shift + c, sh);
    auto run = [&](auto act_c) {                        // the activation is uniform: chosen once, outside the row loop
        constexpr int ACT = decltype(act_c)::value;
        auto one = [&](int64_t o, const Raw& rx, const Raw& rg) {
            float f[VW], d[VW], q[VW];
            unpackv<DT, VW>(rx, f);
            unpackv<DT, VW>(rg, d);
            // z by vg_bn_act_forward's own expression (one fused multiply-add), so the mask is the forward's bit for bit
#pragma unroll
            for (int k = 0; k < VW; ++k)
                q[k] = act_bwd(__builtin_fmaf(sc[k], f[k], sh[k]), d[k], ACT, slope) * sc[k];
            storev<DT, VW>(dx, o, q);
        };
        for (; r + (EV_UNROLL - 1) * rpp < r1; r += EV_UNROLL * rpp, off += EV_UNROLL * step) {
            Raw v[EV_UNROLL], g[EV_UNROLL];
#pragma unroll
            for (int u = 0; u < EV_UNROLL; ++u) { v[u] = loadv<DT, VW>(x, off + u * step); g[u] = loadv<DT, VW>(dy, off + u * step); }
#pragma unroll
            for (int u = 0; u < EV_UNROLL; ++u) one(off + u * step, v[u], g[u]);
        }
        if (r < r1) {                                   // the last one to three rows of the row block, together as well
            Raw v[EV_UNROLL - 1], g[EV_UNROLL - 1];
#pragma unroll
            for (int u = 0; u < EV_UNROLL - 1; ++u)
                if (r + u * rpp < r1) { v[u] = loadv<DT, VW>(x, off + u * step); g[u] = loadv<DT, VW>(dy, off + u * step); }
#pragma unroll
            for (int u = 0; u < EV_UNROLL - 1; ++u)
                if (r + u * rpp < r1) one(off + u * step, v[u], g[u]);
        }
    };
    if (act == VG_ACT_RELU) run(IntC<VG_ACT_RELU>{});
    else if (act == VG_ACT_LRELU) run(IntC<VG_ACT_LRELU>{});
    else run(IntC<VG_ACT_NONE>{});
}

// ---- (b) per-image masked MSE ----------------------------------------------------------------------------------------
constexpr int MM_MAX_BLOCKS = 2048;     // whole launch: 256 CUs x 8 resident 256-thread workgroups

struct Rect {              // half-open f32 bounds; y0 > y1 etc. are simply empty
    float y0, y1, x0, x1;
};

// the hole rule of vg_region_mse_forward_backward (regionloss.hip), word for word
__device__ __forceinline__ Rect load_rect(const float* __restrict__ rects, int64_t img) {
    Rect r;
    const float2* p = reinterpret_cast<const float2*>(rects + img * 8);     // rows of 32 bytes: entries 2..5 as two 8-byte loads
    const float2 hw = p[1], xy = p[2];                                       // {rect_h, rect_w}, {x, y}
    r.y0 = xy.y; r.y1 = xy.y + hw.x; r.x0 = xy.x; r.x1 = xy.x + hw.y;
    return r;
}

// n / d for a divisor fixed at launch: one multiply-high and two shifts (Granlund & Montgomery, round-up form: exact for
// every 32-bit n and every d >= 1), as regionloss.hip
struct Div32 {
    uint32_t d, m, s1, s2;
    explicit Div32(uint64_t div) : d((uint32_t)div) {
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

// Hole elements of one image = C x (rows h with y0 <= h < y1) x (columns w with x0 <= w < x1): the pixel test is the
// conjunction of a row test and a column test, so the count is their product.  Every thread of the workgroup gets the
// result; `cnt` is 2 x 4 words of LDS.  Integer sums: exact whatever the order.
__device__ __forceinline__ uint32_t hole_count(const Rect& r, bool have, int C, int H, int W, uint32_t (*cnt)[4]) {
    uint32_t nr = 0, nc = 0;
    if (have) {
        for (int h = threadIdx.x; h < H; h += blockDim.x) { const float f = (float)h; nr += (f >= r.y0 && f < r.y1) ? 1u : 0u; }
        for (int w = threadIdx.x; w < W; w += blockDim.x) { const float f = (float)w; nc += (f >= r.x0 && f < r.x1) ? 1u : 0u; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nr += __shfl_xor(nr, o); nc += __shfl_xor(nc, o); }
    const int nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) { cnt[0][threadIdx.x >> 6] = nr; cnt[1][threadIdx.x >> 6] = nc; }
    __syncthreads();
    nr = 0; nc = 0;
    for (int k = 0; k < nw; ++k) { nr += cnt[0][k]; nc += cnt[1][k]; }
    return (uint32_t)C * nr * nc;                       // <= C H W < 2^31 (checked on the host)
}

// grid (blocks per image, B): a workgroup's partial is of ONE image.  VEC: one 16-byte vector of a row per step.
template <bool VEC>
__global__ __launch_bounds__(256) void masked_mse_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                 const float* __restrict__ rects, uint32_t nsteps,
                                                                 Div32 by_steps_per_row, Div32 by_H, int C, int H, int W,
                                                                 double two_gscale, float* __restrict__ d_a,
                                                                 double* __restrict__ ws) {
    constexpr int N = VEC ? 4 : 1;
    __shared__ uint32_t cnt[2][4];
    __shared__ double red[4];
    const int img = blockIdx.y;
    Rect r = {0.f, 0.f, 0.f, 0.f};
    if (rects) r = load_rect(rects, img);
    const uint32_t n_hole = hole_count(r, rects != nullptr, C, H, W, cnt);
    const uint32_t n_valid = (uint32_t)C * (uint32_t)H * (uint32_t)W - n_hole;
    const float coef = n_valid ? (float)(two_gscale / (double)n_valid) : 0.f;
    const size_t base = (size_t)img * nsteps;           // in steps: vectors or elements
    double s_valid = 0.0;
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < nsteps; v += gridDim.x * 256u) {
        const uint32_t row = by_steps_per_row(v);       // (channel, h) of this image
        const uint32_t w0 = (v - row * by_steps_per_row.d) * (uint32_t)N;
        bool in_row = false;
        if (rects) {
            const float hf = (float)(row - by_H(row) * by_H.d);
            in_row = hf >= r.y0 && hf < r.y1;
        }
        float x[N], y[N], g[N];
        if constexpr (VEC) {
            const float4 xa = reinterpret_cast<const float4*>(a)[base + v];
            const float4 yb = reinterpret_cast<const float4*>(b)[base + v];
            x[0] = xa.x; x[1] = xa.y; x[2] = xa.z; x[3] = xa.w;
            y[0] = yb.x; y[1] = yb.y; y[2] = yb.z; y[3] = yb.w;
        } else {
            x[0] = a[base + v]; y[0] = b[base + v];
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const float wf = (float)(w0 + (uint32_t)k);
            const bool hole = in_row && wf >= r.x0 && wf < r.x1;
            const float d = x[k] - y[k];
            s_valid += hole ? 0.0 : (double)(d * d);
            g[k] = hole ? 0.f : d * coef;
        }
        if (d_a) {
            if constexpr (VEC) reinterpret_cast<float4*>(d_a)[base + v] = make_float4(g[0], g[1], g[2], g[3]);
            else d_a[base + v] = g[0];
        }
    }
    s_valid = wave_sum_d(s_valid);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s_valid;
    __syncthreads();
    if (threadIdx.x == 0) ws[(size_t)img * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// one wave per image: its partials in fixed order, the hole count again (same integers), the mean
__global__ __launch_bounds__(64) void masked_mse_final_kernel(const double* __restrict__ ws, int nparts,
                                                              const float* __restrict__ rects, int C, int H, int W,
                                                              float* __restrict__ loss_rows) {
    __shared__ uint32_t cnt[2][4];
    const int img = blockIdx.x;
    Rect r = {0.f, 0.f, 0.f, 0.f};
    if (rects) r = load_rect(rects, img);
    const uint32_t n_hole = hole_count(r, rects != nullptr, C, H, W, cnt);
    const uint32_t n_valid = (uint32_t)C * (uint32_t)H * (uint32_t)W - n_hole;
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) s += ws[(size_t)img * nparts + i];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) loss_rows[img] = n_valid ? (float)(s / (double)n_valid) : 0.f;
}

inline bool mm_sizes_ok(int B, int C, int H, int W) {
    return B >= 1 && B <= 65535 && C >= 1 && H >= 1 && W >= 1 && (int64_t)C * H * W < ((int64_t)1 << 31) - MM_MAX_BLOCKS * 256;
}

inline int mm_blocks(int B, int64_t steps_per_image) {
    int64_t b = (steps_per_image + 255) / 256;
    int64_t cap = MM_MAX_BLOCKS / B;
    if (cap < 1) cap = 1;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// ---- (c) Adam over latent rows ----------------------------------------------------------------------------------------
// One wave per row.  Everything is formed in f64 from the f32 state and rounded ONCE into each stored value, so that an f64
// restatement with the same roundings reproduces it; the only sum (of z^2, for the prior term) runs in the fixed order
// lane-strided partials -> xor-shuffle tree.  beta^(t+1) comes from square-and-multiply in f64 (pow_int), not pow(): a fixed
// sequence of products that a restatement repeats bit for bit, about 2 log2(t) of them.
__device__ __forceinline__ double pow_int(double b, int n) {
    double r = 1.0;
    for (; n > 0; n >>= 1) {
        if (n & 1) r *= b;
        b *= b;
    }
    return r;
}

template <int DT>
__global__ __launch_bounds__(64) void latent_adam_kernel(float* __restrict__ z, float* __restrict__ m, float* __restrict__ v,
                                                         int* __restrict__ t, float* __restrict__ best_loss,
                                                         float* __restrict__ best_z, const void* __restrict__ dz,
                                                         const float* __restrict__ loss_rows, const float* __restrict__ p,
                                                         const void* __restrict__ z_in, void* __restrict__ z_out,
                                                         float* __restrict__ objective, int L, int ZP, double lr,
                                                         double beta1, double beta2, double eps, double alpha_adv,
                                                         double prior_weight, int mode) {
    const int row = blockIdx.x, lane = threadIdx.x;
    const size_t zb = (size_t)row * L, pb = (size_t)row * ZP;
    if (mode == VG_LATENT_INIT) {
        for (int l = lane; l < ZP; l += 64) {
            float f = 0.f;
            if (l < L) {
                f = load1<DT>(z_in, pb + l);
                z[zb + l] = f; m[zb + l] = 0.f; v[zb + l] = 0.f; best_z[zb + l] = f;
            }
            if (z_out) store1<DT>(z_out, pb + l, f);
        }
        if (lane == 0) { t[row] = 0; best_loss[row] = __builtin_inff(); }
        return;
    }
    // 1. the objective at the z that was just evaluated
    double q = 0.0;
    if (prior_weight != 0.0)
        for (int l = lane; l < L; l += 64) { const double zl = (double)z[zb + l]; q += zl * zl; }
    q = wave_sum_d(q);
    double J = (double)loss_rows[row];
    if (p) J += alpha_adv * -fmax(log((double)p[row]), -100.0);
    if (prior_weight != 0.0) J += prior_weight * (q / (2.0 * (double)L));
    const float Jf = (float)J;
    if (objective && lane == 0) objective[row] = Jf;
    // 2. keep-best: strictly lower only, so a tie keeps the earlier iterate and a NaN never wins
    const bool better = Jf < best_loss[row];            // every lane reads the old value before lane 0 may write (one wave)
    if (better) {
        for (int l = lane; l < L; l += 64) best_z[zb + l] = z[zb + l];
        if (lane == 0) best_loss[row] = Jf;
    }
    if (mode != VG_LATENT_UPDATE) return;
    // 3. Adam (torch.optim.Adam, no weight decay, no amsgrad) with the row's own step count
    const int tn = t[row] + 1;
    const double b1t = pow_int(beta1, tn), b2t = pow_int(beta2, tn);
    const double step_size = lr / (1.0 - b1t), bc2_sqrt = sqrt(1.0 - b2t);
    for (int l = lane; l < ZP; l += 64) {
        float f = 0.f;
        if (l < L) {
            const double zl = (double)z[zb + l];
            const double g = (double)load1<DT>(dz, pb + l) + prior_weight * zl / (double)L;
            const float mf = (float)(beta1 * (double)m[zb + l] + (1.0 - beta1) * g);
            const float vf = (float)(beta2 * (double)v[zb + l] + (1.0 - beta2) * g * g);
            f = (float)(zl - step_size * ((double)mf / (sqrt((double)vf) / bc2_sqrt + eps)));
            m[zb + l] = mf; v[zb + l] = vf; z[zb + l] = f;
        }
        // 4. the Generator's next input, padding lanes zero
        store1<DT>(z_out, pb + l, f);
    }
    if (lane == 0) t[row] = tn;
}

}  // namespace

extern "C" int vg_bn_act_backward_eval(const void* x, const void* dy, void* dx, const float* scale, const float* shift,
                                       int64_t rows, int C, int act, float slope, int dtype, void* stream) {
    VG_CHECK_ARG(x && dy && dx && scale && shift && rows > 0 && C > 0, VG_EINVAL);
    VG_CHECK_ARG(act == VG_ACT_NONE || act == VG_ACT_RELU || act == VG_ACT_LRELU, VG_EINVAL);
    VG_CHECK_ARG(rows <= INT64_MAX / C, VG_EINVAL);
    VG_CHECK_ARG(dtype == VG_F32 || dtype == VG_BF16, VG_ENOSUP);
    VG_CHECK_ARG(C % 4 == 0, VG_EALIGN);
    // the narrowest vector of the launch: 16 bytes of f32, 8 bytes of bf16; the coefficient vectors are read as float4
    const uintptr_t amask = dtype == VG_F32 ? 15u : 7u;
    VG_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dx)) & amask) == 0,
                 VG_EALIGN);
    VG_CHECK_ARG(vg_aligned16(scale) && vg_aligned16(shift), VG_EALIGN);
    const EvalPlan p = eval_plan(dtype, rows, C, vg_aligned16(x) && vg_aligned16(dy) && vg_aligned16(dx));
    const dim3 grid(p.blocks, p.col_blocks);
    const hipStream_t s = vg_stream(stream);
    if (dtype == VG_F32)
        vg_launch_timed(4, (bn_act_bwd_eval_kernel<VG_F32, 4>), grid, dim3(256), 0, s, x, dy, dx, scale, shift, rows, C, act, slope,
                        p.rows_per_block);
    else if (p.vec == 8)
        vg_launch_timed(4, (bn_act_bwd_eval_kernel<VG_BF16, 8>), grid, dim3(256), 0, s, x, dy, dx, scale, shift, rows, C, act, slope,
                        p.rows_per_block);
    else
        vg_launch_timed(4, (bn_act_bwd_eval_kernel<VG_BF16, 4>), grid, dim3(256), 0, s, x, dy, dx, scale, shift, rows, C, act, slope,
                        p.rows_per_block);
    return VG_LAUNCH_RC();
}

extern "C" int vg_masked_mse_rows_ws_doubles(int B, int C, int H, int W) {
    if (!mm_sizes_ok(B, C, H, W)) return VG_EINVAL;
    // sized for the scalar path's grid (one element per lane), which is never smaller than the vector path's: the pointers'
    // alignment selects the path at launch
    return B * mm_blocks(B, (int64_t)C * H * W);
}

extern "C" int vg_masked_mse_rows(const float* a, const float* b, const float* rects, int B, int C, int H, int W, float gscale,
                                  float* loss_rows, float* d_a, double* ws, int ws_doubles, void* stream) {
    VG_CHECK_ARG(a && b && mm_sizes_ok(B, C, H, W), VG_EINVAL);
    VG_CHECK_ARG(loss_rows || d_a, VG_EINVAL);
    VG_CHECK_ARG(__builtin_isfinite(gscale), VG_EINVAL);
    VG_CHECK_ARG(ws && ws_doubles >= vg_masked_mse_rows_ws_doubles(B, C, H, W), VG_EINVAL);
    VG_CHECK_ARG((reinterpret_cast<uintptr_t>(rects) & 7u) == 0, VG_EALIGN);      // its rows are read as 8-byte pairs
    VG_CHECK_ARG(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(d_a) |
                   reinterpret_cast<uintptr_t>(loss_rows)) & 3u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, VG_EALIGN);
    const int64_t n_img = (int64_t)C * H * W;
    // an image's first element must be 16-byte aligned as well: W % 4 == 0 makes C H W a multiple of 4
    const bool vec = (W % 4 == 0) && vg_aligned16(a) && vg_aligned16(b) && (d_a == nullptr || vg_aligned16(d_a));
    const int64_t nsteps = vec ? n_img / 4 : n_img;
    const int64_t per_row = vec ? W / 4 : W;
    const int blocks = mm_blocks(B, nsteps);
    const dim3 grid(blocks, B);
    const double two_gscale = 2.0 * (double)gscale;
    hipStream_t s = vg_stream(stream);
    if (vec)
        hipLaunchKernelGGL(masked_mse_partial_kernel<true>, grid, dim3(256), 0, s, a, b, rects, (uint32_t)nsteps,
                           Div32((uint64_t)per_row), Div32((uint64_t)H), C, H, W, two_gscale, d_a, ws);
    else
        hipLaunchKernelGGL(masked_mse_partial_kernel<false>, grid, dim3(256), 0, s, a, b, rects, (uint32_t)nsteps,
                           Div32((uint64_t)per_row), Div32((uint64_t)H), C, H, W, two_gscale, d_a, ws);
    int rc = VG_LAUNCH_RC();
    if (rc || !loss_rows) return rc;                   // gradient only: the partial sums are not needed
    hipLaunchKernelGGL(masked_mse_final_kernel, dim3(B), dim3(64), 0, s, (const double*)ws, blocks, rects, C, H, W, loss_rows);
    return VG_LAUNCH_RC();
}

extern "C" int vg_latent_adam(float* z, float* m, float* v, int* t, float* best_loss, float* best_z, const void* dz,
                              const float* loss_rows, const float* p, const void* z_in, void* z_out, float* objective,
                              int B, int L, int ZP, double lr, double beta1, double beta2, double eps, float alpha_adv,
                              float prior_weight, int mode, int dtype, void* stream) {
    VG_CHECK_ARG(mode == VG_LATENT_INIT || mode == VG_LATENT_UPDATE || mode == VG_LATENT_TRACK, VG_EINVAL);
    VG_CHECK_ARG(B >= 1 && L >= 1 && ZP >= L, VG_EINVAL);
    VG_CHECK_ARG(z && best_loss && best_z, VG_EINVAL);
    if (mode == VG_LATENT_INIT) VG_CHECK_ARG(m && v && t && z_in, VG_EINVAL);
    else VG_CHECK_ARG(loss_rows != nullptr, VG_EINVAL);
    if (mode == VG_LATENT_UPDATE) {
        VG_CHECK_ARG(m && v && t && dz && z_out, VG_EINVAL);
        VG_CHECK_ARG(__builtin_isfinite(lr) && lr >= 0.0 && __builtin_isfinite(eps) && eps >= 0.0, VG_EINVAL);
        VG_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, VG_EINVAL);
    }
    VG_CHECK_ARG(__builtin_isfinite(alpha_adv) && alpha_adv >= 0.f && __builtin_isfinite(prior_weight) && prior_weight >= 0.f,
                 VG_EINVAL);
    VG_CHECK_ARG(dtype == VG_F32 || dtype == VG_BF16, VG_ENOSUP);
    VG_CHECK_ARG(ZP % 4 == 0, VG_EALIGN);
    const uintptr_t emask = dtype == VG_F32 ? 3u : 1u;
    VG_CHECK_ARG(((reinterpret_cast<uintptr_t>(dz) | reinterpret_cast<uintptr_t>(z_in) | reinterpret_cast<uintptr_t>(z_out)) & emask) == 0,
                 VG_EALIGN);
    const hipStream_t s = vg_stream(stream);
    if (dtype == VG_F32)
        hipLaunchKernelGGL(latent_adam_kernel<VG_F32>, dim3(B), dim3(64), 0, s, z, m, v, t, best_loss, best_z, dz, loss_rows, p,
                           z_in, z_out, objective, L, ZP, lr, beta1, beta2, eps, (double)alpha_adv, (double)prior_weight, mode);
    else
        hipLaunchKernelGGL(latent_adam_kernel<VG_BF16>, dim3(B), dim3(64), 0, s, z, m, v, t, best_loss, best_z, dz, loss_rows, p,
                           z_in, z_out, objective, L, ZP, lr, beta1, beta2, eps, (double)alpha_adv, (double)prior_weight, mode);
    return VG_LAUNCH_RC();
}
