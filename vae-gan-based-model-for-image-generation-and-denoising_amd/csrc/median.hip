// Median baseline (include/vaegan_hip.h "Median baseline"): the per-channel (2r+1)^2 median of an f32 NCHW batch, r in {1, 2},
// reflection at the border.  No MFMA and almost no arithmetic: the launch moves 8 bytes per pixel and selects.
//
// One workgroup of 256 threads owns one 64 x 16 output tile of one plane (image, channel).  It stages the tile plus its r halo in
// LDS -- every global load of a thread issued before its first LDS write, reflection resolved in the address, consecutive
// threads on consecutive columns -- and after one barrier each thread selects FOUR horizontally adjacent outputs from the
// (2r+1) x (4+2r) window it reads with 16-byte LDS reads (the window starts on a 16-byte boundary of the LDS row), and writes
// them with one 16-byte store where W % 4 == 0 and y is 16-byte aligned, with bounded 4-byte stores elsewhere.
//
// Selection is branch-free and exact: every step is a min, a max or a median-of-3 (v_med3_f32) of input values.
//   r = 1   columns sorted once per thread and shared by the outputs that see them (lo, mid, hi of 3 values); the median of
//           nine is med3(max3(lo's), med3(mid's), min3(hi's)) of the three columns (Smith's network).
//   r = 2   forgetful selection (Devillard, "Fast median search"): of any 14 of the 25 values neither the smallest nor the
//           largest can be the median, so both are dropped and one new value is added; with 13, 12, ... the same holds down
//           to the last three, whose median-of-3 is the answer.  Moving the extremes to the ends of n values takes
//           floor(n/2) + 2 (ceil(n/2) - 1) compare-exchanges.
// All indices are compile-time constants after unrolling: the windows live in registers, nothing spills.
#include "common.hpp"

namespace {

constexpr int MED_TW = 64, MED_TH = 16, MED_THREADS = 256;
constexpr int MED_PITCH = 72;              // floats between LDS rows: >= 64 + 2 * 2, a multiple of 4 (16-byte window reads)

__device__ __forceinline__ int med_reflect(int g, int n) {
    g = g < 0 ? -g : g;
    g = g > n - 1 ? 2 * (n - 1) - g : g;
    return g < 0 ? 0 : (g > n - 1 ? n - 1 : g);       // only coordinates no stored output reads need the clamp
}

__device__ __forceinline__ void med_cx(float& a, float& b) {      // compare-exchange: a <= b afterwards
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo; b = hi;
}

// smallest of v[0 .. n-1] to v[0], largest to v[n-1]; the others keep their multiset
template <int N>
__device__ __forceinline__ void med_extremes(float (&v)[14]) {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) med_cx(v[i], v[N - 1 - i]);           // lows in the first half, highs in the second
    constexpr int L = (N + 1) / 2;                                        // v[0 .. L-1] holds the minimum (the middle one too)
#pragma unroll
    for (int i = 1; i < L; ++i) med_cx(v[0], v[i]);
    constexpr int F = N / 2;                                              // v[F .. N-1] holds the maximum
#pragma unroll
    for (int i = F; i < N - 1; ++i) med_cx(v[i], v[N - 1]);
}

// one forgetful step at N live values v[0 .. N-1]: drop both extremes, take `next`, leaving N - 1 live values v[0 .. N-2]
template <int N>
__device__ __forceinline__ void med_forget(float (&v)[14], float next) {
    med_extremes<N>(v);
    v[0] = next;                           // live: v[0] the new value, v[1 .. N-2] the survivors
}

__device__ __forceinline__ float median25(const float (&w)[25]) {
    float v[14];
#pragma unroll
    for (int i = 0; i < 14; ++i) v[i] = w[i];
    med_forget<14>(v, w[14]);
    med_forget<13>(v, w[15]);
    med_forget<12>(v, w[16]);
    med_forget<11>(v, w[17]);
    med_forget<10>(v, w[18]);
    med_forget<9>(v, w[19]);
    med_forget<8>(v, w[20]);
    med_forget<7>(v, w[21]);
    med_forget<6>(v, w[22]);
    med_forget<5>(v, w[23]);
    med_forget<4>(v, w[24]);
    return __builtin_amdgcn_fmed3f(v[0], v[1], v[2]);
}

template <int R>
__global__ __launch_bounds__(MED_THREADS) void median_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W,
                                                             int vec) {
    constexpr int LH = MED_TH + 2 * R, LW = MED_TW + 2 * R;               // staged rows / columns
    constexpr int ITEMS = LH * LW, NIT = (ITEMS + MED_THREADS - 1) / MED_THREADS;
    constexpr int K = 2 * R + 1, WC = 4 + 2 * R;                          // window rows, window columns of four outputs
    __shared__ __attribute__((aligned(16))) float tile[LH * MED_PITCH];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.z * MED_TW, y0 = blockIdx.y * MED_TH;
    const size_t plane = (size_t)H * W;
    const float* __restrict__ xp = x + (size_t)blockIdx.x * plane;
    float* __restrict__ yp = y + (size_t)blockIdx.x * plane;

    // ---- stage: all loads, then all LDS writes ----
    float st[NIT];
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        const int e = tid + k * MED_THREADS;
        const int row = e / LW, col = e - row * LW;
        st[k] = 0.f;
        if (e < ITEMS) st[k] = xp[(size_t)med_reflect(y0 - R + row, H) * W + med_reflect(x0 - R + col, W)];
    }
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        const int e = tid + k * MED_THREADS;
        const int row = e / LW, col = e - row * LW;
        if (e < ITEMS) tile[row * MED_PITCH + col] = st[k];
    }
    __syncthreads();

    // ---- this thread's four outputs: row ty, columns 4 tx .. 4 tx + 3 of the tile ----
    const int tx = tid & 15, ty = tid >> 4;
    float win[K][8];                                                      // LDS columns 4 tx .. 4 tx + 7 (WC <= 8 of them used)
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float4* q = reinterpret_cast<const float4*>(tile + (ty + i) * MED_PITCH + 4 * tx);
        const float4 a = q[0], b = q[1];
        win[i][0] = a.x; win[i][1] = a.y; win[i][2] = a.z; win[i][3] = a.w;
        win[i][4] = b.x; win[i][5] = b.y; win[i][6] = b.z; win[i][7] = b.w;
    }
    float out[4];
    if constexpr (R == 1) {
        float lo[WC], mid[WC], hi[WC];
#pragma unroll
        for (int j = 0; j < WC; ++j) {
            lo[j] = fminf(fminf(win[0][j], win[1][j]), win[2][j]);
            hi[j] = fmaxf(fmaxf(win[0][j], win[1][j]), win[2][j]);
            mid[j] = __builtin_amdgcn_fmed3f(win[0][j], win[1][j], win[2][j]);
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const float a = fmaxf(fmaxf(lo[o], lo[o + 1]), lo[o + 2]);
            const float m = __builtin_amdgcn_fmed3f(mid[o], mid[o + 1], mid[o + 2]);
            const float b = fminf(fminf(hi[o], hi[o + 1]), hi[o + 2]);
            out[o] = __builtin_amdgcn_fmed3f(a, m, b);
        }
    } else {
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float w[25];
#pragma unroll
            for (int i = 0; i < 5; ++i)
#pragma unroll
                for (int j = 0; j < 5; ++j) w[i * 5 + j] = win[i][o + j];
            out[o] = median25(w);
        }
    }
    const int px = x0 + 4 * tx, py = y0 + ty;
    if (py >= H) return;
    float* __restrict__ dst = yp + (size_t)py * W + px;
    if (vec) {                                                            // W % 4 == 0: the quad is inside or outside as a whole
        if (px < W) *reinterpret_cast<float4*>(dst) = float4{out[0], out[1], out[2], out[3]};
    } else {
#pragma unroll
        for (int o = 0; o < 4; ++o)
            if (px + o < W) dst[o] = out[o];
    }
}

}  // namespace

extern "C" int vg_median_filter(const float* x, float* y, int B, int C, int H, int W, int radius, void* stream) {
    VG_CHECK_ARG(x && y, VG_EINVAL);
    VG_CHECK_ARG(B >= 1 && C >= 1 && H >= 1 && W >= 1 && radius >= 1 && radius <= 2, VG_EINVAL);
    VG_CHECK_ARG((H < W ? H : W) >= radius + 1, VG_EINVAL);
    const int64_t total = (int64_t)B * C * H * W, planes = (int64_t)B * C;
    const int ty = (H + MED_TH - 1) / MED_TH, tx = (W + MED_TW - 1) / MED_TW;
    VG_CHECK_ARG(total <= 0x7fffffffLL && planes <= 0x7fffffffLL && ty <= 65535 && tx <= 65535, VG_EINVAL);
    {   // aliasing: any overlap of the two buffers (y == x included)
        const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(y);
        const uintptr_t bytes = (uintptr_t)total * sizeof(float);
        VG_CHECK_ARG(xa + bytes <= ya || ya + bytes <= xa, VG_EINVAL);
    }
    VG_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 3u) == 0 && (reinterpret_cast<uintptr_t>(y) & 3u) == 0, VG_EALIGN);
    const int vec = (W % 4 == 0 && vg_aligned16(y)) ? 1 : 0;
    const dim3 grid((unsigned)planes, (unsigned)ty, (unsigned)tx);
    hipStream_t s = vg_stream(stream);
    if (radius == 1) hipLaunchKernelGGL(median_kernel<1>, grid, dim3(MED_THREADS), 0, s, x, y, H, W, vec);
    else hipLaunchKernelGGL(median_kernel<2>, grid, dim3(MED_THREADS), 0, s, x, y, H, W, vec);
    return VG_LAUNCH_RC();
}
