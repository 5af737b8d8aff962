// Latent prior (main_vae.py:415-436 vals_to_hist / sample_distribution, :476-499 the generation loop): per-column
// histogram + cumulative distribution of the Encoder's (mu | logvar) rows, inverse-CDF draws from it straight into the
// Generator's input layout, and the [-1, 1] -> uint8 picture conversion.  The contracts (edge arithmetic, bin rule, cdf
// summation order, which Philox word feeds which number) are stated in include/vaegan_hip.h, "Latent prior".
// Everything here is a small streaming or latency-bound kernel: a fit reads N * D * 4 bytes twice (24 MB at the
// reference size), a draw touches two cdf rows per latent dimension.
#include <math.h>
#include "common.hpp"
#include "noise.hpp"

namespace {

constexpr int kColTile = 64;        // columns per workgroup tile of the two passes over x: one wavefront wide, so a
                                    // wave reads 256 contiguous bytes of a row
constexpr int kMaxRowParts = 256;   // row chunks of the min / max pass (= partial rows in the workspace)
constexpr int kMaxBinParts = 64;    // row chunks of the binning pass (each flushes its LDS histogram with global atomics)
constexpr int kLdsWords = 16000;    // 4-byte words of LDS one binning workgroup may use (histogram + edges), < 64 KB

int row_parts(int64_t N) {
    const int64_t p = (N + 63) / 64;
    return (int)(p < kMaxRowParts ? p : kMaxRowParts);
}
int bin_parts(int64_t N) {
    const int64_t p = (N + 255) / 256;
    return (int)(p < kMaxBinParts ? p : kMaxBinParts);
}
// LDS strides of one column's histogram / edge row (odd: columns spread over the banks) and the columns that fit
int hist_stride(int n_bins) { return n_bins | 1; }
int edge_stride(int n_bins) { return (n_bins + 1) | 1; }
int bin_col_tile(int n_bins) {
    const int ct = kLdsWords / (hist_stride(n_bins) + edge_stride(n_bins));
    return ct < kColTile ? ct : kColTile;               // >= 7 for n_bins <= 1024
}

// ---- pass 1: column min / max partials ----------------------------------------------------------------------------
// grid (row parts, column tiles of 64); a workgroup's four waves take rows r0 + w, r0 + w + 4, ...; partial[part][c].
// A column that holds a NaN or an infinity publishes NaN as its partial minimum (fminf / fmaxf would drop a NaN).
__global__ __launch_bounds__(256) void latent_minmax_kernel(const float* __restrict__ x, int64_t N, int D, int64_t stride,
                                                            int rows_per_part, float* __restrict__ pmin,
                                                            float* __restrict__ pmax) {
    __shared__ float smin[4][kColTile], smax[4][kColTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * kColTile + lane;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_part;
    int64_t r1 = r0 + rows_per_part;
    if (r1 > N) r1 = N;
    float lo = INFINITY, hi = -INFINITY;
    bool bad = false;
    if (c < D) {
        for (int64_t r = r0 + wave; r < r1; r += 4) {
            const float v = x[r * stride + c];
            bad = bad || !isfinite(v);
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    smin[wave][lane] = bad ? NAN : lo;
    smax[wave][lane] = hi;
    __syncthreads();
    if (wave == 0 && c < D) {
        float a = smin[0][lane], b = smax[0][lane];
        bool nan = a != a;
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            nan = nan || smin[w][lane] != smin[w][lane];
            a = fminf(a, smin[w][lane]);
            b = fmaxf(b, smax[w][lane]);
        }
        pmin[(int64_t)blockIdx.x * D + c] = nan ? NAN : a;
        pmax[(int64_t)blockIdx.x * D + c] = b;
    }
}

// numpy's bin edges in f32, every product and sum rounded on its own (np.linspace: arange(k) * step + start, last = stop)
__device__ __forceinline__ float edge_value(int k, int n_bins, float lo, float hi, float step) {
#pragma clang fp contract(off)
    if (k == n_bins) return hi;
    const float t = (float)k * step;
    return t + lo;
}

// ---- pass 2: one workgroup per column: range, edges, zeroed counts ---------------------------------------------------
__global__ __launch_bounds__(256) void latent_edges_kernel(const float* __restrict__ pmin, const float* __restrict__ pmax,
                                                           int nparts, int D, int n_bins, float* __restrict__ edges,
                                                           int32_t* __restrict__ counts, int32_t* __restrict__ colbad) {
    __shared__ float smin[256], smax[256];
    __shared__ int sbad[256];
    const int c = blockIdx.x, t = threadIdx.x;
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (int p = t; p < nparts; p += 256) {
        const float a = pmin[(int64_t)p * D + c], b = pmax[(int64_t)p * D + c];
        bad |= !isfinite(a) || !isfinite(b);
        lo = fminf(lo, a);
        hi = fmaxf(hi, b);
    }
    smin[t] = lo; smax[t] = hi; sbad[t] = bad;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            smin[t] = fminf(smin[t], smin[t + s]);
            smax[t] = fmaxf(smax[t], smax[t + s]);
            sbad[t] |= sbad[t + s];
        }
        __syncthreads();
    }
    lo = smin[0]; hi = smax[0]; bad = sbad[0];
    if (lo == hi) {                                    // numpy _get_outer_edges
        lo = __fsub_rn(lo, 0.5f);
        hi = __fadd_rn(hi, 0.5f);
    }
    const float step = __fdiv_rn(__fsub_rn(hi, lo), (float)n_bins);
    bad |= !isfinite(lo) || !isfinite(hi) || !isfinite(step);          // hi - lo may overflow
    if (t == 0) colbad[c] = bad;
    for (int k = t; k <= n_bins; k += 256) edges[(int64_t)c * (n_bins + 1) + k] = edge_value(k, n_bins, lo, hi, step);
    for (int k = t; k < n_bins; k += 256) counts[(int64_t)c * n_bins + k] = 0;
}

// ---- pass 3: binning -----------------------------------------------------------------------------------------------
// grid (row parts, column tiles of CT); LDS: the tile's edges and its histogram.  Thread t owns column t % CT and rows
// t / CT, t / CT + 256 / CT, ...  A first guess from the bin width is corrected against the edges until
// e[b] <= x < e[b + 1] (last bin closed), so the counts are those of the definition whatever the guess was.
__global__ __launch_bounds__(256) void latent_bin_kernel(const float* __restrict__ x, int64_t N, int D, int64_t stride,
                                                         int rows_per_part, int n_bins, int CT,
                                                         const float* __restrict__ edges, int32_t* __restrict__ counts) {
    extern __shared__ uint32_t lds[];
    const int HS = n_bins | 1, ES = (n_bins + 1) | 1;
    uint32_t* hist = lds;                                              // [CT][HS]
    float* e = reinterpret_cast<float*>(lds + CT * HS);                // [CT][ES]
    const int c0 = blockIdx.y * CT;
    const int ncol = D - c0 < CT ? D - c0 : CT;
    for (int i = threadIdx.x; i < CT * HS; i += 256) hist[i] = 0u;
    for (int i = threadIdx.x; i < ncol * (n_bins + 1); i += 256) {
        const int cl = i / (n_bins + 1), k = i - cl * (n_bins + 1);
        e[cl * ES + k] = edges[(int64_t)(c0 + cl) * (n_bins + 1) + k];
    }
    __syncthreads();
    const int cl = threadIdx.x % CT, rl = threadIdx.x / CT, RL = 256 / CT;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_part;
    int64_t r1 = r0 + rows_per_part;
    if (r1 > N) r1 = N;
    if (cl < ncol && rl < RL) {
        const float* ec = e + cl * ES;
        const float lo = ec[0];
        const float scale = (float)n_bins / (ec[n_bins] - lo);
        const float top = (float)(n_bins - 1);
        for (int64_t r = r0 + rl; r < r1; r += RL) {
            const float v = x[r * stride + c0 + cl];
            int b = (int)fminf(fmaxf((v - lo) * scale, 0.f), top);     // a NaN ends as 0: always inside the histogram
            while (b > 0 && v < ec[b]) --b;
            while (b < n_bins - 1 && v >= ec[b + 1]) ++b;
            atomicAdd(&hist[cl * HS + b], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ncol * n_bins; i += 256) {
        const int k = i / n_bins, b = i - k * n_bins;
        const uint32_t h = hist[k * HS + b];
        if (h) atomicAdd(&counts[(int64_t)(c0 + k) * n_bins + b], (int32_t)h);
    }
}

// ---- pass 4: cdf = np.cumsum(counts / N) in f64, summed in bin order; status -----------------------------------------
__global__ __launch_bounds__(256) void latent_cdf_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ colbad,
                                                         int64_t N, int D, int n_bins, double* __restrict__ cdf,
                                                         int32_t* __restrict__ status) {
    __shared__ int sbad;
    if (threadIdx.x == 0) sbad = 0;
    __syncthreads();
    const double n = (double)N;
    int bad = 0;
    for (int c = threadIdx.x; c < D; c += 256) {
        bad |= colbad[c];
        double acc = 0.0;
        for (int b = 0; b < n_bins; ++b) {
            acc = __dadd_rn(acc, __ddiv_rn((double)counts[(int64_t)c * n_bins + b], n));
            cdf[(int64_t)c * n_bins + b] = acc;
        }
    }
    if (bad) atomicOr(&sbad, 1);
    __syncthreads();
    if (threadIdx.x == 0) status[0] = sbad;
}

// ---- sampling --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double u01_word(uint32_t w) { return (double)((float)(w >> 8) * 5.9604644775390625e-08f); }

__device__ __forceinline__ double uniform_at(const double* inj, unsigned long long seed, unsigned long long step,
                                             uint32_t draw, int64_t i) {
    if (inj) return inj[i];
    uint32_t w[4];
    philox4x32_10(seed, step, draw, (unsigned long long)i >> 2, w);
    const uint32_t sel = (uint32_t)(i & 3);
    return u01_word(sel == 0 ? w[0] : sel == 1 ? w[1] : sel == 2 ? w[2] : w[3]);
}

// legacy np.random.uniform(x0, x1) = x0 + (x1 - x0) * v in f64, each operation rounded on its own, then one rounding to f32
__device__ __forceinline__ float uniform_in_bin(double x0, double x1, double v) {
#pragma clang fp contract(off)
    const double w = x1 - x0;
    const double t = w * v;
    return (float)(x0 + t);
}

// np.searchsorted(cdf_row, u) (side left) clamped to the last bin, then the uniform draw inside that bin
__device__ __forceinline__ float draw_column(const float* __restrict__ erow, const double* __restrict__ crow, int n_bins,
                                             double u, double v) {
    int lo = 0, hi = n_bins;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (crow[mid] < u) lo = mid + 1; else hi = mid;
    }
    const int idx = lo < n_bins - 1 ? lo : n_bins - 1;
    return uniform_in_bin((double)erow[idx], (double)erow[idx + 1], v);
}

// one thread per (draw j, output column i < W), W = ZP when z is written, else L
template <int DT>
__global__ __launch_bounds__(256) void latent_sample_kernel(const float* __restrict__ edges, const double* __restrict__ cdf,
                                                            int n_bins, int L, int64_t n, int W, const double* __restrict__ u,
                                                            const double* __restrict__ v, const float* __restrict__ eps,
                                                            const unsigned long long* __restrict__ rng,
                                                            float* __restrict__ mulv, void* __restrict__ z) {
    const unsigned long long seed = rng ? rng[0] : 0ull, step = rng ? rng[1] : 0ull;
    const int64_t total = n * W;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = t / W;
        const int i = (int)(t - j * W);
        float zv = 0.f;
        if (i < L) {
            float s[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = h * L + i;
                const int64_t e = j * (2 * L) + c;
                const double uu = uniform_at(u, seed, step, VG_DRAW_LATENT_U, e);
                const double vv = uniform_at(v, seed, step, VG_DRAW_LATENT_V, e);
                s[h] = draw_column(edges + (int64_t)c * (n_bins + 1), cdf + (int64_t)c * n_bins, n_bins, uu, vv);
                if (mulv) mulv[e] = s[h];
            }
            if (z) {
                const float lv = fminf(fmaxf(s[1], -10.f), 10.f);
                const float ep = eps ? eps[j * L + i]
                                     : philox_randn(seed, step, VG_DRAW_LATENT_EPS, (unsigned long long)(j * L + i));
                zv = s[0] + expf(0.5f * lv) * ep;
            }
        }
        if (z) store1<DT>(z, t, zv);
    }
}

// ---- [-1, 1] f32 NCHW -> uint8 ---------------------------------------------------------------------------------------
// (x + 1) / 2 * 255, clamp, truncate (main_vae.py:492,498-499); a NaN becomes 0
__device__ __forceinline__ uint8_t to_byte(float x) {
#pragma clang fp contract(off)
    const float a = x + 1.0f;
    const float h = a / 2.0f;
    const float t = h * 255.0f;
    return (uint8_t)(int)fminf(fmaxf(t, 0.0f), 255.0f);
}

__global__ __launch_bounds__(256) void to_u8_kernel(const float* __restrict__ x, uint8_t* __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        y[i] = to_byte(x[i]);
}

// one picture [rows * H][cols * W][C]: image i at tile (i / cols, i % cols); tiles past the batch are zero
__global__ __launch_bounds__(256) void to_u8_grid_kernel(const float* __restrict__ x, uint8_t* __restrict__ y, int B, int C,
                                                         int H, int W, int cols, int64_t n) {
    const int64_t PW = (int64_t)cols * W;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < n; o += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(o % C);
        const int64_t p = o / C;
        const int64_t Y = p / PW, X = p - Y * PW;
        const int64_t img = (Y / H) * cols + X / W;
        uint8_t out = 0;
        if (img < B) out = to_byte(x[((img * C + c) * H + Y % H) * W + X % W]);
        y[o] = out;
    }
}

unsigned grid_for(int64_t n) {
    int64_t b = (n + 255) / 256;
    if (b > 4096) b = 4096;
    return (unsigned)(b < 1 ? 1 : b);
}

bool hist_args_ok(int64_t N, int D, int n_bins) {
    return N >= 1 && N <= 2147483647ll && D >= 1 && n_bins >= 1 && n_bins <= 1024;
}

}  // namespace

extern "C" int64_t vg_latent_hist_ws_bytes(int64_t N, int D, int n_bins) {
    if (!hist_args_ok(N, D, n_bins)) return VG_EINVAL;
    return ((int64_t)2 * row_parts(N) * D + D) * 4;
}

extern "C" int vg_latent_hist(const float* x, int64_t N, int D, int64_t row_stride, int n_bins, float* edges,
                              int32_t* counts, double* cdf, int32_t* status, void* ws, int64_t ws_bytes, void* stream) {
    VG_CHECK_ARG(x && edges && counts && cdf && status && ws && hist_args_ok(N, D, n_bins) && row_stride >= D, VG_EINVAL);
    VG_CHECK_ARG(ws_bytes >= vg_latent_hist_ws_bytes(N, D, n_bins), VG_EINVAL);
    VG_CHECK_ARG((reinterpret_cast<uintptr_t>(cdf) & 7u) == 0 && (reinterpret_cast<uintptr_t>(ws) & 3u) == 0, VG_EALIGN);
    hipStream_t st = vg_stream(stream);
    // rows per part first, then the part count again from it: no part is empty (an empty part's +-inf partials would
    // read as a non-finite column)
    const int rows1 = (int)((N + row_parts(N) - 1) / row_parts(N));
    const int RP = (int)((N + rows1 - 1) / rows1);
    float* pmin = static_cast<float*>(ws);
    float* pmax = pmin + (int64_t)RP * D;
    int32_t* colbad = reinterpret_cast<int32_t*>(pmax + (int64_t)RP * D);
    const int col_tiles = (D + kColTile - 1) / kColTile;
    VG_CHECK_ARG(col_tiles <= 65535, VG_EINVAL);
    hipLaunchKernelGGL(latent_minmax_kernel, dim3(RP, col_tiles), dim3(256), 0, st, x, N, D, row_stride, rows1, pmin, pmax);
    hipLaunchKernelGGL(latent_edges_kernel, dim3(D), dim3(256), 0, st, pmin, pmax, RP, D, n_bins, edges, counts, colbad);
    const int CT = bin_col_tile(n_bins);
    const int rows3 = (int)((N + bin_parts(N) - 1) / bin_parts(N));
    const int BP = (int)((N + rows3 - 1) / rows3);
    const int tiles3 = (D + CT - 1) / CT;
    VG_CHECK_ARG(tiles3 <= 65535, VG_EINVAL);
    const size_t lds = (size_t)CT * (hist_stride(n_bins) + edge_stride(n_bins)) * 4;
    hipLaunchKernelGGL(latent_bin_kernel, dim3(BP, tiles3), dim3(256), lds, st, x, N, D, row_stride, rows3, n_bins, CT,
                       edges, counts);
    hipLaunchKernelGGL(latent_cdf_kernel, dim3(1), dim3(256), 0, st, counts, colbad, N, D, n_bins, cdf, status);
    return VG_LAUNCH_RC();
}

extern "C" int vg_latent_sample(const float* edges, const double* cdf, int n_bins, int L, int64_t n, const double* u,
                                const double* v, const float* eps, const uint64_t* rng, float* mulv, void* z, int ZP,
                                int dtype, void* stream) {
    VG_CHECK_ARG(edges && cdf && n_bins >= 1 && n_bins <= 1024 && L >= 1 && n >= 1 && (mulv || z), VG_EINVAL);
    VG_CHECK_ARG((u == nullptr) == (v == nullptr), VG_EINVAL);          // both injected or both drawn
    VG_CHECK_ARG(rng || (u && (eps || !z)), VG_EINVAL);                // whatever is not injected needs the generator
    VG_CHECK_ARG(n * (int64_t)(2 * L) < (1ll << 40), VG_EINVAL);
    int W = L;
    if (z) {
        VG_CHECK_ARG(dtype == VG_F32 || dtype == VG_BF16, VG_ENOSUP);
        VG_CHECK_ARG(ZP >= L, VG_EINVAL);
        VG_CHECK_ARG(vg_aligned16(z), VG_EALIGN);
        W = ZP;
    } else {
        dtype = VG_F32;
    }
    VG_CHECK_ARG((reinterpret_cast<uintptr_t>(cdf) & 7u) == 0 && (reinterpret_cast<uintptr_t>(u) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(v) & 7u) == 0, VG_EALIGN);
    const dim3 grid(grid_for(n * W)), block(256);
    hipStream_t st = vg_stream(stream);
    const unsigned long long* r = reinterpret_cast<const unsigned long long*>(rng);
    if (dtype == VG_F32)
        hipLaunchKernelGGL(latent_sample_kernel<VG_F32>, grid, block, 0, st, edges, cdf, n_bins, L, n, W, u, v, eps, r, mulv, z);
    else
        hipLaunchKernelGGL(latent_sample_kernel<VG_BF16>, grid, block, 0, st, edges, cdf, n_bins, L, n, W, u, v, eps, r, mulv, z);
    return VG_LAUNCH_RC();
}

extern "C" int vg_to_u8(const float* x, uint8_t* y, int B, int C, int H, int W, int grid_cols, void* stream) {
    VG_CHECK_ARG(x && y && B > 0 && C > 0 && H > 0 && W > 0 && grid_cols >= 0, VG_EINVAL);
    hipStream_t st = vg_stream(stream);
    if (grid_cols == 0) {
        const int64_t n = (int64_t)B * C * H * W;
        hipLaunchKernelGGL(to_u8_kernel, dim3(grid_for(n)), dim3(256), 0, st, x, y, n);
    } else {
        const int64_t rows = ((int64_t)B + grid_cols - 1) / grid_cols;
        const int64_t n = rows * H * grid_cols * W * C;
        hipLaunchKernelGGL(to_u8_grid_kernel, dim3(grid_for(n)), dim3(256), 0, st, x, y, B, C, H, W, grid_cols, n);
    }
    return VG_LAUNCH_RC();
}
