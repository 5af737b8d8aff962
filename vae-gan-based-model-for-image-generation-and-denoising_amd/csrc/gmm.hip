// Gaussian-mixture latent prior (ex-post density estimation, Ghosh et al. 2020, "From Variational to Deterministic
// Autoencoders"): the two GEMM-shaped phases of one EM iteration over the Encoder's latents, and the sampler.  The
// contracts are stated in include/vaegan_hip.h, "Gaussian-mixture prior".
//   vg_gmm_log_resp   E-step: per row and component the quadratic form |(x - mean_k) U_k|^2 on v_mfma_f64_16x16x4_f64,
//                     then the log-sum-exp over the components
//   vg_gmm_moments    M-step sums: nk, s1 = sum r d, s2 = sum r d d^T with d = x - shift_k, (r * d)^T d on the same MFMA
//                     over a fixed row split; the splits' partials are added in split order by a second launch
//   vg_gmm_sample     component by inverse cdf, z = mean_k + L_k eps, straight into the Generator's input layout
// The K small D x D steps between the two phases (Cholesky, triangular inverse) are the caller's, on the host.
#include <math.h>
#include "common.hpp"
#include "noise.hpp"

typedef __attribute__((ext_vector_type(4))) double f64x4;

namespace {

constexpr int kMaxD = 256;
constexpr int kMaxK = 64;
constexpr int kLdsBudget = 65536;

bool gmm_args_ok(int64_t N, int D, int K) {
    return N >= 1 && N <= 2147483647ll && D >= 1 && D <= kMaxD && K >= 1 && K <= kMaxK;
}
bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// ---- E-step ------------------------------------------------------------------------------------------------------------
// A workgroup owns R = 16 * RF rows; its x tile sits in LDS as f32 [R][DP + 4], DP = D rounded up to 16, pad columns and
// rows past N zero.  Per component the four waves share the rows and split the 16-column tiles of y = d U_k.  U_k is upper
// triangular, so column tile jt needs only d's columns below 16 (jt + 1) (entries below the diagonal are never read) and
// costs jt + 1 units: the tiles are dealt from the widest down in boustrophedon order (waves 0 1 2 3, 3 2 1 0, ...), which
// evens the waves' work out (7 tiles, D = 100: 7 units each).  MFMA operands: A[row][i] = d (one f64 per lane, row = lane & 15, i = i0 + (lane >> 4)),
// B[i][col] = U_k[i][col] from global memory (the K factors stay in L2); C/D: col = lane & 15, row = (lane >> 4) + 4 * reg.
// The sum of squares over a tile's columns is the epilogue: 16 lanes of a row by xor shuffles, the four waves through LDS.
int64_t eresp_lds_bytes(int RF, int D, int K) {
    const int R = 16 * RF, DP = (D + 15) & ~15;
    return (int64_t)8 * (DP + 4 * R + K * R + R) + (int64_t)4 * R * (DP + 4);
}

template <int RF>
__global__ __launch_bounds__(256) void gmm_log_resp_kernel(const float* __restrict__ x, int64_t N, int D, int64_t stride,
                                                           int K, const double* __restrict__ mean,
                                                           const double* __restrict__ U, const double* __restrict__ log_coef,
                                                           double* __restrict__ log_prob, double* __restrict__ log_norm,
                                                           double* __restrict__ resp) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int R = 16 * RF;
    const int DP = (D + 15) & ~15, XS = DP + 4, DT = DP >> 4;
    double* sm = reinterpret_cast<double*>(smem);      // [DP]    mean_k, pad columns 0
    double* spart = sm + DP;                           // [4][R]  the waves' partial sums of squares
    double* slp = spart + 4 * R;                       // [K][R]  log_prob
    double* sln = slp + K * R;                         // [R]     log_norm
    float* sx = reinterpret_cast<float*>(sln + R);     // [R][XS]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lc = lane & 15, lq = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * R;

    for (int e = t; e < R * DP; e += 256) {
        const int r = e / DP, c = e - r * DP;
        const int64_t row = row0 + r;
        sx[r * XS + c] = (row < N && c < D) ? x[row * stride + c] : 0.f;
    }
    for (int k = 0; k < K; ++k) {
        __syncthreads();
        for (int c = t; c < DP; c += 256) sm[c] = c < D ? mean[(int64_t)k * D + c] : 0.0;
        __syncthreads();
        const double* Uk = U + (int64_t)k * D * D;
        double sq[RF][4];
#pragma unroll
        for (int f = 0; f < RF; ++f)
#pragma unroll
            for (int g = 0; g < 4; ++g) sq[f][g] = 0.0;
        for (int rd = 0; 4 * rd < DT; ++rd) {
            const int p = 4 * rd + ((rd & 1) ? 3 - wave : wave);
            if (p >= DT) continue;
            const int jt = DT - 1 - p, col = jt * 16 + lc;
            f64x4 acc[RF];
#pragma unroll
            for (int f = 0; f < RF; ++f) acc[f] = f64x4{0.0, 0.0, 0.0, 0.0};
            const int iend = (jt + 1) * 16;
            auto load_b = [&](int i) { return (col < D && i <= col) ? Uk[(int64_t)i * D + col] : 0.0; };
            double bnext = load_b(lq);
            for (int i0 = 0; i0 < iend; i0 += 4) {
                const int i = i0 + lq;
                const double b = bnext;
                if (i0 + 4 < iend) bnext = load_b(i + 4);              // in flight while this step's MFMAs run
                const double mu = sm[i];
#pragma unroll
                for (int f = 0; f < RF; ++f) {
                    const double a = (double)sx[(16 * f + lc) * XS + i] - mu;
                    acc[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[f], 0, 0, 0);
                }
            }
#pragma unroll
            for (int f = 0; f < RF; ++f)
#pragma unroll
                for (int g = 0; g < 4; ++g) sq[f][g] += acc[f][g] * acc[f][g];
        }
#pragma unroll
        for (int f = 0; f < RF; ++f)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                double v = sq[f][g];
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
                if (lc == 0) spart[wave * R + 16 * f + lq + 4 * g] = v;
            }
        __syncthreads();
        if (t < R) slp[k * R + t] = log_coef[k] - 0.5 * (((spart[t] + spart[R + t]) + spart[2 * R + t]) + spart[3 * R + t]);
    }
    __syncthreads();
    if (t < R) {
        double m = slp[t];
        for (int k = 1; k < K; ++k) {
            const double v = slp[k * R + t];
            m = v > m ? v : m;                         // a NaN stays or surfaces in the sum below
        }
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += exp(slp[k * R + t] - m);
        const double ln = m + log(s);
        sln[t] = ln;
        if (log_norm && row0 + t < N) log_norm[row0 + t] = ln;
    }
    __syncthreads();
    const int64_t left = N - row0;
    const int nrows = left < R ? (int)left : R;
    for (int e = t; e < nrows * K; e += 256) {
        const int r = e / K, k = e - r * K;
        const double lp = slp[k * R + r];
        if (log_prob) log_prob[row0 * K + e] = lp;
        if (resp) resp[row0 * K + e] = exp(lp - sln[r]);
    }
}

// ---- M-step sums ---------------------------------------------------------------------------------------------------
// s2_k is cut into 16 x 16 blocks, one MFMA accumulator each; only the blocks bi <= bj exist (NB = TB (TB + 1) / 2 with
// TB = ceil(D / 16)), numbered row by row.  A workgroup owns one component, one row split and one chunk of 32 blocks:
// wave w takes blocks chunk * 32 + 4 b + w, b < 8, so D <= 112 is a single chunk and the x rows are read once per
// component.  The rows go through LDS 16 at a time as d = (double)x - shift_k, f64 [16][DP + 2], pad columns and rows past
// the split zero; the next 16 rows are loaded into registers while the MFMAs of the current ones run.
constexpr int kMW = 8;            // blocks per wave
constexpr int kMC = 4 * kMW;      // blocks per workgroup
constexpr int kMK = 16;           // rows staged per step
constexpr int kMTargetWgs = 768;  // 256 CUs x 3 resident workgroups (registers): one round, no tail

struct MomPlan {
    int TB, NB, chunks, splits;
    int64_t rows_per_split;                                     // up to 2^31 when one split holds every row
};

MomPlan mom_plan(int64_t N, int D, int K) {
    MomPlan p;
    p.TB = (D + 15) / 16;
    p.NB = p.TB * (p.TB + 1) / 2;
    p.chunks = (p.NB + kMC - 1) / kMC;
    int64_t s = kMTargetWgs / (p.chunks * K);
    if (s < 1) s = 1;
    const int64_t most = (N + 63) / 64;                         // at least 64 rows per split
    if (s > most) s = most;
    if (s < 1) s = 1;
    int64_t rps = (N + s - 1) / s;
    rps = (rps + kMK - 1) / kMK * kMK;
    p.rows_per_split = rps;
    p.splits = (int)((N + rps - 1) / rps);
    if (p.splits < 1) p.splits = 1;
    return p;
}

int64_t mom_ws_doubles(const MomPlan& p, int K) {
    return (int64_t)p.splits * ((int64_t)K * ((int64_t)p.NB * 256 + p.TB * 16 + 1) + 1);
}
int64_t mom_lds_bytes(int D) {
    const int DP = (D + 15) & ~15;
    return (int64_t)8 * (kMK * (DP + 2) + 2 * kMK + DP);
}

// block q of the upper triangle, row by row -> (bi, bj)
__device__ __forceinline__ void block_of(int q, int TB, int& bi, int& bj) {
    bi = 0;
    while (q >= TB - bi) { q -= TB - bi; ++bi; }
    bj = bi + q;
}

// grid (chunks, row splits, K).  The MFMA's "k" runs over the rows: A[i][n] = r_n * d_n[16 bi + i], B[n][j] = d_n[16 bj + j].
// Chunk 0 also carries s1 (one thread per column, rows in ascending order), nk and, for component 0, the sum of log_norm.
__global__ __launch_bounds__(256) void gmm_moments_kernel(const float* __restrict__ x, int64_t N, int D, int64_t stride,
                                                          int K, const double* __restrict__ shift,
                                                          const double* __restrict__ resp, const double* __restrict__ log_norm,
                                                          int64_t rows_per_split, int TB, int NB, double* __restrict__ pouter,
                                                          double* __restrict__ psum, double* __restrict__ pnk,
                                                          double* __restrict__ pll) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int DP = TB * 16, DS = DP + 2;
    double* sd = reinterpret_cast<double*>(smem);      // [kMK][DS]
    double* sr = sd + kMK * DS;                        // [kMK] resp of the staged rows
    double* sl = sr + kMK;                             // [kMK] log_norm of the staged rows
    double* ssh = sl + kMK;                            // [DP]  shift_k, pad columns 0
    const int k = blockIdx.z;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lc = lane & 15, lq = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_split;
    int64_t r1 = r0 + rows_per_split;
    if (r1 > N) r1 = N;
    const double* sh = shift + (int64_t)k * D;
    const bool first = blockIdx.x == 0;
    const bool want_ll = first && k == 0 && log_norm != nullptr;

    // this wave's blocks
    int ca[kMW], cb[kMW], nb = 0;
#pragma unroll
    for (int b = 0; b < kMW; ++b) {
        const int q = blockIdx.x * kMC + 4 * b + wave;
        int bi = 0, bj = 0;
        if (q < NB) {
            block_of(q, TB, bi, bj);
            nb = b + 1;
        }
        ca[b] = 16 * bi;
        cb[b] = 16 * bj;
    }
    f64x4 acc[kMW];
#pragma unroll
    for (int b = 0; b < kMW; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};

    // staging: thread t owns row t >> 4 of the step and column (t & 15) of every 16-column block s < TB <= 16
    const int sn = t >> 4, sc = t & 15;
    float px[16];
    double pr = 0.0;
    auto fetch = [&](int64_t r) {
        const bool in = r + sn < r1;
        const float* xr = x + (r + sn) * stride + sc;
#pragma unroll
        for (int s = 0; s < 16; ++s) px[s] = (in && 16 * s + sc < D) ? xr[16 * s] : 0.f;
        if (t < kMK) {
            pr = r + t < r1 ? resp[(r + t) * K + k] : 0.0;
        } else if (t < 2 * kMK) {
            const int64_t row = r + t - kMK;
            pr = (want_ll && row < r1) ? log_norm[row] : 0.0;
        }
    };
    double csum = 0.0, nksum = 0.0, llsum = 0.0;
    if (t < DP) ssh[t] = t < D ? sh[t] : 0.0;
    if (r0 < r1) fetch(r0);
    __syncthreads();
    for (int64_t r = r0; r < r1; r += kMK) {
        __syncthreads();                               // the previous step's MFMAs have read sd
        {
            const bool in = r + sn < r1;
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int c = 16 * s + sc;
                if (s < TB) sd[sn * DS + c] = (in && c < D) ? (double)px[s] - ssh[c] : 0.0;
            }
        }
        if (t < kMK) sr[t] = pr; else if (t < 2 * kMK) sl[t - kMK] = pr;
        __syncthreads();
        if (r + kMK < r1) fetch(r + kMK);
        if (first) {
            if (t < DP) {
#pragma unroll 8
                for (int n = 0; n < kMK; ++n) csum += sr[n] * sd[n * DS + t];        // row order: the sum's order is fixed
            }
            if (t == 0) {
#pragma unroll 8
                for (int n = 0; n < kMK; ++n) nksum += sr[n];
            }
            if (want_ll && t == 64) {
#pragma unroll 8
                for (int n = 0; n < kMK; ++n) llsum += sl[n];
            }
        }
#pragma unroll 1                                        // one k-step's operands in registers at a time
        for (int kk = 0; kk < kMK; kk += 4) {
            const int n = kk + lq;
            const double rn = sr[n];
            const double* drow = sd + n * DS + lc;
#pragma unroll
            for (int b = 0; b < kMW; ++b) {
                if (b < nb) {
                    const double a = rn * drow[ca[b]];
                    acc[b] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, drow[cb[b]], acc[b], 0, 0, 0);
                }
            }
        }
    }
    // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
    const int64_t sk = (int64_t)blockIdx.y * K + k;
#pragma unroll
    for (int b = 0; b < kMW; ++b) {
        if (b < nb) {
            double* out = pouter + (sk * NB + blockIdx.x * kMC + 4 * b + wave) * 256;
#pragma unroll
            for (int g = 0; g < 4; ++g) out[(lq + 4 * g) * 16 + lc] = acc[b][g];
        }
    }
    if (first) {
        if (t < DP) psum[sk * DP + t] = csum;
        if (t == 0) pnk[sk] = nksum;
        if (k == 0 && t == 64) pll[blockIdx.y] = llsum;
    }
}

// grid (NB, 1, K): the splits' partials are added in split order and stored; the entries below the diagonal are copies
__global__ __launch_bounds__(256) void gmm_moments_reduce_kernel(const double* __restrict__ pouter,
                                                                 const double* __restrict__ psum,
                                                                 const double* __restrict__ pnk, const double* __restrict__ pll,
                                                                 int splits, int D, int K, int TB, int NB, double* __restrict__ nk,
                                                                 double* __restrict__ s1, double* __restrict__ s2,
                                                                 double* __restrict__ loglik_sum) {
    int bi, bj;
    block_of(blockIdx.x, TB, bi, bj);
    const int k = blockIdx.z, t = threadIdx.x, DP = TB * 16;
    const int i = bi * 16 + (t >> 4), j = bj * 16 + (t & 15);
    if (i < D && j < D && i <= j) {                    // a diagonal block's lower half is the mirror image too: (r d_i) d_j and
        double s = 0.0;                                // (r d_j) d_i round differently, and s2 is exactly symmetric
        for (int sp = 0; sp < splits; ++sp) s += pouter[(((int64_t)sp * K + k) * NB + blockIdx.x) * 256 + t];
        double* o = s2 + (int64_t)k * D * D;
        o[(int64_t)i * D + j] = s;
        if (i != j) o[(int64_t)j * D + i] = s;
    }
    if (blockIdx.x != 0) return;
    if (t < D) {
        double s = 0.0;
        for (int sp = 0; sp < splits; ++sp) s += psum[((int64_t)sp * K + k) * DP + t];
        s1[(int64_t)k * D + t] = s;
    }
    if (t == 255) {
        double s = 0.0;
        for (int sp = 0; sp < splits; ++sp) s += pnk[(int64_t)sp * K + k];
        nk[k] = s;
        if (k == 0 && loglik_sum) {
            double l = 0.0;
            for (int sp = 0; sp < splits; ++sp) l += pll[sp];
            loglik_sum[0] = l;
        }
    }
}

// ---- sampling --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double u01_word(uint32_t w) { return (double)((float)(w >> 8) * 5.9604644775390625e-08f); }

// one workgroup per draw j (grid-stride): the component and the row's eps go through LDS, then one thread per output column
template <int DT>
__global__ __launch_bounds__(256) void gmm_sample_kernel(const double* __restrict__ cdf, const double* __restrict__ mean,
                                                         const double* __restrict__ chol, int K, int D, int64_t n, int W,
                                                         const double* __restrict__ u, const float* __restrict__ eps,
                                                         const unsigned long long* __restrict__ rng, int32_t* __restrict__ comp,
                                                         float* __restrict__ z32, void* __restrict__ z) {
    __shared__ double se[kMaxD];
    __shared__ int sk;
    const unsigned long long seed = rng ? rng[0] : 0ull, step = rng ? rng[1] : 0ull;
    const int t = threadIdx.x;
    for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
        __syncthreads();
        for (int c = t; c < D; c += 256)
            se[c] = (double)(eps ? eps[j * D + c] : philox_randn(seed, step, VG_DRAW_GMM_EPS, (unsigned long long)(j * D + c)));
        if (t == 0) {
            double uu;
            if (u) {
                uu = u[j];
            } else {
                uint32_t w[4];
                philox4x32_10(seed, step, VG_DRAW_GMM_U, (unsigned long long)j >> 2, w);
                const uint32_t sel = (uint32_t)(j & 3);
                uu = u01_word(sel == 0 ? w[0] : sel == 1 ? w[1] : sel == 2 ? w[2] : w[3]);
            }
            int k = 0;
            while (k < K - 1 && !(cdf[k] > uu)) ++k;                   // first k with cdf[k] > u, clamped to K - 1
            sk = k;
            if (comp) comp[j] = k;
        }
        __syncthreads();
        const int k = sk;
        const double* Lk = chol + (int64_t)k * D * D;
        for (int i = t; i < W; i += 256) {
            float v = 0.f;
            if (i < D) {
                const double* row = Lk + (int64_t)i * D;
                double acc = 0.0;
                for (int c = 0; c <= i; ++c) acc = fma(row[c], se[c], acc);
                v = (float)(mean[(int64_t)k * D + i] + acc);
                if (z32) z32[j * D + i] = v;
            }
            if (z) store1<DT>(z, j * W + i, v);
        }
    }
}

}  // namespace

extern "C" int vg_gmm_log_resp(const float* x, int64_t N, int D, int64_t row_stride, int K, const double* mean,
                               const double* prec_chol, const double* log_coef, double* log_prob, double* log_norm,
                               double* resp, void* stream) {
    VG_CHECK_ARG(x && mean && prec_chol && log_coef && gmm_args_ok(N, D, K) && row_stride >= D, VG_EINVAL);
    VG_CHECK_ARG(log_prob || log_norm || resp, VG_EINVAL);
    VG_CHECK_ARG(aligned8(mean) && aligned8(prec_chol) && aligned8(log_coef) && aligned8(log_prob) && aligned8(log_norm) &&
                 aligned8(resp), VG_EALIGN);
    hipStream_t st = vg_stream(stream);
    const int RF = eresp_lds_bytes(4, D, K) <= kLdsBudget ? 4 : 2;     // 64 rows, or 32 where D and K are both large
    const int64_t lds = eresp_lds_bytes(RF, D, K);
    VG_CHECK_ARG(lds <= kLdsBudget, VG_EINVAL);                        // 52 992 bytes at D = 256, K = 64, RF = 2
    const int R = 16 * RF;
    const dim3 grid((unsigned)((N + R - 1) / R)), block(256);
    if (RF == 4)
        hipLaunchKernelGGL(gmm_log_resp_kernel<4>, grid, block, (size_t)lds, st, x, N, D, row_stride, K, mean, prec_chol,
                           log_coef, log_prob, log_norm, resp);
    else
        hipLaunchKernelGGL(gmm_log_resp_kernel<2>, grid, block, (size_t)lds, st, x, N, D, row_stride, K, mean, prec_chol,
                           log_coef, log_prob, log_norm, resp);
    return VG_LAUNCH_RC();
}

extern "C" int64_t vg_gmm_moments_ws_bytes(int64_t N, int D, int K) {
    if (!gmm_args_ok(N, D, K)) return VG_EINVAL;
    return mom_ws_doubles(mom_plan(N, D, K), K) * 8;
}

extern "C" int vg_gmm_moments(const float* x, int64_t N, int D, int64_t row_stride, int K, const double* shift,
                              const double* resp, const double* log_norm, double* nk, double* s1, double* s2,
                              double* loglik_sum, void* ws, int64_t ws_bytes, void* stream) {
    VG_CHECK_ARG(x && shift && resp && nk && s1 && s2 && ws && gmm_args_ok(N, D, K) && row_stride >= D, VG_EINVAL);
    VG_CHECK_ARG(loglik_sum == nullptr || log_norm != nullptr, VG_EINVAL);
    VG_CHECK_ARG(ws_bytes >= vg_gmm_moments_ws_bytes(N, D, K), VG_EINVAL);
    VG_CHECK_ARG(aligned8(shift) && aligned8(resp) && aligned8(log_norm) && aligned8(nk) && aligned8(s1) && aligned8(s2) &&
                 aligned8(loglik_sum) && aligned8(ws), VG_EALIGN);
    const MomPlan p = mom_plan(N, D, K);
    double* pouter = static_cast<double*>(ws);
    double* psum = pouter + (int64_t)p.splits * K * p.NB * 256;
    double* pnk = psum + (int64_t)p.splits * K * p.TB * 16;
    double* pll = pnk + (int64_t)p.splits * K;
    hipStream_t st = vg_stream(stream);
    hipLaunchKernelGGL(gmm_moments_kernel, dim3(p.chunks, p.splits, K), dim3(256), (size_t)mom_lds_bytes(D), st, x, N, D,
                       row_stride, K, shift, resp, loglik_sum ? log_norm : nullptr, p.rows_per_split, p.TB, p.NB, pouter,
                       psum, pnk, pll);
    hipLaunchKernelGGL(gmm_moments_reduce_kernel, dim3(p.NB, 1, K), dim3(256), 0, st, pouter, psum, pnk, pll, p.splits, D,
                       K, p.TB, p.NB, nk, s1, s2, loglik_sum);
    return VG_LAUNCH_RC();
}

extern "C" int vg_gmm_sample(const double* cdf, const double* mean, const double* cov_chol, int K, int D, int64_t n,
                             const double* u, const float* eps, const uint64_t* rng, int32_t* comp, float* z32, void* z,
                             int ZP, int dtype, void* stream) {
    VG_CHECK_ARG(cdf && mean && cov_chol && K >= 1 && K <= kMaxK && D >= 1 && D <= kMaxD && n >= 1 && n <= 2147483647ll,
                 VG_EINVAL);
    VG_CHECK_ARG(comp || z32 || z, VG_EINVAL);
    VG_CHECK_ARG(rng || (u && eps), VG_EINVAL);                        // whatever is not injected needs the generator
    int W = D;
    if (z) {
        VG_CHECK_ARG(dtype == VG_F32 || dtype == VG_BF16, VG_ENOSUP);
        VG_CHECK_ARG(ZP >= D, VG_EINVAL);
        VG_CHECK_ARG(vg_aligned16(z), VG_EALIGN);
        W = ZP;
    } else {
        dtype = VG_F32;
    }
    VG_CHECK_ARG(aligned8(cdf) && aligned8(mean) && aligned8(cov_chol) && aligned8(u), VG_EALIGN);
    const dim3 grid((unsigned)(n < 65535 ? n : 65535)), block(256);
    hipStream_t st = vg_stream(stream);
    const unsigned long long* r = reinterpret_cast<const unsigned long long*>(rng);
    if (dtype == VG_F32)
        hipLaunchKernelGGL(gmm_sample_kernel<VG_F32>, grid, block, 0, st, cdf, mean, cov_chol, K, D, n, W, u, eps, r, comp,
                           z32, z);
    else
        hipLaunchKernelGGL(gmm_sample_kernel<VG_BF16>, grid, block, 0, st, cdf, mean, cov_chol, K, D, n, W, u, eps, r, comp,
                           z32, z);
    return VG_LAUNCH_RC();
}
