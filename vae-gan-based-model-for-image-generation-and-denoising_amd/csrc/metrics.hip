// Feature-space generation metrics (vaegan_code.py:143-185 / gan_code.py:111-145 / main_vae.py:472-512: fid.update /
// fid.compute; README.md:22: precision / recall "via manifold distances", Kynkaanniemi et al. 2019): everything AFTER a
// feature vector exists.  The contracts are stated in include/vaegan_hip.h, "Feature-space metrics".
//   vg_feat_stats_accum  f64 running sums: sum += column sums, outer += X^T X, on v_mfma_f64_16x16x4_f64
//   vg_knn_radius2       k-th smallest squared distance of every row to the OTHER rows, on v_mfma_f32_16x16x4_f32
//   vg_manifold_cover    is a query row inside some reference row's k-NN ball, same distance engine
// The N x N distance matrix never exists: a workgroup owns 128 query rows, walks the reference rows 64 at a time, and keeps
// each row's running k smallest (or its "inside" bit) in registers.
#include <math.h>
#include "common.hpp"

typedef __attribute__((ext_vector_type(4))) double f64x4;

namespace {

// ---- f64 statistics --------------------------------------------------------------------------------------------------
constexpr int kFT = 64;          // outer-product tile: 64 x 64 columns per workgroup, 32 x 32 per wave
constexpr int kFK = 32;          // rows staged per step
constexpr int kFS = 80;          // LDS row stride in floats: the 4 rows a wave reads at once fall 16 banks apart
constexpr int kFTargetWgs = 512; // workgroups a launch aims at when it splits the rows
constexpr int kMaxD = 2048;

struct StatPlan {
    int T, P, splits, rows_per_split;
};

StatPlan stat_plan(int64_t n, int D) {
    StatPlan p;
    p.T = (D + kFT - 1) / kFT;
    p.P = p.T * (p.T + 1) / 2;                       // upper triangle of tiles, the diagonal included
    int64_t s = kFTargetWgs / p.P;
    if (s < 1) s = 1;
    const int64_t most = (n + 2 * kFK - 1) / (2 * kFK);        // at least 64 rows per split
    if (s > most) s = most;
    if (s < 1) s = 1;
    int64_t rps = (n + s - 1) / s;
    rps = (rps + kFK - 1) / kFK * kFK;
    if (rps < kFK) rps = kFK;
    p.rows_per_split = (int)rps;
    p.splits = (int)((n + rps - 1) / rps);
    if (p.splits < 1) p.splits = 1;
    return p;
}

bool stat_args_ok(int64_t n, int D) { return n >= 0 && n <= 2147483647ll && D >= 1 && D <= kMaxD; }

__device__ __forceinline__ void pair_tiles(int p, int T, int& ti, int& tj) {
    ti = 0;
    while (p >= T - ti) { p -= T - ti; ++ti; }
    tj = ti + p;
}

// grid (tile pairs ti <= tj, row splits).  The MFMA's "k" runs over the rows of x: A[i][k] = x[r + k][ci + i],
// B[k][j] = x[r + k][cj + j], both converted exactly to f64; rows past the split and columns past D are staged as 0.
__global__ __launch_bounds__(256) void feat_stats_kernel(const float* __restrict__ x, int64_t n, int D, int64_t stride,
                                                         int rows_per_split, int T, int P, double* __restrict__ pouter,
                                                         double* __restrict__ psum) {
    __shared__ float si[kFK][kFS], sj[kFK][kFS];
    int ti, tj;
    pair_tiles(blockIdx.x, T, ti, tj);
    const bool diag = ti == tj;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_split;
    int64_t r1 = r0 + rows_per_split;
    if (r1 > n) r1 = n;
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    double csum = 0.0;
    const int lc = t & 63, lr = t >> 6;                               // staging: column lc, rows lr, lr + 4, ...
    const int ci = ti * kFT + lc, cj = tj * kFT + lc;
    const float (*sb)[kFS] = diag ? si : sj;
    for (int64_t r = r0; r < r1; r += kFK) {
#pragma unroll
        for (int q = 0; q < kFK / 4; ++q) {
            const int64_t row = r + lr + 4 * q;
            const bool in = row < r1;
            si[lr + 4 * q][lc] = (in && ci < D) ? x[row * stride + ci] : 0.f;
            if (!diag) sj[lr + 4 * q][lc] = (in && cj < D) ? x[row * stride + cj] : 0.f;
        }
        __syncthreads();
        if (diag && t < kFT) {
#pragma unroll 8
            for (int k = 0; k < kFK; ++k) csum += (double)si[k][t];   // row order: the sum's order is fixed
        }
#pragma unroll
        for (int kk = 0; kk < kFK; kk += 4) {
            const int k = kk + (lane >> 4), c = lane & 15;
            const double a0 = (double)si[k][32 * wi + c], a1 = (double)si[k][32 * wi + 16 + c];
            const double b0 = (double)sb[k][32 * wj + c], b1 = (double)sb[k][32 * wj + 16 + c];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
    double* out = pouter + ((int64_t)blockIdx.y * P + blockIdx.x) * (kFT * kFT);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = 32 * wi + 16 * a + (lane >> 4) + 4 * g, j = 32 * wj + 16 * b + (lane & 15);
                out[i * kFT + j] = acc[a][b][g];
            }
    if (diag && t < kFT) psum[(int64_t)blockIdx.y * T * kFT + ti * kFT + t] = csum;
}

// grid (tile pairs, 16): the splits' partials are added in split order, then added to outer (and to its mirror image)
__global__ __launch_bounds__(256) void feat_stats_reduce_kernel(const double* __restrict__ pouter,
                                                                const double* __restrict__ psum, int splits, int D, int T,
                                                                int P, double* __restrict__ sum, double* __restrict__ outer) {
    int ti, tj;
    pair_tiles(blockIdx.x, T, ti, tj);
    const int e = blockIdx.y * 256 + threadIdx.x;
    const int li = e / kFT, lj = e - li * kFT;
    const int i = ti * kFT + li, j = tj * kFT + lj;
    if (i < D && j < D) {
        double s = 0.0;
        for (int sp = 0; sp < splits; ++sp) s += pouter[((int64_t)sp * P + blockIdx.x) * (kFT * kFT) + e];
        outer[(int64_t)i * D + j] += s;
        if (ti != tj) outer[(int64_t)j * D + i] += s;
    }
    if (ti == tj && blockIdx.y == 0 && threadIdx.x < kFT) {
        const int c = ti * kFT + threadIdx.x;
        if (c < D) {
            double s = 0.0;
            for (int sp = 0; sp < splits; ++sp) s += psum[(int64_t)sp * T * kFT + c];
            sum[c] += s;
        }
    }
}

// ---- pairwise squared distances ----------------------------------------------------------------------------------------
constexpr int kRA = 2;                 // 16-row A fragments per wave
constexpr int kDM = 64 * kRA;          // query rows per workgroup (4 waves x 16 * kRA)
constexpr int kDN = 64;                // reference rows per step
constexpr int kDK = 32;                // feature columns staged per step
constexpr int kDS = 36;                // LDS row stride in floats: 16 rows x 4 adjacent k, conflict-free
constexpr int kMaxK = 8;
constexpr int kMaxSplits = 16;
constexpr int kDTargetWgs = 1024;

struct DistPlan {
    int row_tiles, col_tiles, splits, tiles_per_split;
};

DistPlan dist_plan(int64_t Nq, int64_t Nr) {
    DistPlan p;
    p.row_tiles = (int)((Nq + kDM - 1) / kDM);
    p.col_tiles = (int)((Nr + kDN - 1) / kDN);
    int s = (kDTargetWgs + p.row_tiles - 1) / p.row_tiles;
    if (s > kMaxSplits) s = kMaxSplits;
    if (s > p.col_tiles) s = p.col_tiles;
    if (s < 1) s = 1;
    p.tiles_per_split = (p.col_tiles + s - 1) / s;
    p.splits = (p.col_tiles + p.tiles_per_split - 1) / p.tiles_per_split;
    return p;
}

bool dist_args_ok(int64_t Nq, int64_t Nr, int D) {
    return Nq >= 1 && Nr >= 1 && Nq <= (1ll << 24) && Nr <= (1ll << 24) && D >= 1 && D <= kMaxD;
}

// |x_r|^2 in f32: one wavefront per row, a fused multiply-add chain per lane, then the wave tree
__global__ __launch_bounds__(256) void row_norm2_kernel(const float* __restrict__ x, int64_t N, int D,
                                                        float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) {
        const float v = x[row * D + c];
        s = fmaf(v, v, s);
    }
    s = wave_sum(s);
    if (lane == 0) out[row] = s;
}

template <int KM>
__device__ __forceinline__ void topk_insert(float (&best)[KM], float v) {
#pragma unroll
    for (int s = 0; s < KM; ++s) {
        const float lo = fminf(best[s], v);
        v = fmaxf(best[s], v);
        best[s] = lo;
    }
}

// MODE 0 (k nearest): q == ref, column j == row i is skipped by INDEX; part[split][row][k] = the k smallest d2 of the
// split's columns, ascending (+inf where the split holds fewer).  MODE 1 (cover): flag[split][row] = 1 where some column
// of the split has d2 <= r2ref[col].   d2 = max(0, (|a|^2 + |b|^2) - 2 * dot), dot on the exact-f32 MFMA.
template <int MODE, int KM>
__global__ __launch_bounds__(256) void dist_kernel(const float* __restrict__ q, const float* __restrict__ ref,
                                                   const float* __restrict__ nq, const float* __restrict__ nr,
                                                   const float* __restrict__ r2ref, int Nq, int Nr, int D, int k,
                                                   int tiles_per_split, int col_tiles, float* __restrict__ part,
                                                   int32_t* __restrict__ flag) {
    __shared__ __attribute__((aligned(16))) float sa[kDM][kDS], sb[kDN][kDS];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lq = lane >> 4, lc = lane & 15;
    const int row0 = blockIdx.x * kDM;
    const int wrow0 = row0 + wave * 16 * kRA;
    int ct0 = blockIdx.y * tiles_per_split, ct1 = ct0 + tiles_per_split;
    if (ct1 > col_tiles) ct1 = col_tiles;
    const bool vec = (D & 3) == 0;

    // this lane's rows: fragment a, accumulator register g -> wrow0 + 16 * a + 4 * lq + g
    float na[kRA][4];
    float best[kRA * 4][KM];
    int inside = 0;
#pragma unroll
    for (int a = 0; a < kRA; ++a)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int row = wrow0 + 16 * a + 4 * lq + g;
            na[a][g] = row < Nq ? nq[row] : 0.f;
#pragma unroll
            for (int s = 0; s < KM; ++s) best[a * 4 + g][s] = INFINITY;
        }

    for (int ct = ct0; ct < ct1; ++ct) {
        const int col0 = ct * kDN;
        f32x4 acc[kRA][4];
#pragma unroll
        for (int a = 0; a < kRA; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < D; k0 += kDK) {
            // stage a[kDM][32] and b[kDN][32]; rows past the matrix and columns past D are 0
            if (vec) {
                const int kq = (t & 7) * 4, rr = t >> 3;                  // 8 float4 per row, 32 rows per pass
                const bool kin = k0 + kq < D;
#pragma unroll
                for (int p = 0; p < kDM / 32; ++p) {
                    const int r = rr + 32 * p, row = row0 + r;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (kin && row < Nq) v = *reinterpret_cast<const float4*>(q + (int64_t)row * D + k0 + kq);
                    *reinterpret_cast<float4*>(&sa[r][kq]) = v;
                }
#pragma unroll
                for (int p = 0; p < kDN / 32; ++p) {
                    const int r = rr + 32 * p, row = col0 + r;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (kin && row < Nr) v = *reinterpret_cast<const float4*>(ref + (int64_t)row * D + k0 + kq);
                    *reinterpret_cast<float4*>(&sb[r][kq]) = v;
                }
            } else {
                const int kq = t & 31, rr = t >> 5;                       // 8 rows per pass
                const bool kin = k0 + kq < D;
#pragma unroll 4
                for (int p = 0; p < kDM / 8; ++p) {
                    const int r = rr + 8 * p, row = row0 + r;
                    sa[r][kq] = (kin && row < Nq) ? q[(int64_t)row * D + k0 + kq] : 0.f;
                }
#pragma unroll 4
                for (int p = 0; p < kDN / 8; ++p) {
                    const int r = rr + 8 * p, row = col0 + r;
                    sb[r][kq] = (kin && row < Nr) ? ref[(int64_t)row * D + k0 + kq] : 0.f;
                }
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kDK; kk += 4) {
                float av[kRA], bv[4];
#pragma unroll
                for (int a = 0; a < kRA; ++a) av[a] = sa[wave * 16 * kRA + 16 * a + lc][kk + lq];
#pragma unroll
                for (int b = 0; b < 4; ++b) bv[b] = sb[16 * b + lc][kk + lq];
#pragma unroll
                for (int a = 0; a < kRA; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc[a][b], 0, 0, 0);
            }
            __syncthreads();
        }
        // f32 C/D layout: col = lane & 15, row = 4 * (lane >> 4) + reg
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int col = col0 + 16 * b + lc;
            const bool cin = col < Nr;
            const float nb = cin ? nr[col] : 0.f;
            const float rad = (MODE == 1 && cin) ? r2ref[col] : 0.f;
#pragma unroll
            for (int a = 0; a < kRA; ++a)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float d2 = fmaxf(0.f, (na[a][g] + nb) - 2.f * acc[a][b][g]);
                    if (MODE == 0) {
                        const int row = wrow0 + 16 * a + 4 * lq + g;
                        const float v = (cin && col != row) ? d2 : INFINITY;
                        if (v < best[a * 4 + g][KM - 1]) topk_insert<KM>(best[a * 4 + g], v);
                    } else {
                        if (cin && d2 <= rad) inside |= 1 << (a * 4 + g);
                    }
                }
        }
    }

    // the 16 lanes that share lane >> 4 hold disjoint candidates of the same rows: butterfly over lane bits 0..3
    if (MODE == 0) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
            for (int r = 0; r < kRA * 4; ++r) {
                float other[KM];
#pragma unroll
                for (int s = 0; s < KM; ++s) other[s] = __shfl_xor(best[r][s], o);
#pragma unroll
                for (int s = 0; s < KM; ++s) topk_insert<KM>(best[r], other[s]);
            }
        }
        if (lc == 0) {
#pragma unroll
            for (int a = 0; a < kRA; ++a)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int row = wrow0 + 16 * a + 4 * lq + g;
                    if (row < Nq) {
                        float* dst = part + ((int64_t)blockIdx.y * Nq + row) * k;
#pragma unroll
                        for (int s = 0; s < KM; ++s)
                            if (s < k) dst[s] = best[a * 4 + g][s];
                    }
                }
        }
    } else {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) inside |= __shfl_xor(inside, o);
        if (lc == 0) {
#pragma unroll
            for (int a = 0; a < kRA; ++a)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int row = wrow0 + 16 * a + 4 * lq + g;
                    if (row < Nq) flag[(int64_t)blockIdx.y * Nq + row] = (inside >> (a * 4 + g)) & 1;
                }
        }
    }
}

// one thread per row: the k-th smallest of the splits' ascending lists
__global__ __launch_bounds__(256) void knn_merge_kernel(const float* __restrict__ part, int N, int k, int splits,
                                                        float* __restrict__ r2) {
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= N) return;
    float best[kMaxK];
#pragma unroll
    for (int s = 0; s < kMaxK; ++s) best[s] = INFINITY;
    for (int sp = 0; sp < splits; ++sp)
        for (int s = 0; s < k; ++s) topk_insert<kMaxK>(best, part[((int64_t)sp * N + row) * k + s]);
    float out = best[0];
#pragma unroll
    for (int s = 1; s < kMaxK; ++s)
        if (s == k - 1) out = best[s];
    r2[row] = out;
}

// OR over the splits; the count is an integer sum (order-independent)
__global__ __launch_bounds__(256) void cover_merge_kernel(const int32_t* __restrict__ flag, int N, int splits,
                                                          int32_t* __restrict__ inside, unsigned long long* __restrict__ count) {
    __shared__ int wsum[4];
    const int row = blockIdx.x * 256 + threadIdx.x;
    int f = 0;
    if (row < N) {
        for (int sp = 0; sp < splits; ++sp) f |= flag[(int64_t)sp * N + row];
        inside[row] = f;
    }
    int c = f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (tot) atomicAdd(count, (unsigned long long)tot);
    }
}

int64_t align256(int64_t b) { return (b + 255) / 256 * 256; }

}  // namespace

extern "C" int64_t vg_feat_stats_accum_ws_bytes(int64_t n, int D) {
    if (!stat_args_ok(n, D)) return VG_EINVAL;
    if (n == 0) return 0;
    const StatPlan p = stat_plan(n, D);
    return (int64_t)p.splits * ((int64_t)p.P * kFT * kFT + (int64_t)p.T * kFT) * 8;
}

extern "C" int vg_feat_stats_accum(const float* x, int64_t n, int D, int64_t row_stride, double* sum, double* outer,
                                   void* ws, int64_t ws_bytes, void* stream) {
    VG_CHECK_ARG(sum && outer && stat_args_ok(n, D) && row_stride >= D, VG_EINVAL);
    VG_CHECK_ARG((reinterpret_cast<uintptr_t>(sum) & 7u) == 0 && (reinterpret_cast<uintptr_t>(outer) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(ws) & 7u) == 0, VG_EALIGN);
    if (n == 0) return 0;
    VG_CHECK_ARG(x && ws && ws_bytes >= vg_feat_stats_accum_ws_bytes(n, D), VG_EINVAL);
    const StatPlan p = stat_plan(n, D);
    hipStream_t st = vg_stream(stream);
    double* pouter = static_cast<double*>(ws);
    double* psum = pouter + (int64_t)p.splits * p.P * kFT * kFT;
    hipLaunchKernelGGL(feat_stats_kernel, dim3(p.P, p.splits), dim3(256), 0, st, x, n, D, row_stride, p.rows_per_split, p.T,
                       p.P, pouter, psum);
    hipLaunchKernelGGL(feat_stats_reduce_kernel, dim3(p.P, kFT * kFT / 256), dim3(256), 0, st, pouter, psum, p.splits, D,
                       p.T, p.P, sum, outer);
    return VG_LAUNCH_RC();
}

extern "C" int64_t vg_knn_radius2_ws_bytes(int64_t N, int D, int k) {
    if (!dist_args_ok(N, N, D) || k < 1 || k > kMaxK || k >= N) return VG_EINVAL;
    const DistPlan p = dist_plan(N, N);
    return align256(N * 4) + (int64_t)p.splits * N * k * 4;
}

extern "C" int vg_knn_radius2(const float* x, int64_t N, int D, int k, float* r2, void* ws, int64_t ws_bytes, void* stream) {
    VG_CHECK_ARG(x && r2 && ws && dist_args_ok(N, N, D) && k >= 1 && k <= kMaxK && k < N, VG_EINVAL);
    VG_CHECK_ARG(ws_bytes >= vg_knn_radius2_ws_bytes(N, D, k), VG_EINVAL);
    VG_CHECK_ARG(vg_aligned16(x) && vg_aligned16(ws), VG_EALIGN);
    const DistPlan p = dist_plan(N, N);
    hipStream_t st = vg_stream(stream);
    float* norms = static_cast<float*>(ws);
    float* part = reinterpret_cast<float*>(static_cast<char*>(ws) + align256(N * 4));
    const int n = (int)N;
    hipLaunchKernelGGL(row_norm2_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, x, N, D, norms);
    const dim3 grid(p.row_tiles, p.splits);
    if (k == 1)
        hipLaunchKernelGGL((dist_kernel<0, 1>), grid, dim3(256), 0, st, x, x, norms, norms, (const float*)nullptr, n, n, D, k,
                           p.tiles_per_split, p.col_tiles, part, (int32_t*)nullptr);
    else if (k <= 4)
        hipLaunchKernelGGL((dist_kernel<0, 4>), grid, dim3(256), 0, st, x, x, norms, norms, (const float*)nullptr, n, n, D, k,
                           p.tiles_per_split, p.col_tiles, part, (int32_t*)nullptr);
    else
        hipLaunchKernelGGL((dist_kernel<0, 8>), grid, dim3(256), 0, st, x, x, norms, norms, (const float*)nullptr, n, n, D, k,
                           p.tiles_per_split, p.col_tiles, part, (int32_t*)nullptr);
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, part, n, k, p.splits, r2);
    return VG_LAUNCH_RC();
}

extern "C" int64_t vg_manifold_cover_ws_bytes(int64_t Nq, int64_t Nr, int D) {
    if (!dist_args_ok(Nq, Nr, D)) return VG_EINVAL;
    const DistPlan p = dist_plan(Nq, Nr);
    return align256(Nq * 4) + align256(Nr * 4) + (int64_t)p.splits * Nq * 4;
}

extern "C" int vg_manifold_cover(const float* q, int64_t Nq, const float* ref, int64_t Nr, int D, const float* r2_ref,
                                 int32_t* inside, int64_t* count, void* ws, int64_t ws_bytes, void* stream) {
    VG_CHECK_ARG(q && ref && r2_ref && inside && count && ws && dist_args_ok(Nq, Nr, D), VG_EINVAL);
    VG_CHECK_ARG(ws_bytes >= vg_manifold_cover_ws_bytes(Nq, Nr, D), VG_EINVAL);
    VG_CHECK_ARG(vg_aligned16(q) && vg_aligned16(ref) && vg_aligned16(ws) &&
                 (reinterpret_cast<uintptr_t>(count) & 7u) == 0, VG_EALIGN);
    const DistPlan p = dist_plan(Nq, Nr);
    hipStream_t st = vg_stream(stream);
    char* w = static_cast<char*>(ws);
    float* nq = reinterpret_cast<float*>(w);
    float* nr = reinterpret_cast<float*>(w + align256(Nq * 4));
    int32_t* flag = reinterpret_cast<int32_t*>(w + align256(Nq * 4) + align256(Nr * 4));
    hipError_t e = hipMemsetAsync(count, 0, 8, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(row_norm2_kernel, dim3((unsigned)((Nq + 3) / 4)), dim3(256), 0, st, q, Nq, D, nq);
    hipLaunchKernelGGL(row_norm2_kernel, dim3((unsigned)((Nr + 3) / 4)), dim3(256), 0, st, ref, Nr, D, nr);
    hipLaunchKernelGGL((dist_kernel<1, 1>), dim3(p.row_tiles, p.splits), dim3(256), 0, st, q, ref, nq, nr, r2_ref, (int)Nq,
                       (int)Nr, D, 1, p.tiles_per_split, p.col_tiles, (float*)nullptr, flag);
    hipLaunchKernelGGL(cover_merge_kernel, dim3((unsigned)((Nq + 255) / 256)), dim3(256), 0, st, flag, (int)Nq, p.splits,
                       inside, reinterpret_cast<unsigned long long*>(count));
    return VG_LAUNCH_RC();
}
