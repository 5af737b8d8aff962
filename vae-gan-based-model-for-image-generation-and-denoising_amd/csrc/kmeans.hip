// K-means over feature or latent rows that already sit in HBM: Lloyd's two phases and the k-means++ seeding.  The
// contracts are stated in include/vaegan_hip.h, "K-means".
//   vg_kmeans_assign   per row the nearest centre: the N x K x D product x . c on v_mfma_f64_16x16x4_f64, the running
//                      (min, argmin) in registers, the lowest k on a tie; direct-form dist2, one-hot resp, changed count
//   vg_kmeans_update   count, sum and centre per cluster from the labels over a FIXED row split (one thread per column,
//                      rows in ascending order, one LDS cell per (cluster, column)); the splits' partials are added in
//                      split order by a second launch, the two scalars of stats by a third, tiny one
//   vg_kmeans_seed     plain k-means++ with no host sync: per step a mind2 update with block totals, then a pick
//   vg_kmeans_plan     the record all of the above launch from, as a host-only query
#include <math.h>
#include "common.hpp"
#include "noise.hpp"

typedef __attribute__((ext_vector_type(4))) double f64x4;

namespace {

constexpr int kMaxD = 256;
constexpr int kMaxK = 1024;
constexpr int kLdsBudget = 65536;
constexpr int kUpdAccBytes = 49152;   // LDS of the update's accumulators: chunk * D * 8 bytes
constexpr int kUpdMinCap = 128;       // splits: at most max(128, 16 MiB of partial sums), never more than 1024
constexpr int kUpdMaxSplits = 1024;
constexpr int64_t kUpdPartialBytes = 16ll << 20;
constexpr int kUpdTargetWgs = 1024;
constexpr int kUpdRows = 256;         // labels staged per step; rows_per_split is a multiple
constexpr int kSeedBlock = 256;       // rows per block of the seed's two-level cumulative sum

bool km_args_ok(int64_t N, int D, int K) {
    return N >= 1 && N <= 2147483647ll && D >= 1 && D <= kMaxD && K >= 1 && K <= kMaxK;
}
bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

int64_t assign_lds_bytes(int RF, int D) {
    const int R = 16 * RF, XS = ((D + 15) & ~15) + 4;
    return (int64_t)R * (52 + 4 * XS) + 16;
}

// The one record the launchers launch from; vg_kmeans_plan hands it out.
vg_km_plan km_plan(int64_t N, int D, int K) {
    vg_km_plan p;
    const int RF = assign_lds_bytes(4, D) <= kLdsBudget ? 4 : 2;       // 64 rows, 32 where D > 224
    p.assign_rows = 16 * RF;
    p.assign_tile = 16;
    p.assign_row_split = (RF == 4 && (K + 15) / 16 < 4) ? 1 : 0;       // fewer than four centre tiles: the waves split the rows
    p.assign_lds_bytes = (int32_t)assign_lds_bytes(RF, D);
    p.assign_grid = (N + p.assign_rows - 1) / p.assign_rows;
    int ch = kUpdAccBytes / (8 * D);
    if (ch > K) ch = K;
    p.update_chunk = ch;
    p.update_chunks = (K + ch - 1) / ch;
    int64_t s = kUpdTargetWgs / p.update_chunks;
    int64_t cap = kUpdPartialBytes / ((int64_t)8 * K * D);
    if (cap < kUpdMinCap) cap = kUpdMinCap;
    if (cap > kUpdMaxSplits) cap = kUpdMaxSplits;
    if (s > cap) s = cap;
    const int64_t most = (N + kUpdRows - 1) / kUpdRows;
    if (s > most) s = most;
    if (s < 1) s = 1;
    int64_t rps = (N + s - 1) / s;
    rps = (rps + kUpdRows - 1) / kUpdRows * kUpdRows;
    p.update_rows_per_split = rps;
    p.update_splits = (int32_t)((N + rps - 1) / rps);
    p.seed_block = kSeedBlock;
    p.seed_blocks = (N + kSeedBlock - 1) / kSeedBlock;
    p.update_ws_bytes = 8 * ((int64_t)p.update_splits * ((int64_t)K * D + K + 1) + K);
    p.seed_ws_bytes = 8 * (N + p.seed_blocks);
    return p;
}

// ---- assignment --------------------------------------------------------------------------------------------------------
// A workgroup owns R = 16 * RF rows; its x tile sits in LDS as f32 [R][DP + 4], DP = D rounded up to 16, pad columns and
// rows past N zero, for all K centres.  Centre tile jt holds centres 16 jt .. 16 jt + 15.  !ROWSPLIT: the four waves share
// the rows and take the tiles wave, wave + 4, ...; ROWSPLIT (fewer than four tiles): wave w owns rows 16 w .. 16 w + 15
// and walks every tile.  MFMA operands: A[row][i] = (double)x, row = lane & 15; B[i][col] = c[16 jt + col][i], col =
// lane & 15, from global memory (the centres stay in L2): a lane loads the FOUR consecutive doubles i0 + 4 (lane >> 4) + s
// of its centre per 16 columns, one group ahead of the MFMAs, so MFMA step s of a group carries column i0 + 4 q + s on
// k-index q for both operands.  The same loads give h: per lane the sum of its squares, then the four lanes of a centre by
// xor shuffles.  C/D: col = lane & 15, row = (lane >> 4) + 4 * reg.
template <int RF, bool ROWSPLIT>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ x, int64_t N, int D, int64_t stride,
                                                            int K, const double* __restrict__ center,
                                                            int32_t* __restrict__ label, double* __restrict__ dist2,
                                                            double* __restrict__ resp, const int32_t* __restrict__ prev,
                                                            int32_t* __restrict__ changed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int R = 16 * RF;
    constexpr int FW = ROWSPLIT ? 1 : RF;
    constexpr int LPR = 256 / R;                       // lanes per row of the dist2 pass
    const int DP = (D + 15) & ~15, XS = DP + 4, KT = (K + 15) >> 4;
    double* sbest = reinterpret_cast<double*>(smem);   // [4][R] the waves' candidates
    int* sarg = reinterpret_cast<int*>(sbest + 4 * R); // [4][R]
    int* slab = sarg + 4 * R;                          // [R]    the labels
    int* schg = slab + R;                              // [4]    changed rows of this workgroup
    float* sx = reinterpret_cast<float*>(schg + 4);    // [R][XS]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int lc = lane & 15, lq = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * R;

    for (int e = t; e < R * DP; e += 256) {
        const int r = e / DP, c = e - r * DP;
        const int64_t row = row0 + r;
        sx[r * XS + c] = (row < N && c < D) ? x[row * stride + c] : 0.f;
    }
    if (t == 0) schg[0] = 0;
    __syncthreads();

    const int fb = ROWSPLIT ? wave : 0;
    double best[FW][4];
    int bk[FW][4];
#pragma unroll
    for (int f = 0; f < FW; ++f)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            best[f][g] = INFINITY;
            bk[f][g] = 0;
        }
    for (int jt = ROWSPLIT ? 0 : wave; jt < KT; jt += ROWSPLIT ? 1 : 4) {
        const int k = jt * 16 + lc;
        const bool kin = k < K;
        const double* ck = center + (int64_t)(kin ? k : 0) * D;
        f64x4 acc[FW];
#pragma unroll
        for (int f = 0; f < FW; ++f) acc[f] = f64x4{0.0, 0.0, 0.0, 0.0};
        double hp = 0.0;
        double bn[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) bn[s] = (kin && 4 * lq + s < D) ? ck[4 * lq + s] : 0.0;
        for (int i0 = 0; i0 < DP; i0 += 16) {
            const int i = i0 + 4 * lq;
            double b[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) b[s] = bn[s];
            if (i0 + 16 < DP) {                                        // in flight while this group's MFMAs run
#pragma unroll
                for (int s = 0; s < 4; ++s) bn[s] = (kin && i + 16 + s < D) ? ck[i + 16 + s] : 0.0;
            }
            float a[FW][4];
#pragma unroll
            for (int f = 0; f < FW; ++f) {
                const float4 v = *reinterpret_cast<const float4*>(sx + (16 * (fb + f) + lc) * XS + i);
                a[f][0] = v.x; a[f][1] = v.y; a[f][2] = v.z; a[f][3] = v.w;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
#pragma unroll
                for (int f = 0; f < FW; ++f)
                    acc[f] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)a[f][s], b[s], acc[f], 0, 0, 0);
                hp = fma(b[s], b[s], hp);
            }
        }
        hp += __shfl_xor(hp, 16);
        hp += __shfl_xor(hp, 32);
        const double h = 0.5 * hp;
#pragma unroll
        for (int f = 0; f < FW; ++f)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const double s = h - acc[f][g];
                if (kin && s < best[f][g]) {                            // strict: the lowest k of this lane stays
                    best[f][g] = s;
                    bk[f][g] = k;
                }
            }
    }
    // the 16 lanes of a row, then the waves: the smaller score, on a tie the lower k
#pragma unroll
    for (int f = 0; f < FW; ++f)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            double v = best[f][g];
            int kk = bk[f][g];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) {
                const double ov = __shfl_xor(v, o);
                const int ok = __shfl_xor(kk, o);
                if (ov < v || (ov == v && ok < kk)) {
                    v = ov;
                    kk = ok;
                }
            }
            if (lc == 0) {
                const int r = 16 * (fb + f) + lq + 4 * g;
                sbest[wave * R + r] = v;
                sarg[wave * R + r] = kk;
            }
        }
    __syncthreads();
    const int64_t left = N - row0;
    const int nrows = left < R ? (int)left : R;
    if (t < R) {
        double v;
        int kk;
        if (ROWSPLIT) {
            v = sbest[(t >> 4) * R + t];
            kk = sarg[(t >> 4) * R + t];
        } else {
            v = sbest[t];
            kk = sarg[t];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const double ov = sbest[w * R + t];
                const int ok = sarg[w * R + t];
                if (ov < v || (ov == v && ok < kk)) {
                    v = ov;
                    kk = ok;
                }
            }
        }
        slab[t] = kk;
        if (t < nrows) {
            if (label) label[row0 + t] = kk;
            if (changed && prev[row0 + t] != kk) atomicAdd(&schg[0], 1);
        }
    }
    __syncthreads();
    if (changed && t == 0 && schg[0] > 0) atomicAdd(changed, schg[0]);
    if (dist2) {
        const int r = t / LPR, q = t - r * LPR;
        const double* c = center + (int64_t)slab[r] * D;
        double p = 0.0;
        for (int i = q; i < D; i += LPR) {
            const double d = (double)sx[r * XS + i] - c[i];
            p = fma(d, d, p);
        }
#pragma unroll
        for (int o = 1; o < LPR; o <<= 1) p += __shfl_xor(p, o);
        if (q == 0 && r < nrows) dist2[row0 + r] = p;
    }
    if (resp) {
        for (int e = t; e < nrows * K; e += 256) {
            const int r = e / K, k = e - r * K;
            resp[row0 * K + e] = slab[r] == k ? 1.0 : 0.0;
        }
    }
}

// ---- update ------------------------------------------------------------------------------------------------------------
// grid (splits, chunks): a workgroup owns the rows [r0, r1) of its split and the clusters [k0, k0 + ch) of its chunk.  The
// labels go through LDS 256 at a time; thread i owns column i and walks the staged rows in ascending order, adding x[n][i]
// into its own cell acc[label - k0][i] -- no two threads share a cell, and only the chunk that owns a row's label reads
// that row of x.  A label outside [0, K) belongs to no chunk.  Counts: integer LDS atomics.  Chunk 0 also adds the split's
// dist2: thread t the rows r0 + t + 256 j, j ascending, then a halving tree over the 256 threads.
__global__ __launch_bounds__(256) void kmeans_update_kernel(const float* __restrict__ x, int64_t N, int D, int64_t stride,
                                                            int K, const int32_t* __restrict__ label,
                                                            const double* __restrict__ dist2, int64_t rows_per_split, int CH,
                                                            int want_sum, double* __restrict__ psum,
                                                            int64_t* __restrict__ pcnt, double* __restrict__ pd2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* acc = reinterpret_cast<double*>(smem);     // [CH][D]
    double* sred = acc + (int64_t)CH * D;              // [256]
    int* scnt = reinterpret_cast<int*>(sred + 256);    // [CH]
    int* slab = scnt + CH;                             // [256]
    const int t = threadIdx.x;
    const int k0 = blockIdx.y * CH;
    const int ch = K - k0 < CH ? K - k0 : CH;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_split;
    int64_t r1 = r0 + rows_per_split;
    if (r1 > N) r1 = N;
    for (int e = t; e < ch * D; e += 256) acc[e] = 0.0;
    for (int e = t; e < ch; e += 256) scnt[e] = 0;
    __syncthreads();
    for (int64_t r = r0; r < r1; r += kUpdRows) {
        int l = -1;
        if (r + t < r1) {
            const int lab = label[r + t];
            if (lab >= k0 && lab < k0 + ch) l = lab - k0;
        }
        slab[t] = l;
        if (l >= 0) atomicAdd(&scnt[l], 1);
        __syncthreads();
        if (want_sum && t < D) {
            const int64_t rem = r1 - r;
            const int nr = rem < kUpdRows ? (int)rem : kUpdRows;
            const float* xr = x + r * stride + t;
            for (int b = 0; b < nr; b += 8) {
                float v[8];
                int li[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    li[u] = b + u < nr ? slab[b + u] : -1;
                    v[u] = li[u] >= 0 ? xr[(int64_t)(b + u) * stride] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (li[u] >= 0) acc[li[u] * D + t] += (double)v[u];
            }
        }
        __syncthreads();
    }
    const int64_t base = (int64_t)blockIdx.x * K + k0;
    if (want_sum)
        for (int e = t; e < ch * D; e += 256) psum[base * D + e] = acc[e];
    for (int e = t; e < ch; e += 256) pcnt[base + e] = scnt[e];
    if (blockIdx.y == 0 && dist2 != nullptr) {
        double p = 0.0;
        for (int64_t n = r0 + t; n < r1; n += 256) p += dist2[n];
        sred[t] = p;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) sred[t] += sred[t + o];
            __syncthreads();
        }
        if (t == 0) pd2[blockIdx.x] = sred[0];
    }
}

// grid (K): the splits' partials of cluster k are added in split order; one IEEE division per centre element; the
// cluster's share of stats[0], columns ascending, goes to pshift[k].  The partials of 16 splits at a time go through LDS
// (all 256 threads load, the next 16 already in registers), then thread i adds column i's 16 values in split order: with
// up to 1024 splits a chain of dependent loads per column would be the whole cost.  The counts are integers: any order.
constexpr int kRedSplits = 16;
__global__ __launch_bounds__(256) void kmeans_update_reduce_kernel(const double* __restrict__ psum,
                                                                   const int64_t* __restrict__ pcnt, int splits, int D, int K,
                                                                   int want_sum, const double* __restrict__ old,
                                                                   int64_t* __restrict__ count, double* __restrict__ sum,
                                                                   double* __restrict__ center, double* __restrict__ pshift) {
    __shared__ double sdiff[kMaxD];
    __shared__ double tile[kRedSplits * kMaxD];
    __shared__ int64_t scnt[256];
    const int k = blockIdx.x, t = threadIdx.x;
    int64_t c = 0;
    for (int sp = t; sp < splits; sp += 256) c += pcnt[(int64_t)sp * K + k];
    scnt[t] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) scnt[t] += scnt[t + o];
        __syncthreads();
    }
    const int64_t cnt = scnt[0];
    double s = 0.0;
    if (want_sum) {
        const int TE = kRedSplits * D;                                  // elements of a tile, [split][column]
        double pf[kRedSplits];
        auto fetch = [&](int sp0) {
#pragma unroll
            for (int u = 0; u < kRedSplits; ++u) {
                const int e = t + 256 * u;
                const int sp = e / D, i = e - sp * D;
                pf[u] = (e < TE && sp0 + sp < splits) ? psum[((int64_t)(sp0 + sp) * K + k) * D + i] : 0.0;
            }
        };
        fetch(0);
        for (int sp0 = 0; sp0 < splits; sp0 += kRedSplits) {
            __syncthreads();                                            // the previous tile has been added
#pragma unroll
            for (int u = 0; u < kRedSplits; ++u) {
                const int e = t + 256 * u;
                if (e < TE) tile[e] = pf[u];
            }
            __syncthreads();
            if (sp0 + kRedSplits < splits) fetch(sp0 + kRedSplits);
            if (t < D) {
                const int n = splits - sp0 < kRedSplits ? splits - sp0 : kRedSplits;
                for (int sp = 0; sp < n; ++sp) s += tile[sp * D + t];
            }
        }
    }
    if (want_sum && t < D) {
        if (sum) sum[(int64_t)k * D + t] = s;
        if (center) {
            const double o = old[(int64_t)k * D + t];
            const double c = cnt > 0 ? s / (double)cnt : o;
            center[(int64_t)k * D + t] = c;
            const double d = c - o;
            sdiff[t] = d * d;
        }
    }
    __syncthreads();
    if (t == 0) {
        count[k] = cnt;
        double s = 0.0;
        if (center)
            for (int i = 0; i < D; ++i) s += sdiff[i];
        pshift[k] = s;
    }
}

// one workgroup: stats[0] = the clusters' shares in k order, stats[1] = the splits' dist2 sums in split order
__global__ __launch_bounds__(256) void kmeans_update_stats_kernel(const double* __restrict__ pshift, int K,
                                                                  const double* __restrict__ pd2, int splits,
                                                                  double* __restrict__ stats) {
    __shared__ double sa[kMaxK];
    __shared__ double sb[kUpdMaxSplits];
    const int t = threadIdx.x;
    for (int e = t; e < K; e += 256) sa[e] = pshift[e];
    if (pd2)
        for (int e = t; e < splits; e += 256) sb[e] = pd2[e];
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += sa[k];
        stats[0] = s;
    } else if (t == 64) {
        double s = 0.0;
        if (pd2)
            for (int sp = 0; sp < splits; ++sp) s += sb[sp];
        stats[1] = s;
    }
}

// ---- seeding -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double km_u01(const double* u, const unsigned long long* rng, int j) {
    if (u) return u[j];
    uint32_t w[4];
    philox4x32_10(rng[0], rng[1], VG_DRAW_KMEANS_U, (unsigned long long)j >> 2, w);
    const uint32_t sel = (uint32_t)(j & 3);
    const uint32_t ww = sel == 0 ? w[0] : sel == 1 ? w[1] : sel == 2 ? w[2] : w[3];
    return (double)((float)(ww >> 8) * 5.9604644775390625e-08f);
}

// step j, first launch: mind2 against centre j (the row idx[j]; for j = 0 every workgroup derives idx[0] from u_0 and
// workgroup 0 stores it and centre 0), one thread per row, columns ascending; then the block's total, rows ascending
__global__ __launch_bounds__(256) void kmeans_seed_update_kernel(const float* __restrict__ x, int64_t N, int D, int64_t stride,
                                                                 int j, const double* __restrict__ u,
                                                                 const unsigned long long* __restrict__ rng,
                                                                 int32_t* __restrict__ idx, double* __restrict__ center,
                                                                 double* __restrict__ mind2, double* __restrict__ btot) {
    __shared__ double sc[kMaxD];
    __shared__ double sm[kSeedBlock];
    __shared__ int64_t sidx;
    const int t = threadIdx.x;
    if (t == 0) {
        int64_t c;
        if (j == 0) {
            c = (int64_t)(km_u01(u, rng, 0) * (double)N);
            if (c > N - 1) c = N - 1;
            if (c < 0) c = 0;
            if (blockIdx.x == 0) idx[0] = (int32_t)c;
        } else {
            c = idx[j];
        }
        sidx = c;
    }
    __syncthreads();
    const int64_t c = sidx;
    if (t < D) {
        sc[t] = (double)x[c * stride + t];
        if (j == 0 && blockIdx.x == 0) center[t] = sc[t];
    }
    __syncthreads();
    const int64_t n = (int64_t)blockIdx.x * kSeedBlock + t;
    double m = 0.0;
    if (n < N) {
        const float* xr = x + n * stride;
        double d = 0.0;
        for (int i = 0; i < D; ++i) {
            const double e = (double)xr[i] - sc[i];
            d = fma(e, e, d);
        }
        m = d;
        if (j > 0) {
            const double o = mind2[n];
            m = d < o ? d : o;
        }
        mind2[n] = m;
    }
    sm[t] = m;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int q = 0; q < kSeedBlock; ++q) s += sm[q];               // rows past N hold 0
        btot[blockIdx.x] = s;
    }
}

// step j, second launch, ONE workgroup: total = the block totals in ascending order; idx[j] = the first row whose
// two-level cumulative sum exceeds u_j * total (N - 1 if there is none); centre j = that row
__global__ __launch_bounds__(256) void kmeans_seed_pick_kernel(const float* __restrict__ x, int64_t N, int D, int64_t stride,
                                                               int j, const double* __restrict__ u,
                                                               const unsigned long long* __restrict__ rng,
                                                               const double* __restrict__ mind2,
                                                               const double* __restrict__ btot, int64_t nblocks,
                                                               int32_t* __restrict__ idx, double* __restrict__ center) {
    __shared__ double sb[1024];
    __shared__ double srun, starget;
    __shared__ int64_t sfound, spick;
    const int t = threadIdx.x;
    if (t == 0) srun = 0.0;
    for (int64_t base = 0; base < nblocks; base += 1024) {
        __syncthreads();
        for (int e = t; e < 1024; e += 256) sb[e] = base + e < nblocks ? btot[base + e] : 0.0;
        __syncthreads();
        if (t == 0) {
            double s = srun;
            const int64_t m = nblocks - base < 1024 ? nblocks - base : 1024;
            for (int q = 0; q < m; ++q) s += sb[q];
            srun = s;
        }
    }
    __syncthreads();
    if (t == 0) {
        starget = km_u01(u, rng, j) * srun;
        srun = 0.0;
        sfound = -1;
    }
    for (int64_t base = 0; base < nblocks; base += 1024) {
        __syncthreads();
        if (sfound >= 0) break;                                        // uniform: read after the barrier
        for (int e = t; e < 1024; e += 256) sb[e] = base + e < nblocks ? btot[base + e] : 0.0;
        __syncthreads();
        if (t == 0) {
            double s = srun;
            const double target = starget;
            const int64_t m = nblocks - base < 1024 ? nblocks - base : 1024;
            for (int q = 0; q < m; ++q) {
                const double ns = s + sb[q];
                if (ns > target) {
                    sfound = base + q;
                    break;
                }
                s = ns;
            }
            srun = s;                                                   // the prefix below the found block
        }
    }
    __syncthreads();
    const int64_t b = sfound;
    if (b >= 0) {
        const int64_t n = b * kSeedBlock + t;
        sb[t] = n < N ? mind2[n] : 0.0;
    }
    __syncthreads();
    if (t == 0) {
        int64_t pick = N - 1;
        if (b >= 0) {
            const double prefix = srun, target = starget;
            double s = 0.0;                                             // the block's own running sum: its end is the block total,
            for (int q = 0; q < kSeedBlock; ++q) {                      // so prefix + s ends at the value that found the block
                s += sb[q];
                if (prefix + s > target) {
                    const int64_t n = b * kSeedBlock + q;
                    pick = n < N ? n : N - 1;
                    break;
                }
            }
        }
        spick = pick;
        idx[j] = (int32_t)pick;
    }
    __syncthreads();
    const int64_t pick = spick;
    if (t < D) center[(int64_t)j * D + t] = (double)x[pick * stride + t];
}

template <int RF, bool RS>
void launch_assign(const vg_km_plan& p, hipStream_t st, const float* x, int64_t N, int D, int64_t stride, int K,
                   const double* center, int32_t* label, double* dist2, double* resp, const int32_t* prev,
                   int32_t* changed) {
    hipLaunchKernelGGL((kmeans_assign_kernel<RF, RS>), dim3((unsigned)p.assign_grid), dim3(256),
                       (size_t)p.assign_lds_bytes, st, x, N, D, stride, K, center, label, dist2, resp, prev, changed);
}

}  // namespace

extern "C" int vg_kmeans_plan(int64_t N, int D, int K, vg_km_plan* out) {
    VG_CHECK_ARG(out && km_args_ok(N, D, K), VG_EINVAL);
    *out = km_plan(N, D, K);
    return 0;
}

extern "C" int vg_kmeans_assign(const float* x, int64_t N, int D, int64_t row_stride, int K, const double* center,
                                int32_t* label, double* dist2, double* resp, const int32_t* prev_label, int32_t* changed,
                                void* stream) {
    VG_CHECK_ARG(x && center && km_args_ok(N, D, K) && row_stride >= D, VG_EINVAL);
    VG_CHECK_ARG(label || dist2 || resp || changed, VG_EINVAL);
    VG_CHECK_ARG((changed != nullptr) == (prev_label != nullptr), VG_EINVAL);
    VG_CHECK_ARG(aligned8(center) && aligned8(dist2) && aligned8(resp), VG_EALIGN);
    const vg_km_plan p = km_plan(N, D, K);
    VG_CHECK_ARG(p.assign_lds_bytes <= kLdsBudget, VG_EINVAL);
    hipStream_t st = vg_stream(stream);
    if (changed) {
        const hipError_t e = hipMemsetAsync(changed, 0, sizeof(int32_t), st);
        if (e != hipSuccess) return (int)e;
    }
    if (p.assign_rows == 64 && p.assign_row_split)
        launch_assign<4, true>(p, st, x, N, D, row_stride, K, center, label, dist2, resp, prev_label, changed);
    else if (p.assign_rows == 64)
        launch_assign<4, false>(p, st, x, N, D, row_stride, K, center, label, dist2, resp, prev_label, changed);
    else
        launch_assign<2, false>(p, st, x, N, D, row_stride, K, center, label, dist2, resp, prev_label, changed);
    return VG_LAUNCH_RC();
}

extern "C" int64_t vg_kmeans_update_ws_bytes(int64_t N, int D, int K) {
    if (!km_args_ok(N, D, K)) return VG_EINVAL;
    return km_plan(N, D, K).update_ws_bytes;
}

extern "C" int vg_kmeans_update(const float* x, int64_t N, int D, int64_t row_stride, int K, const int32_t* label,
                                const double* dist2, const double* old, int64_t* count, double* sum, double* center,
                                double* stats, void* ws, int64_t ws_bytes, void* stream) {
    VG_CHECK_ARG(x && label && count && ws && km_args_ok(N, D, K) && row_stride >= D, VG_EINVAL);
    VG_CHECK_ARG(center == nullptr || old != nullptr, VG_EINVAL);
    VG_CHECK_ARG(dist2 == nullptr || stats != nullptr, VG_EINVAL);
    const vg_km_plan p = km_plan(N, D, K);
    VG_CHECK_ARG(ws_bytes >= p.update_ws_bytes, VG_EINVAL);
    VG_CHECK_ARG(aligned8(dist2) && aligned8(old) && aligned8(count) && aligned8(sum) && aligned8(center) &&
                 aligned8(stats) && aligned8(ws), VG_EALIGN);
    const int want_sum = (sum || center) ? 1 : 0;
    double* psum = static_cast<double*>(ws);
    int64_t* pcnt = reinterpret_cast<int64_t*>(psum + (int64_t)p.update_splits * K * D);
    double* pd2 = reinterpret_cast<double*>(pcnt + (int64_t)p.update_splits * K);
    double* pshift = pd2 + p.update_splits;
    const size_t lds = (size_t)8 * ((size_t)p.update_chunk * D + 256) + (size_t)4 * (p.update_chunk + 256);
    hipStream_t st = vg_stream(stream);
    hipLaunchKernelGGL(kmeans_update_kernel, dim3(p.update_splits, p.update_chunks), dim3(256), lds, st, x, N, D, row_stride,
                       K, label, dist2, p.update_rows_per_split, p.update_chunk, want_sum, psum, pcnt, pd2);
    hipLaunchKernelGGL(kmeans_update_reduce_kernel, dim3(K), dim3(256), 0, st, psum, pcnt, p.update_splits, D, K, want_sum,
                       old, count, sum, center, pshift);
    if (stats)
        hipLaunchKernelGGL(kmeans_update_stats_kernel, dim3(1), dim3(256), 0, st, pshift, K, dist2 ? pd2 : nullptr,
                           p.update_splits, stats);
    return VG_LAUNCH_RC();
}

extern "C" int64_t vg_kmeans_seed_ws_bytes(int64_t N, int D, int K) {
    if (!km_args_ok(N, D, K)) return VG_EINVAL;
    return km_plan(N, D, K).seed_ws_bytes;
}

extern "C" int vg_kmeans_seed(const float* x, int64_t N, int D, int64_t row_stride, int K, const double* u,
                              const uint64_t* rng, int32_t* idx, double* center, void* ws, int64_t ws_bytes, void* stream) {
    VG_CHECK_ARG(x && idx && center && ws && km_args_ok(N, D, K) && row_stride >= D, VG_EINVAL);
    VG_CHECK_ARG(u || rng, VG_EINVAL);
    const vg_km_plan p = km_plan(N, D, K);
    VG_CHECK_ARG(ws_bytes >= p.seed_ws_bytes, VG_EINVAL);
    VG_CHECK_ARG(aligned8(u) && aligned8(rng) && aligned8(center) && aligned8(ws), VG_EALIGN);
    double* mind2 = static_cast<double*>(ws);
    double* btot = mind2 + N;
    const unsigned long long* r = reinterpret_cast<const unsigned long long*>(rng);
    hipStream_t st = vg_stream(stream);
    for (int j = 0; j < K; ++j) {
        hipLaunchKernelGGL(kmeans_seed_update_kernel, dim3((unsigned)p.seed_blocks), dim3(256), 0, st, x, N, D, row_stride, j,
                           u, r, idx, center, mind2, btot);
        if (j + 1 < K)
            hipLaunchKernelGGL(kmeans_seed_pick_kernel, dim3(1), dim3(256), 0, st, x, N, D, row_stride, j + 1, u, r, mind2,
                               btot, p.seed_blocks, idx, center);
    }
    return VG_LAUNCH_RC();
}
