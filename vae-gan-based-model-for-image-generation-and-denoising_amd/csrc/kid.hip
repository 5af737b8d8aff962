// Kernel Inception Distance (Binkowski et al. 2018, "Demystifying MMD GANs"): the unbiased polynomial-kernel MMD^2
// estimate of two feature sets, one score per random subset pair.  The reference computes no KID; like precision / recall
// (its README.md:22) this goes beyond its code.  The contract is stated in include/vaegan_hip.h, "Feature-space metrics".
//   vg_kid_scores   sums of k(a, c) = (gamma dot(a, c) + coef)^degree over the real / real, fake / fake and real / fake
//                   pairs of every subset, dot on v_mfma_f64_16x16x4_f64 over the exactly converted f32 rows
// The m x m Gram matrix never exists: a workgroup owns one 64 x 64 tile of one family of one subset, applies the kernel
// function to its accumulators and writes ONE f64; a second launch adds the tiles in a fixed order and forms the scores.
#include <cmath>
#include "common.hpp"

typedef __attribute__((ext_vector_type(4))) double f64x4;

namespace {

constexpr int kKT = 64;            // tile: 64 x 64 subset positions per workgroup, 32 x 32 per wave
constexpr int kKK = 32;            // feature columns staged per step
constexpr int kKS = 36;            // LDS row stride in floats: 16 rows x 4 adjacent columns, conflict-free
constexpr int kMaxD = 2048;
constexpr int kMaxM = 32768;
constexpr int kMaxS = 4096;
constexpr int kMaxDegree = 8;
constexpr int kFinalThreads = 1024;

struct KidPlan {
    int T;          // tiles per side
    int64_t P;      // tiles on or above the diagonal (families xx and yy)
    int64_t W;      // tiles of one subset: xx | yy | xy
};

KidPlan kid_plan(int64_t m) {
    KidPlan p;
    p.T = (int)((m + kKT - 1) / kKT);
    p.P = (int64_t)p.T * (p.T + 1) / 2;
    p.W = 2 * p.P + (int64_t)p.T * p.T;
    return p;
}

bool kid_size_ok(int64_t m, int S) {
    if (m < 2 || m > kMaxM || S < 1 || S > kMaxS) return false;
    return kid_plan(m).W * S <= 2147483647ll;
}

__device__ __forceinline__ void kid_pair_tiles(int p, int T, int& ti, int& tj) {
    ti = 0;
    while (p >= T - ti) { p -= T - ti; ++ti; }
    tj = ti + p;
}

// One k-step of one operand in registers: 64 rows x 32 columns over 256 threads.
// VEC (D % 4 == 0): thread = (row t >> 3 (+32), columns 4 (t & 7) .. + 3) as one 16-byte load;
// else: thread = (row t >> 5 (+8 p), column t & 31).
template <bool VEC> struct KidRegs;
template <> struct KidRegs<true> {
    float4 v[2];
    __device__ __forceinline__ void fetch(const float* __restrict__ src, const int64_t* roff, int D, int k0, int t) {
        const int kq = (t & 7) * 4, rr = t >> 3;
        const bool kin = k0 + kq < D;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int64_t off = roff[rr + 32 * p];
            v[p] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kin && off >= 0) v[p] = *reinterpret_cast<const float4*>(src + off + k0 + kq);
        }
    }
    __device__ __forceinline__ void commit(float (*s)[kKS], int t) const {
        const int kq = (t & 7) * 4, rr = t >> 3;
#pragma unroll
        for (int p = 0; p < 2; ++p) *reinterpret_cast<float4*>(&s[rr + 32 * p][kq]) = v[p];
    }
};
template <> struct KidRegs<false> {
    float v[8];
    __device__ __forceinline__ void fetch(const float* __restrict__ src, const int64_t* roff, int D, int k0, int t) {
        const int kq = t & 31, rr = t >> 5;
        const bool kin = k0 + kq < D;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int64_t off = roff[rr + 8 * p];
            v[p] = (kin && off >= 0) ? src[off + k0 + kq] : 0.f;
        }
    }
    __device__ __forceinline__ void commit(float (*s)[kKS], int t) const {
        const int kq = t & 31, rr = t >> 5;
#pragma unroll
        for (int p = 0; p < 8; ++p) s[rr + 8 * p][kq] = v[p];
    }
};

// grid (W tiles, S subsets).  Tile order inside a subset: xx pairs (ti <= tj), yy pairs, xy (ti * T + tj).
// A[i][c] = rowsA[ia + i][c], B[c][j] = rowsB[jb + j][c], both converted exactly to f64 on the way into the MFMA; rows at
// subset positions >= m and columns >= D are staged as 0 and their results are masked (never multiplied in).  The next
// k-step's rows are fetched into registers while the MFMAs of the current one run.
template <bool VEC>
__global__ __launch_bounds__(256) void kid_tile_kernel(const float* __restrict__ real, int64_t Nr,
                                                       const float* __restrict__ fake, int64_t Nf, int D,
                                                       const int32_t* __restrict__ idx_real,
                                                       const int32_t* __restrict__ idx_fake, int m, int T, int P, int degree,
                                                       double gamma, double coef, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sa[kKT][kKS], sb[kKT][kKS];
    __shared__ int64_t roff_a[kKT], roff_b[kKT];
    __shared__ double wpart[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int lq = lane >> 4, lc = lane & 15;
    const int s = blockIdx.y;
    int w = blockIdx.x, fam, ti, tj;
    if (w < P) { fam = 0; kid_pair_tiles(w, T, ti, tj); }
    else if (w < 2 * P) { fam = 1; kid_pair_tiles(w - P, T, ti, tj); }
    else { fam = 2; w -= 2 * P; ti = w / T; tj = w - ti * T; }
    const bool diag = fam != 2 && ti == tj;                 // B is A: staged once, position i == j masked
    const float* srcA = fam == 1 ? fake : real;
    const float* srcB = fam == 0 ? real : fake;
    const int64_t NA = fam == 1 ? Nf : Nr, NB = fam == 0 ? Nr : Nf;
    const int32_t* ta = (fam == 1 ? idx_fake : idx_real) + (int64_t)s * m;
    const int32_t* tb = (fam == 0 ? idx_real : idx_fake) + (int64_t)s * m;
    const int ia = ti * kKT, jb = tj * kKT;

    // the tile's row offsets, clamped into the matrix; -1: a position past the subset
    if (t < kKT) {
        const int pos = ia + t;
        int64_t off = -1;
        if (pos < m) {
            int64_t r = ta[pos];
            r = r < 0 ? 0 : (r >= NA ? NA - 1 : r);
            off = r * D;
        }
        roff_a[t] = off;
    } else if (t < 2 * kKT) {
        const int pos = jb + t - kKT;
        int64_t off = -1;
        if (pos < m) {
            int64_t r = tb[pos];
            r = r < 0 ? 0 : (r >= NB ? NB - 1 : r);
            off = r * D;
        }
        roff_b[t - kKT] = off;
    }
    __syncthreads();

    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};

    const float (*sbb)[kKS] = diag ? sa : sb;
    KidRegs<VEC> ra, rb;
    ra.fetch(srcA, roff_a, D, 0, t);
    if (!diag) rb.fetch(srcB, roff_b, D, 0, t);
    for (int k0 = 0; k0 < D; k0 += kKK) {
        ra.commit(sa, t);
        if (!diag) rb.commit(sb, t);
        __syncthreads();
        if (k0 + kKK < D) {
            ra.fetch(srcA, roff_a, D, k0 + kKK, t);
            if (!diag) rb.fetch(srcB, roff_b, D, k0 + kKK, t);
        }
#pragma unroll
        for (int kk = 0; kk < kKK; kk += 4) {
            const double a0 = (double)sa[32 * wi + lc][kk + lq], a1 = (double)sa[32 * wi + 16 + lc][kk + lq];
            const double b0 = (double)sbb[32 * wj + lc][kk + lq], b1 = (double)sbb[32 * wj + 16 + lc][kk + lq];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }

    // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg.  k = b^degree by degree - 1 multiplications.
    double lsum = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int i = ia + 32 * wi + 16 * a + lq + 4 * g, j = jb + 32 * wj + 16 * b + lc;
                const double base = gamma * acc[a][b][g] + coef;
                double k = base;
                for (int d = 1; d < degree; ++d) k *= base;
                const bool keep = i < m && j < m && !(diag && i == j);
                lsum += keep ? k : 0.0;
            }
    lsum = wave_sum_d(lsum);
    if (lane == 0) wpart[wave] = lsum;
    __syncthreads();
    if (t == 0) {
        double tot = ((wpart[0] + wpart[1]) + wpart[2]) + wpart[3];
        if (fam != 2 && ti != tj) tot *= 2.0;               // k is symmetric: the tile below the diagonal is this one
        part[(int64_t)s * (2 * (int64_t)P + (int64_t)T * T) + blockIdx.x] = tot;
    }
}

// One workgroup.  A wavefront per subset: the family's tile partials are read 64 at a time (one per lane) through LDS and
// added by lane 0 in ascending tile order; then thread 0 forms mean and population standard deviation in ascending s.
__global__ __launch_bounds__(kFinalThreads) void kid_final_kernel(const double* __restrict__ part, int S, int m, int64_t P,
                                                                  int64_t TT, double* __restrict__ sums,
                                                                  double* __restrict__ scores, double* __restrict__ stat) {
    __shared__ double chunk[kFinalThreads / 64][64];
    __shared__ double ssc[kMaxS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t W = 2 * P + TT;
    for (int s = wave; s < S; s += kFinalThreads / 64) {
        double fs[3];
#pragma unroll
        for (int fam = 0; fam < 3; ++fam) {
            const int64_t cnt = fam == 2 ? TT : P;
            const double* src = part + (int64_t)s * W + fam * P;          // xx at 0, yy at P, xy at 2 P
            double a = 0.0;
            for (int64_t c0 = 0; c0 < cnt; c0 += 64) {
                const int n = cnt - c0 < 64 ? (int)(cnt - c0) : 64;
                if (lane < n) chunk[wave][lane] = src[c0 + lane];
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                for (int i = 0; i < n; ++i) a += chunk[wave][i];
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            fs[fam] = a;
        }
        if (lane == 0) {
            const double dm = (double)m;
            const double sc = (fs[0] + fs[1]) / (dm * (dm - 1.0)) - 2.0 * fs[2] / (dm * dm);
            sums[3 * s + 0] = fs[0];
            sums[3 * s + 1] = fs[1];
            sums[3 * s + 2] = fs[2];
            scores[s] = sc;
            ssc[s] = sc;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int s = 0; s < S; ++s) tot += ssc[s];
        const double mean = tot / (double)S;
        double var = 0.0;
        for (int s = 0; s < S; ++s) {
            const double d = ssc[s] - mean;
            var += d * d;
        }
        stat[0] = mean;
        stat[1] = S == 1 ? 0.0 : sqrt(var / (double)S);
    }
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

}  // namespace

extern "C" int64_t vg_kid_scores_ws_bytes(int64_t m, int S) {
    if (!kid_size_ok(m, S)) return VG_EINVAL;
    return 8 * (int64_t)S * kid_plan(m).W;
}

extern "C" int vg_kid_scores(const float* real, int64_t Nr, const float* fake, int64_t Nf, int D, const int32_t* idx_real,
                             const int32_t* idx_fake, int S, int64_t m, int degree, double gamma, double coef, double* sums,
                             double* scores, double* stat, void* ws, int64_t ws_bytes, void* stream) {
    VG_CHECK_ARG(real && fake && idx_real && idx_fake && sums && scores && stat && ws, VG_EINVAL);
    VG_CHECK_ARG(D >= 1 && D <= kMaxD && degree >= 1 && degree <= kMaxDegree && std::isfinite(gamma) && std::isfinite(coef), VG_EINVAL);
    VG_CHECK_ARG(Nr >= 2 && Nf >= 2 && Nr <= 2147483647ll && Nf <= 2147483647ll, VG_EINVAL);
    VG_CHECK_ARG(kid_size_ok(m, S) && m <= Nr && m <= Nf, VG_EINVAL);
    VG_CHECK_ARG(ws_bytes >= vg_kid_scores_ws_bytes(m, S), VG_EINVAL);
    VG_CHECK_ARG(vg_aligned16(real) && vg_aligned16(fake) && (reinterpret_cast<uintptr_t>(idx_real) & 3u) == 0 &&
                 (reinterpret_cast<uintptr_t>(idx_fake) & 3u) == 0 && aligned8(sums) && aligned8(scores) && aligned8(stat) &&
                 aligned8(ws), VG_EALIGN);
    const KidPlan p = kid_plan(m);
    hipStream_t st = vg_stream(stream);
    double* part = static_cast<double*>(ws);
    const dim3 grid((unsigned)p.W, (unsigned)S);
    if ((D & 3) == 0)
        hipLaunchKernelGGL(kid_tile_kernel<true>, grid, dim3(256), 0, st, real, Nr, fake, Nf, D, idx_real, idx_fake, (int)m,
                           p.T, (int)p.P, degree, gamma, coef, part);
    else
        hipLaunchKernelGGL(kid_tile_kernel<false>, grid, dim3(256), 0, st, real, Nr, fake, Nf, D, idx_real, idx_fake, (int)m,
                           p.T, (int)p.P, degree, gamma, coef, part);
    hipLaunchKernelGGL(kid_final_kernel, dim3(1), dim3(kFinalThreads), 0, st, part, S, (int)m, p.P, (int64_t)p.T * p.T, sums,
                       scores, stat);
    return VG_LAUNCH_RC();
}
