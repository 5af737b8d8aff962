// BatchNorm2d (train/eval) + ReLU/LeakyReLU forward and backward on NHWC tensors.
// Replaces the ATen batch_norm / leaky_relu / relu kernels reached through nn.BatchNorm2d,
// nn.LeakyReLU and nn.ReLU at main_vae.py:24-25 and gan_code.py:22-82 (+ their backward).
//
// All tensors are [rows = B*H*W][C] with C contiguous, so a per-channel reduction is a column
// sum: a workgroup owns a contiguous block of rows, each thread a fixed 4-channel column
// (16-byte loads, fully coalesced), partial sums go wave -> LDS -> one slab row per
// workgroup, and a one-thread-per-channel finalize kernel adds the slab rows in fixed order
// in double precision.  Ideal traffic is one read (+ one write) of the tensor; the elementwise passes (normalise +
// activation, backward apply) use the same thread -> column mapping and reach 0.75 of the HBM rate on the largest tensors.
#include "common.hpp"

namespace {

// The launch geometry of every launcher below is a vg_bn_plan (include/vaegan_hip.h): vg_bn_launch_plan returns the record
// a launcher launches from.  Column reduce: a part (rows_per_block rows of one group) per workgroup and column block.
inline vg_bn_plan plan_reduce(int64_t rows_per_group, int C, int groups) {
    const int cols = C / 4;
    const int ncol = cols < 256 ? cols : 256;
    const int rpp = 256 / ncol;
    const int64_t passes = (rows_per_group + rpp - 1) / rpp;
    int64_t np = passes / 8;
    if (np < 1) np = 1;
    if (np > 1024) np = 1024;
    int64_t rows_per_part = ((passes + np - 1) / np) * rpp;
    vg_bn_plan p = {};
    p.kind = VG_BN_PLAN_REDUCE;
    p.vec = 4;
    p.threads_per_row = ncol;
    p.rows_per_pass = rpp;
    p.rows_per_block = (int)rows_per_part;
    p.blocks_per_group = (int)((rows_per_group + rows_per_part - 1) / rows_per_part);
    p.col_blocks = (cols + 255) / 256;
    p.groups = groups;
    return p;
}

// MODE 0: (sum x, sum x*x).  MODE 1: (sum dz, sum dz*xhat) with dz = dy*act'(scale*x+shift).
template <int DT, int MODE>
__global__ __launch_bounds__(256) void col_reduce_kernel(const void* __restrict__ x, const void* __restrict__ dy,
                                                         const float* __restrict__ scale,
                                                         const float* __restrict__ shift,
                                                         const float* __restrict__ mean,
                                                         const float* __restrict__ invstd, int64_t rows, int C,
                                                         int act, float slope, float* __restrict__ partial,
                                                         int rows_per_part, int64_t rows_per_group,
                                                         int parts_per_group, int64_t gstride) {
    __shared__ float4 red[2][256];
    const int cols = C >> 2;
    const int cb = blockIdx.y * 256;
    const int ncol = min(256, cols - cb);
    const int rpp = 256 / ncol;
    const int tid = threadIdx.x;
    const int tr = tid / ncol, tc = tid - tr * ncol;
    const bool active = tr < rpp;
    const int c4 = (cb + tc) * 4;
    // groups: independent row ranges with their own coefficient sets (two Discriminator passes in one launch)
    const int grp = blockIdx.x / parts_per_group;
    const int64_t gbase = (int64_t)grp * rows_per_group;
    const int64_t r0 = gbase + (int64_t)(blockIdx.x - grp * parts_per_group) * rows_per_part;
    const int64_t r1 = min(min(rows, gbase + rows_per_group), r0 + (int64_t)rows_per_part);
    const int64_t go = (int64_t)grp * gstride;
    float4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        float4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f}, mu = sh, is = sc;
        if (MODE == 1) {
            if (scale) { sc = *reinterpret_cast<const float4*>(scale + go + c4); sh = *reinterpret_cast<const float4*>(shift + go + c4); }
            mu = *reinterpret_cast<const float4*>(mean + go + c4);
            is = *reinterpret_cast<const float4*>(invstd + go + c4);
        }
        auto accum = [&](const float4& v, const float4& g) {
            if (MODE == 0) {
                s1.x += v.x; s1.y += v.y; s1.z += v.z; s1.w += v.w;
                s2.x += v.x * v.x; s2.y += v.y * v.y; s2.z += v.z * v.z; s2.w += v.w * v.w;
            } else {
                const float dz0 = act_bwd(sc.x * v.x + sh.x, g.x, act, slope);
                const float dz1 = act_bwd(sc.y * v.y + sh.y, g.y, act, slope);
                const float dz2 = act_bwd(sc.z * v.z + sh.z, g.z, act, slope);
                const float dz3 = act_bwd(sc.w * v.w + sh.w, g.w, act, slope);
                s1.x += dz0; s1.y += dz1; s1.z += dz2; s1.w += dz3;
                s2.x += dz0 * ((v.x - mu.x) * is.x); s2.y += dz1 * ((v.y - mu.y) * is.y);
                s2.z += dz2 * ((v.z - mu.z) * is.z); s2.w += dz3 * ((v.w - mu.w) * is.w);
            }
        };
        // four rows (eight loads) in flight per thread; summation order unchanged
        int64_t r = r0 + tr;
        for (; r + 3 * rpp < r1; r += 4 * rpp) {
            float4 v[4], g[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u] = load4<DT>(x, (r + (int64_t)u * rpp) * C + c4);
                g[u] = (MODE == 1) ? load4<DT>(dy, (r + (int64_t)u * rpp) * C + c4) : float4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) accum(v[u], g[u]);
        }
        for (; r < r1; r += rpp) {
            const float4 v = load4<DT>(x, r * C + c4);
            const float4 g = (MODE == 1) ? load4<DT>(dy, r * C + c4) : float4{0.f, 0.f, 0.f, 0.f};
            accum(v, g);
        }
    }
    red[0][tid] = s1;
    red[1][tid] = s2;
    __syncthreads();
    if (tid < ncol) {
        float4 a = red[0][tid], b = red[1][tid];
        for (int k = 1; k < rpp; ++k) {
            const float4 u = red[0][k * ncol + tid], w = red[1][k * ncol + tid];
            a.x += u.x; a.y += u.y; a.z += u.z; a.w += u.w;
            b.x += w.x; b.y += w.y; b.z += w.z; b.w += w.w;
        }
        const int64_t part = blockIdx.x;
        *reinterpret_cast<float4*>(partial + (part * 2 + 0) * C + c4) = a;
        *reinterpret_cast<float4*>(partial + (part * 2 + 1) * C + c4) = b;
    }
}

// Sum the [nparts][2][C] partial slabs for 8 channels per workgroup: 128 "planes" of threads stride over the
// slab rows (a one-thread-per-channel loop over up to 4096 rows is pure latency: it cost 23 % of the step; with
// 32 planes these ~48 launches per iteration were still 5 us each, 6 % of it), double accumulation, then a
// fixed-order combine (xor-shuffles over the 8 planes of a wave, LDS over the 16 waves) -> bitwise reproducible.
// Returns the sums to threads tid < 8.
//
// Every load a thread needs is issued before the first add that waits for one: a load-add loop is one memory round trip
// per row (s_waitcnt vmcnt(0) in front of every add), and these launches are nothing but round trips.  A thread's first
// FIN_FIRST rows are one batch (FinRows: rows beyond nparts hold +0, and a sum that started at +0 is never -0, so adding
// them changes no bit), the rest follows FIN_DEPTH rows at a time; the grouped kernels load the next group's first batch
// before they finish the current group.  The adds stay in row order per thread.
constexpr int FIN_CH = 8, FIN_PL = 128, FIN_FIRST = 4, FIN_DEPTH = 8;
struct FinRows { float x[FIN_FIRST], y[FIN_FIRST]; };

// The slab is read through a buffer descriptor over exactly its nparts rows (SlabBuf): a load is a uniform descriptor plus
// one 32-bit per-thread byte offset, and a row beyond the slab comes back as +0 from the hardware range check -- no
// predicate, so no branch around a load (the compiler moves the conversion to double into a predicated block, and the wait
// with it) and no 64-bit address per load in flight.  The launchers refuse slabs of 2^31 bytes.
struct SlabBuf {
    __amdgpu_buffer_rsrc_t rsrc;
    unsigned row;                                              // bytes per slab row: 2 * C floats
    __device__ __forceinline__ SlabBuf(const float* slabs, int nparts, int C, bool live = true)
        : rsrc(__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(slabs), 0, live ? (int)((unsigned)nparts * 2u * (unsigned)C * 4u) : 0, 0x00020000)),
          row((unsigned)C * 8u) {}
    // (sum x, sum x*x) entries of row p, channel c
    __device__ __forceinline__ void load(unsigned p, unsigned c, float& x, float& y) const {
        const unsigned off = p * row + c * 4u;
        x = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0));
        y = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, off + row / 2u, 0, 0));
    }
};

// SlabBuf's 32-bit byte offsets: a thread asks for rows up to one batch beyond the slab, and that offset must not wrap
inline bool slab_fits(int64_t nparts, int64_t C) { return (nparts + 2048) * 2 * C * 4 < (1ll << 32); }

// a thread's first batch: rows pl + k * FIN_PL, k < FIN_FIRST -- the whole slab up to 4 * FIN_PL rows (every launch of the
// flagship step but one).  live = false: no slab (every row +0, nothing is read).
__device__ __forceinline__ void fin_load_first(const float* __restrict__ slabs, int nparts, int C, FinRows& r, bool live = true) {
    const int c = blockIdx.x * FIN_CH + (threadIdx.x & (FIN_CH - 1)), pl = threadIdx.x / FIN_CH;
    const SlabBuf sb(slabs, nparts, C, live);
    const unsigned cc = c < C ? c : C - 1;                     // (a thread without a channel adds nothing: see slab_sums_from)
#pragma unroll
    for (int k = 0; k < FIN_FIRST; ++k) sb.load(pl + k * FIN_PL, cc, r.x[k], r.y[k]);
}

// r: what fin_load_first(slabs, nparts, C, .) gave
__device__ __forceinline__ bool slab_sums_from(const float* __restrict__ slabs, int nparts, int C, const FinRows& r,
                                               double& s1, double& s2, int& c_out) {
    constexpr int NW = FIN_CH * FIN_PL / 64;
    __shared__ double red[NW][FIN_CH][2];
    const int cl = threadIdx.x & (FIN_CH - 1);
    const int pl = threadIdx.x / FIN_CH;
    const int c = blockIdx.x * FIN_CH + cl;
    double a = 0.0, b = 0.0;
    if (c < C) {
#pragma unroll
        for (int k = 0; k < FIN_FIRST; ++k) { a += (double)r.x[k]; b += (double)r.y[k]; }
        const SlabBuf sb(slabs, nparts, C);
        for (int base = FIN_FIRST * FIN_PL; base < nparts; base += FIN_DEPTH * FIN_PL) {
            float x[FIN_DEPTH], y[FIN_DEPTH];
#pragma unroll
            for (int k = 0; k < FIN_DEPTH; ++k) sb.load(base + pl + k * FIN_PL, c, x[k], y[k]);
#pragma unroll
            for (int k = 0; k < FIN_DEPTH; ++k) { a += (double)x[k]; b += (double)y[k]; }
        }
    }
    // a wave holds 8 planes x 8 channels (lane = 8*plane + channel): butterfly over the plane bits
#pragma unroll
    for (int o = FIN_CH; o < 64; o <<= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane < FIN_CH) { red[wave][lane][0] = a; red[wave][lane][1] = b; }
    __syncthreads();
    if (pl != 0 || c >= C) return false;
    a = red[0][cl][0]; b = red[0][cl][1];
#pragma unroll
    for (int k = 1; k < NW; ++k) { a += red[k][cl][0]; b += red[k][cl][1]; }
    s1 = a; s2 = b; c_out = c;
    return true;
}

__device__ __forceinline__ bool slab_sums(const float* __restrict__ slabs, int nparts, int C, double& s1, double& s2,
                                          int& c_out) {
    FinRows r;
    fin_load_first(slabs, nparts, C, r);
    return slab_sums_from(slabs, nparts, C, r, s1, s2, c_out);
}

// the lead thread of channel c (the one slab_sums returns the sums to), known before the sums: it loads its per-channel
// operands at kernel entry, together with the slab rows, not one more round trip after them
__device__ __forceinline__ bool fin_lead(int C, int& c) {
    c = blockIdx.x * FIN_CH + (threadIdx.x & (FIN_CH - 1));
    return threadIdx.x < FIN_CH && c < C;
}
__device__ __forceinline__ float lead_load(bool lead, const float* __restrict__ p, int c, float otherwise) {
    return (lead && p) ? p[c] : otherwise;
}

// running statistic after one batch: both products rounded, then the sum (torch's own order; spelled out because the value
// now lives in a register across the groups, where the compiler would contract one product into the sum and move the
// last bit of the running statistics)
__device__ __forceinline__ float running_update(float momentum, float r, float v) {
#pragma clang fp contract(off)
    return (1.f - momentum) * r + momentum * v;
}

__global__ __launch_bounds__(FIN_CH * FIN_PL) void bn_finalize_kernel(
    const float* __restrict__ stats, int nparts, int C, double count, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar, float momentum, float eps,
    float* __restrict__ mean, float* __restrict__ invstd, float* __restrict__ scale, float* __restrict__ shift) {
    double s1, s2;
    int c;
    const bool lead = fin_lead(C, c);
    const float g = lead_load(lead, gamma, c, 1.f), b = lead_load(lead, beta, c, 0.f);
    const float rm = lead_load(lead, rmean, c, 0.f), rv = lead_load(lead && rmean, rvar, c, 0.f);
    if (!slab_sums(stats, nparts, C, s1, s2, c)) return;
    const double mu = s1 / count;
    double var = s2 / count - mu * mu;
    if (var < 0.0) var = 0.0;
    const float is = (float)(1.0 / sqrt(var + (double)eps));
    const float muf = (float)mu;
    mean[c] = muf;
    invstd[c] = is;
    const float sc = g * is;
    scale[c] = sc;
    shift[c] = b - muf * sc;
    if (rmean) {
        const double unbiased = count > 1.0 ? var * (count / (count - 1.0)) : var;
        rmean[c] = running_update(momentum, rm, muf);
        rvar[c] = running_update(momentum, rv, (float)unbiased);
    }
}

// ---- grouped finalize: `groups` independent row blocks (a Discriminator iteration's real and fake batches) in
// ONE launch; a channel's groups are processed in order by the same thread, so the running statistics are updated
// real-then-fake exactly as two separate forward calls would (and dgamma/dbeta accumulate in that order).
__global__ __launch_bounds__(FIN_CH * FIN_PL) void bn_finalize_grouped_kernel(
    const float* __restrict__ stats, int nparts, int groups, int C, double count, const float* __restrict__ gamma,
    const float* __restrict__ beta, float* __restrict__ rmean, float* __restrict__ rvar, float momentum, float eps,
    float* __restrict__ coeffs) {
    int c;
    const bool lead = fin_lead(C, c);
    const float gm = lead_load(lead, gamma, c, 1.f), bt = lead_load(lead, beta, c, 0.f);
    float rm = lead_load(lead, rmean, c, 0.f), rv = lead_load(lead && rmean, rvar, c, 0.f);
    FinRows cur, nxt;
    fin_load_first(stats, nparts, C, cur);
    for (int g = 0; g < groups; ++g) {
        const float* slab = stats + (int64_t)g * nparts * 2 * C;
        fin_load_first(slab + (int64_t)nparts * 2 * C, nparts, C, nxt, g + 1 < groups);      // in flight while g is summed
        double s1, s2;
        if (slab_sums_from(slab, nparts, C, cur, s1, s2, c)) {
            float* co = coeffs + (int64_t)g * 4 * C;
            const double mu = s1 / count;
            double var = s2 / count - mu * mu;
            if (var < 0.0) var = 0.0;
            const float is = (float)(1.0 / sqrt(var + (double)eps));
            const float muf = (float)mu;
            co[c] = muf;
            co[C + c] = is;
            const float sc = gm * is;
            co[2 * C + c] = sc;
            co[3 * C + c] = bt - muf * sc;
            if (rmean) {
                const double unbiased = count > 1.0 ? var * (count / (count - 1.0)) : var;
                rm = running_update(momentum, rm, muf);
                rv = running_update(momentum, rv, (float)unbiased);
            }
        }
        cur = nxt;
        __syncthreads();                                    // slab_sums' LDS scratch is reused by the next group
    }
    if (lead && rmean && groups > 0) { rmean[c] = rm; rvar[c] = rv; }
}

__global__ __launch_bounds__(FIN_CH * FIN_PL) void bn_bwd_finalize_grouped_kernel(
    const float* __restrict__ partial, int nparts, int groups, int C, double count, const float* __restrict__ gamma,
    const float* __restrict__ coeffs, float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate,
    float* __restrict__ coef) {
    int c;
    const bool lead = fin_lead(C, c);
    const float gm = lead_load(lead, gamma, c, 1.f);
    float dg = lead_load(lead && accumulate, dgamma, c, 0.f), db = lead_load(lead && accumulate, dbeta, c, 0.f);
    float is = lead_load(lead, coeffs + C, c, 0.f), is_nxt = 0.f;                           // group 0's invstd
    FinRows cur, nxt;
    fin_load_first(partial, nparts, C, cur);
    for (int g = 0; g < groups; ++g) {
        const float* slab = partial + (int64_t)g * nparts * 2 * C;
        // the next group's rows and invstd, in flight while g is summed
        fin_load_first(slab + (int64_t)nparts * 2 * C, nparts, C, nxt, g + 1 < groups);
        is_nxt = lead_load(lead && g + 1 < groups, coeffs + (int64_t)(g + 1) * 4 * C + C, c, 0.f);
        double s1, s2;
        if (slab_sums_from(slab, nparts, C, cur, s1, s2, c)) {
            const float fs1 = (float)s1, fs2 = (float)s2;
            const bool acc = accumulate || g > 0;
            dg = acc ? dg + fs2 : fs2;
            db = acc ? db + fs1 : fs1;
            const float a = gm * is;                        // gamma * invstd
            float* cf = coef + (int64_t)g * 3 * C;
            cf[c] = a;
            cf[C + c] = (float)((double)a * s2 / count);
            cf[2 * C + c] = (float)((double)a * s1 / count);
        }
        cur = nxt; is = is_nxt;
        __syncthreads();
    }
    if (lead && groups > 0) {
        if (dgamma) dgamma[c] = dg;
        if (dbeta) dbeta[c] = db;
    }
}

// ---- synchronised BatchNorm (one process per GPU, statistics over the GLOBAL batch) --------------------------
// The host all-reduces the f64 [2][C] sums between these kernels (vaegan_amd ddp.py); arithmetic after the sums
// is the same as bn_finalize_kernel / bn_bwd_finalize_kernel.
__global__ __launch_bounds__(FIN_CH * FIN_PL) void slab_sums_kernel(const float* __restrict__ slabs, int nparts, int C,
                                                                    double* __restrict__ sums) {
    double s1, s2;
    int c;
    if (!slab_sums(slabs, nparts, C, s1, s2, c)) return;
    sums[c] = s1;
    sums[C + c] = s2;
}

__global__ void bn_finalize_sums_kernel(const double* __restrict__ sums, int C, double count,
                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                        float* __restrict__ rmean, float* __restrict__ rvar, float momentum, float eps,
                                        float* __restrict__ mean, float* __restrict__ invstd,
                                        float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double mu = sums[c] / count;
    double var = sums[C + c] / count - mu * mu;
    if (var < 0.0) var = 0.0;
    const float is = (float)(1.0 / sqrt(var + (double)eps));
    const float muf = (float)mu;
    mean[c] = muf;
    invstd[c] = is;
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
    const float sc = g * is;
    scale[c] = sc;
    shift[c] = b - muf * sc;
    if (rmean) {
        const double unbiased = count > 1.0 ? var * (count / (count - 1.0)) : var;
        rmean[c] = (1.f - momentum) * rmean[c] + momentum * muf;
        rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unbiased;
    }
}

// dgamma/dbeta are this rank's LOCAL sums (the gradient all-reduce averages them like every other parameter
// gradient); the dx coefficients use the GLOBAL sums and the global element count.
__global__ void bn_bwd_finalize_sums_kernel(const double* __restrict__ gsums, const double* __restrict__ lsums, int C,
                                            double count, const float* __restrict__ gamma,
                                            const float* __restrict__ invstd, float* __restrict__ dgamma,
                                            float* __restrict__ dbeta, int accumulate, float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float l1 = (float)lsums[c], l2 = (float)lsums[C + c];
    if (dgamma) dgamma[c] = accumulate ? dgamma[c] + l2 : l2;
    if (dbeta) dbeta[c] = accumulate ? dbeta[c] + l1 : l1;
    const float a = (gamma ? gamma[c] : 1.f) * invstd[c];
    coef[c] = a;
    coef[C + c] = (float)((double)a * gsums[C + c] / count);
    coef[2 * C + c] = (float)((double)a * gsums[c] / count);
}

__global__ void bn_eval_kernel(const float* gamma, const float* beta, const float* rmean, const float* rvar,
                               float eps, int C, float* scale, float* shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float is = 1.f / sqrtf(rvar[c] + eps);
    const float sc = (gamma ? gamma[c] : 1.f) * is;
    scale[c] = sc;
    shift[c] = (beta ? beta[c] : 0.f) - rmean[c] * sc;
}

// ---- streaming passes over a [rows][C] tensor (normalise + activation, backward apply) -------------------------------
// A thread owns VW consecutive channels -- 16 bytes: 8 channels of bf16 when C % 8 == 0, 4 channels of f32; 8 bytes (4
// channels of bf16) otherwise -- and walks rows, with col_reduce_kernel's thread -> (row slot, channel column) mapping:
// min(C / VW, 256) threads per row, 256 / that rows per pass (leftover threads idle), blockIdx.y the block of 256 columns.
// blockIdx = (row block, column block, group): a workgroup never straddles a group, so the per-channel coefficients of its
// group are loaded ONCE into registers before the row loop, and the loop has no division: the offset advances by
// rows-per-pass * C.  Four rows (4 x 16 bytes per tensor) are in flight per thread; a row block's last trip may be short.
constexpr int EW_UNROLL = 4;
// Grid cap = the workgroups that are resident at once on the 256 CUs, so that larger tensors give each thread several trips
// of EW_UNROLL rows and no second, partly filled round of workgroups follows: 4 per CU for the forward pass; 3 per CU for
// the backward apply, whose 7 coefficient vectors + 8 packed vectors in flight take 164 VGPRs with 8 channels per thread.
constexpr int EW_FWD_WGS = 1024, EW_BWD_WGS = 768;
// Below 4 MiB (VG_BN_WIDE_MIN) a bf16 tensor keeps 4 channels (8 bytes) per thread: such a launch is one pass per workgroup
// and one round trip long, and what it waits for is its coefficients (seven vectors per thread in the backward apply) --
// half as many bytes per thread on twice as many CUs is 0.2-0.3 us quicker there; from 4 MiB on the 16-byte form wins
// (DESIGN.md 4.3).
inline bool stream_wide(int dtype, int64_t rows, int C) {
    return dtype == VG_BF16 && C % 8 == 0 && rows * C * 2 >= (int64_t)vg_sw().bn_wide_min;
}

// kind: VG_BN_PLAN_FORWARD or VG_BN_PLAN_APPLY (their grid caps differ); aligned16: the tensors allow 16-byte vectors
inline vg_bn_plan plan_stream(int kind, int dtype, int64_t rows, int C, int groups, bool aligned16) {
    const int64_t rows_per_group = rows / groups;
    const int max_wgs = kind == VG_BN_PLAN_FORWARD ? EW_FWD_WGS : EW_BWD_WGS;
    vg_bn_plan p = {};
    p.kind = kind;
    p.vec = stream_wide(dtype, rows, C) && aligned16 ? 8 : 4;
    const int cols = C / p.vec;
    const int ncol = cols < 256 ? cols : 256;
    const int rpp = 256 / ncol;
    p.threads_per_row = ncol;
    p.rows_per_pass = rpp;
    p.col_blocks = (cols + 255) / 256;
    p.groups = groups;
    const int64_t passes = (rows_per_group + rpp - 1) / rpp;
    int64_t cap = max_wgs / ((int64_t)groups * p.col_blocks);
    if (cap < 1) cap = 1;
    const int64_t blocks = passes < cap ? passes : cap;            // small tensors: one pass per workgroup
    const int64_t rpb = (passes + blocks - 1) / blocks * rpp;
    p.rows_per_block = (int)rpb;
    p.blocks_per_group = (int)((rows_per_group + rpb - 1) / rpb);
    return p;
}

// VW consecutive elements: loaded as one vector (kept packed while in flight), unpacked to floats where they are used
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
template <int V> struct IntC { static constexpr int value = V; };      // a uniform run-time choice made compile-time

template <int VW> __device__ __forceinline__ void load_coef(const float* __restrict__ p, float (&c)[VW]) {
#pragma unroll
    for (int k = 0; k < VW; k += 4) {
        const float4 r = *reinterpret_cast<const float4*>(p + k);
        c[k] = r.x; c[k + 1] = r.y; c[k + 2] = r.z; c[k + 3] = r.w;
    }
}

// the rows r0, r0 + rpp, ... < r1 and the channel offset of this thread (blockIdx: row block, column block, group); an idle
// thread gets an empty range and a valid channel offset -- no early exit, so that the kernel arguments arrive in one batch
template <int VW>
__device__ __forceinline__ void stream_range(int64_t rows, int C, int64_t rows_per_group, int rows_per_block, int& c,
                                             int& rpp, int64_t& r0, int64_t& r1) {
    const int cols = C / VW;
    const int cb = blockIdx.y * 256;
    const int ncol = min(256, cols - cb);
    rpp = 256 / ncol;
    const int tr = threadIdx.x / ncol, tc = threadIdx.x - tr * ncol;
    c = (cb + tc) * VW;
    const int64_t gbase = (int64_t)blockIdx.z * rows_per_group;
    const int64_t b0 = gbase + (int64_t)blockIdx.x * rows_per_block;
    r1 = min(min(rows, gbase + rows_per_group), b0 + (int64_t)rows_per_block);
    r0 = tr < rpp ? b0 + tr : r1;
}

template <int DT, int VW>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const void* __restrict__ x, void* __restrict__ y,
                                                         const float* __restrict__ scale,
                                                         const float* __restrict__ shift, int64_t rows, int C, int act,
                                                         float slope, int64_t rows_per_group, int rows_per_block,
                                                         int64_t gstride, uint8_t* __restrict__ y8) {
    int c, rpp;
    int64_t r, r1;
    stream_range<VW>(rows, C, rows_per_group, rows_per_block, c, rpp, r, r1);
    typedef typename RawVec<DT, VW>::type Raw;
    const int64_t step = (int64_t)rpp * C;
    int64_t off = r * C + c;
    float sc[VW], sh[VW];
    if (scale) {
        load_coef<VW>(scale + (int64_t)blockIdx.z * gstride + c, sc);
        load_coef<VW>(shift + (int64_t)blockIdx.z * gstride + c, sh);
    }
    // the activation and the activation-only mode are uniform: chosen once, outside the row loop
    auto run = [&](auto act_c, auto affine_c) {
        constexpr int ACT = decltype(act_c)::value;
        constexpr bool AFFINE = decltype(affine_c)::value;
        auto one = [&](int64_t o, const Raw& raw) {
            float f[VW];
            unpackv<DT, VW>(raw, f);
            if (AFFINE) {                                       // sc * x + sh, contracted: spelled out, see bn_act_bwd_apply_kernel
#pragma unroll
                for (int k = 0; k < VW; ++k) f[k] = __builtin_fmaf(sc[k], f[k], sh[k]);
            }
#pragma unroll
            for (int k = 0; k < VW; ++k) f[k] = act_fwd(f[k], ACT, slope);
            storev<DT, VW>(y, o, f);
            if (y8) {               // e4m3 twin of the activated tensor for an fp8 forward GEMM (same NHWC layout)
                // cast from the STORED value, as vg_cast_fp8 does: casting the f32 value directly rounds differently
                // wherever the bf16 rounding lands on an e4m3 midpoint (about 2 % of the elements)
                if constexpr (DT == VG_BF16) {
#pragma unroll
                    for (int k = 0; k < VW; ++k) f[k] = ElemT<VG_BF16>::to_f32(ElemT<VG_BF16>::from_f32(f[k]));
                }
                typedef __attribute__((ext_vector_type(VW / 4))) uint32_t W8;
                W8 w8;
#pragma unroll
                for (int k = 0; k < VW / 4; ++k) {
                    int w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * k], f[4 * k + 1], 0, false);
                    w = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * k + 2], f[4 * k + 3], w, true);
                    w8[k] = (uint32_t)w;
                }
                *reinterpret_cast<W8*>(y8 + o) = w8;
            }
        };
        for (; r + (EW_UNROLL - 1) * rpp < r1; r += EW_UNROLL * rpp, off += EW_UNROLL * step) {
            Raw v[EW_UNROLL];
#pragma unroll
            for (int u = 0; u < EW_UNROLL; ++u) v[u] = loadv<DT, VW>(x, off + u * step);
#pragma unroll
            for (int u = 0; u < EW_UNROLL; ++u) one(off + u * step, v[u]);
        }
        if (r < r1) {                                           // the last one to three rows of the row block, together as well
            Raw v[EW_UNROLL - 1];
#pragma unroll
            for (int u = 0; u < EW_UNROLL - 1; ++u)
                if (r + u * rpp < r1) v[u] = loadv<DT, VW>(x, off + u * step);
#pragma unroll
            for (int u = 0; u < EW_UNROLL - 1; ++u)
                if (r + u * rpp < r1) one(off + u * step, v[u]);
        }
    };
    auto with_act = [&](auto affine_c) {
        if (act == VG_ACT_RELU) run(IntC<VG_ACT_RELU>{}, affine_c);
        else if (act == VG_ACT_LRELU) run(IntC<VG_ACT_LRELU>{}, affine_c);
        else run(IntC<VG_ACT_NONE>{}, affine_c);
    };
    if (scale) with_act(IntC<1>{}); else with_act(IntC<0>{});
}

__global__ __launch_bounds__(FIN_CH * FIN_PL) void bn_bwd_finalize_kernel(
    const float* __restrict__ partial, int nparts, int C, double count, const float* __restrict__ gamma,
    const float* __restrict__ invstd, float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate,
    float* __restrict__ coef) {
    double s1, s2;
    int c;
    const bool lead = fin_lead(C, c);
    const float gm = lead_load(lead, gamma, c, 1.f), is = lead_load(lead, invstd, c, 0.f);
    const float dg = lead_load(lead && accumulate, dgamma, c, 0.f), db = lead_load(lead && accumulate, dbeta, c, 0.f);
    if (!slab_sums(partial, nparts, C, s1, s2, c)) return;
    const float fs1 = (float)s1, fs2 = (float)s2;
    if (dgamma) dgamma[c] = accumulate ? dg + fs2 : fs2;
    if (dbeta) dbeta[c] = accumulate ? db + fs1 : fs1;
    const float a = gm * is;
    coef[c] = a;
    coef[C + c] = (float)((double)a * s2 / count);
    coef[2 * C + c] = (float)((double)a * s1 / count);
}

template <int DT, int VW>
__global__ __launch_bounds__(256) void bn_act_bwd_apply_kernel(const void* __restrict__ x, const void* __restrict__ dy,
                                                               void* __restrict__ dx,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd,
                                                               const float* __restrict__ coef, int64_t rows, int C,
                                                               int act, float slope, int64_t rows_per_group,
                                                               int rows_per_block, int64_t gstride, int64_t cstride) {
    int c, rpp;
    int64_t r, r1;
    stream_range<VW>(rows, C, rows_per_group, rows_per_block, c, rpp, r, r1);
    typedef typename RawVec<DT, VW>::type Raw;
    const int64_t step = (int64_t)rpp * C;
    int64_t off = r * C + c;
    float sc[VW], sh[VW], mu[VW], is[VW], ca[VW], cbv[VW], cc[VW];
    const int64_t go = (int64_t)blockIdx.z * gstride + c;
    const float* cf = coef + (int64_t)blockIdx.z * cstride + c;
    load_coef<VW>(scale + go, sc);
    load_coef<VW>(shift + go, sh);
    load_coef<VW>(mean + go, mu);
    load_coef<VW>(invstd + go, is);
    load_coef<VW>(cf, ca);
    load_coef<VW>(cf + C, cbv);
    load_coef<VW>(cf + 2 * C, cc);
    auto run = [&](auto act_c) {                                // the activation is uniform: chosen once, outside the row loop
        constexpr int ACT = decltype(act_c)::value;
        auto one = [&](int64_t o, const Raw& rx, const Raw& rg) {
            float f[VW], d[VW], q[VW];
            unpackv<DT, VW>(rx, f);
            unpackv<DT, VW>(rg, d);
            // ca * act_bwd(sc * x + sh, dy) - cb * ((x - mu) * is) - cc with the two contractions the compiler has always made
            // here spelled out: left to -ffp-contract it fused the second one in the full trips and not in every lane of the
            // short last trip, and the same element came out one ulp apart depending on where its row fell in a row block
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                const float dz = act_bwd(__builtin_fmaf(sc[k], f[k], sh[k]), d[k], ACT, slope);
                const float xh = cbv[k] * ((f[k] - mu[k]) * is[k]);
                q[k] = __builtin_fmaf(ca[k], dz, -xh) - cc[k];
            }
            storev<DT, VW>(dx, o, q);
        };
        for (; r + (EW_UNROLL - 1) * rpp < r1; r += EW_UNROLL * rpp, off += EW_UNROLL * step) {
            Raw v[EW_UNROLL], g[EW_UNROLL];
#pragma unroll
            for (int u = 0; u < EW_UNROLL; ++u) { v[u] = loadv<DT, VW>(x, off + u * step); g[u] = loadv<DT, VW>(dy, off + u * step); }
#pragma unroll
            for (int u = 0; u < EW_UNROLL; ++u) one(off + u * step, v[u], g[u]);
        }
        if (r < r1) {                                           // the last one to three rows of the row block, together as well
            Raw v[EW_UNROLL - 1], g[EW_UNROLL - 1];
#pragma unroll
            for (int u = 0; u < EW_UNROLL - 1; ++u)
                if (r + u * rpp < r1) { v[u] = loadv<DT, VW>(x, off + u * step); g[u] = loadv<DT, VW>(dy, off + u * step); }
#pragma unroll
            for (int u = 0; u < EW_UNROLL - 1; ++u)
                if (r + u * rpp < r1) one(off + u * step, v[u], g[u]);
        }
    };
    if (act == VG_ACT_RELU) run(IntC<VG_ACT_RELU>{});
    else if (act == VG_ACT_LRELU) run(IntC<VG_ACT_LRELU>{});
    else run(IntC<VG_ACT_NONE>{});
}

// ---- train-mode BatchNorm finalize + normalise + activation in ONE launch (bf16, small statistics slabs) ----------
// bn_finalize_grouped_kernel is a 5 us launch whose only output is 4 C floats; for layers whose slab is small
// (<= 200 rows per group, tensor <= 9 MB) every workgroup of the elementwise pass can afford to redo it: a workgroup of 1024 threads
// owns 64 channels of a block of rows, sums the slab rows of its group for those channels (16 part lanes x 64
// channels, double, fixed order -- every workgroup of a channel slice computes bit-identical coefficients), keeps
// scale / shift in LDS and applies them.  The workgroups of row block 0 also publish the coefficients
// ([groups][4][C], what the backward pass reads) and update the running statistics, group after group.
constexpr int FF_CH = 64, FF_PL = 16, FF_TH = FF_CH * FF_PL, FF_MAXPARTS = 200;
constexpr int64_t FF_MAXBYTES = 9ll << 20;       // tensor size up to which re-deriving the coefficients per workgroup pays

// A part lane's slab rows (pl, pl + 16, ...: at most FF_TRIPS), all loaded before the first is added: the load-add loop was
// one memory round trip per row, up to 13 in a row before a workgroup touched its tensor.  Rows beyond nparts come back as
// +0 (a sum that started at +0 is never -0: adding them changes no bit); the adds stay in row order.
constexpr int FF_TRIPS = (FF_MAXPARTS + FF_PL - 1) / FF_PL;

// -> a part lane's sums: T trips' loads (through a SlabBuf: rows beyond the slab are +0), then the adds
template <int T>
__device__ __forceinline__ void ff_lane_sums(const SlabBuf& sb, int c, double& a, double& b) {
    const int pl = threadIdx.x / FF_CH;
    float x[T], y[T];
#pragma unroll
    for (int k = 0; k < T; ++k) sb.load(pl + k * FF_PL, c, x[k], y[k]);
    a = 0.0; b = 0.0;
#pragma unroll
    for (int k = 0; k < T; ++k) { a += (double)x[k]; b += (double)y[k]; }
}

// -> the slice's sums in every thread of channel ch: 16 part lanes in double, combined in lane order through LDS
__device__ __forceinline__ void ff_slice_sums(const float* __restrict__ slabs, int nparts, int C, int c0,
                                              double (*red)[FF_CH][2], double& s1, double& s2) {
    const int ch = threadIdx.x & (FF_CH - 1), pl = threadIdx.x / FF_CH;
    const SlabBuf sb(slabs, nparts, C);
    double a, b;
    if (nparts <= FF_PL) ff_lane_sums<1>(sb, c0 + ch, a, b);               // no more loads than the slab has rows per lane
    else if (nparts <= 2 * FF_PL) ff_lane_sums<2>(sb, c0 + ch, a, b);
    else if (nparts <= 4 * FF_PL) ff_lane_sums<4>(sb, c0 + ch, a, b);
    else if (nparts <= 8 * FF_PL) ff_lane_sums<8>(sb, c0 + ch, a, b);
    else ff_lane_sums<FF_TRIPS>(sb, c0 + ch, a, b);
    red[pl][ch][0] = a;
    red[pl][ch][1] = b;
    __syncthreads();
    s1 = 0.0; s2 = 0.0;
#pragma unroll
    for (int k = 0; k < FF_PL; ++k) { s1 += red[k][ch][0]; s2 += red[k][ch][1]; }
    __syncthreads();                                           // red[] is reused by the next group (publisher blocks)
}

__device__ __forceinline__ void ff_slice_stats(const float* __restrict__ slabs, int nparts, int C, int c0, double count,
                                               double (*red)[FF_CH][2], double& mu_out, double& var_out) {
    double s1, s2;
    ff_slice_sums(slabs, nparts, C, c0, red, s1, s2);
    const double mu = s1 / count;
    double var = s2 / count - mu * mu;
    if (var < 0.0) var = 0.0;
    mu_out = mu;
    var_out = var;
}

__global__ __launch_bounds__(FF_TH) void bn_fin_act_fwd_kernel(
    const uint16_t* __restrict__ x, uint16_t* __restrict__ y, const float* __restrict__ stats, int nparts, int groups,
    int C, double count, const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ rmean,
    float* __restrict__ rvar, float momentum, float eps, float* __restrict__ coeffs, int64_t rows_per_group,
    int rows_per_block, int act, float slope) {
    __shared__ double red[FF_PL][FF_CH][2];
    __shared__ float s_sc[FF_CH], s_sh[FF_CH];
    const int tid = threadIdx.x, ch = tid & (FF_CH - 1);
    const int c0 = blockIdx.y * FF_CH, grp = blockIdx.z;
    const bool lead = tid < FF_CH && c0 + ch < C;              // one thread per channel of the slice
    const float gm = (lead && gamma) ? gamma[c0 + ch] : 1.f, bt = (lead && beta) ? beta[c0 + ch] : 0.f;
    if (blockIdx.x == 0 && grp == 0) {
        // publisher of this channel slice: every group's coefficients, running statistics in group order
        float rm = (lead && rmean) ? rmean[c0 + ch] : 0.f, rv = (lead && rmean) ? rvar[c0 + ch] : 0.f;
        for (int g = 0; g < groups; ++g) {
            double mu, var;
            ff_slice_stats(stats + (int64_t)g * nparts * 2 * C, nparts, C, c0, count, red, mu, var);
            if (lead) {
                const float is = (float)(1.0 / sqrt(var + (double)eps));
                const float muf = (float)mu, sc = gm * is, sh = bt - muf * sc;
                float* co = coeffs + (int64_t)g * 4 * C + c0 + ch;
                co[0] = muf; co[C] = is; co[2 * C] = sc; co[3 * C] = sh;
                if (g == 0) { s_sc[ch] = sc; s_sh[ch] = sh; }
                if (rmean) {
                    const double unbiased = count > 1.0 ? var * (count / (count - 1.0)) : var;
                    rm = (1.f - momentum) * rm + momentum * muf;
                    rv = (1.f - momentum) * rv + momentum * (float)unbiased;
                }
            }
        }
        if (lead && rmean) { rmean[c0 + ch] = rm; rvar[c0 + ch] = rv; }
    } else {
        double mu, var;
        ff_slice_stats(stats + (int64_t)grp * nparts * 2 * C, nparts, C, c0, count, red, mu, var);
        if (lead) {
            const float is = (float)(1.0 / sqrt(var + (double)eps));
            const float muf = (float)mu, sc = gm * is;
            s_sc[ch] = sc;
            s_sh[ch] = bt - muf * sc;
        }
    }
    __syncthreads();
    // ---- apply: a thread owns 8 channels (16 bytes) of a row; 8 threads per row, 128 rows per pass ----
    const int u8 = (tid & 7) * 8, rl = tid >> 3;
    float sc[8], sh[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { sc[k] = s_sc[u8 + k]; sh[k] = s_sh[u8 + k]; }
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < rows_per_group ? r0 + rows_per_block : rows_per_group;
    const int64_t base = (int64_t)grp * rows_per_group;
    if (c0 + u8 < C) {
        for (int64_t r = r0 + rl; r < r1; r += FF_TH / 8) {
            const int64_t off = (base + r) * C + c0 + u8;
            const u32x4 v = *reinterpret_cast<const u32x4*>(x + off);
            u32x4 o;
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) {
                const float lo = act_fwd(sc[2 * k2] * __uint_as_float(v[k2] << 16) + sh[2 * k2], act, slope);
                const float hi = act_fwd(sc[2 * k2 + 1] * __uint_as_float(v[k2] & 0xffff0000u) + sh[2 * k2 + 1], act, slope);
                o[k2] = (uint32_t)ElemT<VG_BF16>::from_f32(lo) | ((uint32_t)ElemT<VG_BF16>::from_f32(hi) << 16);
            }
            *reinterpret_cast<u32x4*>(y + off) = o;
        }
    }
}

inline bool bn_fin_fwd_ok(int nparts_per_group, int groups, int C, int64_t rows, int dtype) {
    const int mode = vg_sw().bn_fused_fwd;
    // measured per shape (tools/bn_fwd_bench.py, S=64 B=128): wins 1-3 us per layer up to 8.4 MB / 196 slab rows
    // (G0 7.2 -> 4.5, D3 6.2 -> 4.3, E3 5.5 -> 3.8 us), loses beyond (G2 16.8 MB 13.4 -> 15.0, D1 256 slab rows 9.1 -> 11.4)
    return mode != 0 && dtype == VG_BF16 && C % FF_CH == 0 && groups >= 1 && rows % groups == 0 &&
           nparts_per_group > 0 && nparts_per_group <= FF_MAXPARTS && rows * C * 2 <= FF_MAXBYTES;
}

// the one-launch forms (forward and backward twin share it): fused = 0 and no geometry where the shape is refused
inline vg_bn_plan plan_fused(int nparts_per_group, int groups, int C, int64_t rows, int dtype) {
    vg_bn_plan p = {};
    p.kind = VG_BN_PLAN_FUSED;
    if (!bn_fin_fwd_ok(nparts_per_group, groups, C, rows, dtype)) return p;
    const int64_t rpg = rows / groups;
    // ~512 workgroups in all; whole passes of 128 rows per workgroup
    const int slices = C / FF_CH;
    int64_t want = 512 / (slices * groups);
    if (want < 1) want = 1;
    int64_t rpb = (rpg + want - 1) / want;
    rpb = (rpb + 127) / 128 * 128;
    p.fused = 1;
    p.vec = 8;
    p.threads_per_row = 8;
    p.rows_per_pass = FF_TH / 8;
    p.rows_per_block = (int)rpb;
    p.blocks_per_group = (int)((rpg + rpb - 1) / rpb);
    p.col_blocks = slices;
    p.groups = groups;
    return p;
}

// ---- backward twin: bn_bwd_finalize_grouped + bn_act_bwd_apply in one launch (same eligibility, same structure) ----
// Every workgroup sums the column-reduce partials (sum dz | sum dz * xhat) of its group for its 64 channels, forms the
// three coefficients of bn_bwd_finalize_grouped_kernel and applies dx = a * dz - b * xhat - c; the workgroups of row
// block 0 accumulate dgamma / dbeta, group after group.
__global__ __launch_bounds__(FF_TH) void bn_bwd_fin_apply_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy, uint16_t* __restrict__ dx,
    const float* __restrict__ partial, int nparts, int groups, int C, double count, const float* __restrict__ gamma,
    const float* __restrict__ coeffs, float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate,
    int64_t rows_per_group, int rows_per_block, int act, float slope) {
    __shared__ double red[FF_PL][FF_CH][2];
    __shared__ float s_co[7][FF_CH];                            // mean | invstd | scale | shift | a | b | c
    const int tid = threadIdx.x, ch = tid & (FF_CH - 1);
    const int c0 = blockIdx.y * FF_CH, grp = blockIdx.z;
    const bool lead = tid < FF_CH && c0 + ch < C;
    const float gm = (lead && gamma) ? gamma[c0 + ch] : 1.f;
    // the forward coefficients of the group this workgroup applies (the publisher: group 0 = grp), loaded at entry with the
    // slab rows and not one more round trip after the sums
    float co[4] = {0.f, 0.f, 0.f, 0.f};
    if (lead) {
        const float* cp = coeffs + (int64_t)grp * 4 * C + c0 + ch;
        co[0] = cp[0]; co[1] = cp[C]; co[2] = cp[2 * C]; co[3] = cp[3 * C];
    }
    auto publish_coef = [&](double s1, double s2) {             // lead threads: this group's coefficients into LDS
        const float is = co[1];
        const float a = gm * is;
        s_co[0][ch] = co[0]; s_co[1][ch] = is; s_co[2][ch] = co[2]; s_co[3][ch] = co[3];
        s_co[4][ch] = a;
        s_co[5][ch] = (float)((double)a * s2 / count);
        s_co[6][ch] = (float)((double)a * s1 / count);
    };
    if (blockIdx.x == 0 && grp == 0) {
        float dg = (lead && dgamma && accumulate) ? dgamma[c0 + ch] : 0.f;
        float db = (lead && dbeta && accumulate) ? dbeta[c0 + ch] : 0.f;
        for (int g = 0; g < groups; ++g) {                      // dgamma / dbeta accumulate in group order
            double s1, s2;
            ff_slice_sums(partial + (int64_t)g * nparts * 2 * C, nparts, C, c0, red, s1, s2);
            if (lead) {
                if (g == 0) publish_coef(s1, s2);               // this workgroup applies group 0's rows
                const bool acc = accumulate || g > 0;
                dg = acc ? dg + (float)s2 : (float)s2;
                db = acc ? db + (float)s1 : (float)s1;
            }
        }
        if (lead) {
            if (dgamma) dgamma[c0 + ch] = dg;
            if (dbeta) dbeta[c0 + ch] = db;
        }
    } else {
        double s1, s2;
        ff_slice_sums(partial + (int64_t)grp * nparts * 2 * C, nparts, C, c0, red, s1, s2);
        if (lead) publish_coef(s1, s2);
    }
    __syncthreads();
    const int u8 = (tid & 7) * 8, rl = tid >> 3;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < rows_per_group ? r0 + rows_per_block : rows_per_group;
    const int64_t base = (int64_t)grp * rows_per_group;
    if (c0 + u8 < C) {
        for (int64_t r = r0 + rl; r < r1; r += FF_TH / 8) {
            const int64_t off = (base + r) * C + c0 + u8;
            const u32x4 v = *reinterpret_cast<const u32x4*>(x + off);
            const u32x4 gq = *reinterpret_cast<const u32x4*>(dy + off);
            u32x4 o;
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) {
                float ov[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int k = u8 + 2 * k2 + h;
                    const float yv = __uint_as_float(h ? (v[k2] & 0xffff0000u) : (v[k2] << 16));
                    const float gr = __uint_as_float(h ? (gq[k2] & 0xffff0000u) : (gq[k2] << 16));
                    ov[h] = s_co[4][k] * act_bwd(s_co[2][k] * yv + s_co[3][k], gr, act, slope) -
                            s_co[5][k] * ((yv - s_co[0][k]) * s_co[1][k]) - s_co[6][k];
                }
                o[k2] = (uint32_t)ElemT<VG_BF16>::from_f32(ov[0]) | ((uint32_t)ElemT<VG_BF16>::from_f32(ov[1]) << 16);
            }
            *reinterpret_cast<u32x4*>(dx + off) = o;
        }
    }
}

template <int DT>
__global__ __launch_bounds__(256) void act_bwd_kernel(const void* __restrict__ x, const void* __restrict__ dy,
                                                      void* __restrict__ dx, int64_t nvec, int act, float slope) {
    auto one = [&](int64_t i, const float4& v, const float4& g) {
        float4 o;
        o.x = act_bwd(v.x, g.x, act, slope); o.y = act_bwd(v.y, g.y, act, slope);
        o.z = act_bwd(v.z, g.z, act, slope); o.w = act_bwd(v.w, g.w, act, slope);
        store4<DT>(dx, i * 4, o);
    };
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {
        float4 v[4], g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { v[u] = load4<DT>(x, (i + u * stride) * 4); g[u] = load4<DT>(dy, (i + u * stride) * 4); }
#pragma unroll
        for (int u = 0; u < 4; ++u) one(i + u * stride, v[u], g[u]);
    }
    for (; i < nvec; i += stride) one(i, load4<DT>(x, i * 4), load4<DT>(dy, i * 4));
}

__global__ __launch_bounds__(FIN_CH * FIN_PL) void bias_finalize_kernel(const float* __restrict__ partial, int nparts,
                                                                        int C, int NC, float* __restrict__ dbias,
                                                                        int accumulate) {
    double s1, s2;
    int c;
    const bool lead = fin_lead(C, c);
    const float d0 = lead_load(lead && accumulate && c < NC, dbias, c, 0.f);
    if (!slab_sums(partial, nparts, C, s1, s2, c)) return;
    if (c >= NC) return;
    dbias[c] = accumulate ? d0 + (float)s1 : (float)s1;
}

inline int ew_blocks(int64_t nvec) {
    int64_t b = (nvec + 255) / 256;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (int)b;
}

inline int check_rows_c(const void* x, int64_t rows, int C, int dtype) {
    VG_CHECK_ARG(x != nullptr && rows > 0 && C > 0, VG_EINVAL);
    VG_CHECK_ARG(dtype == VG_F32 || dtype == VG_BF16, VG_ENOSUP);
    VG_CHECK_ARG(C % 4 == 0, VG_EALIGN);
    VG_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 7u) == 0, VG_EALIGN);
    return 0;
}

// groups > 1: `rows` = groups * rows_per_group; the slabs of group g are parts [g*nparts_out, (g+1)*nparts_out)
template <int MODE>
int launch_reduce(const void* x, const void* dy, const float* scale, const float* shift, const float* mean,
                  const float* invstd, int64_t rows, int C, int act, float slope, float* partial, int capacity,
                  int* nparts_out, int dtype, hipStream_t s, int groups = 1, int64_t gstride = 0) {
    VG_CHECK_ARG(groups >= 1 && rows % groups == 0, VG_EINVAL);
    const int64_t rpg = rows / groups;
    const vg_bn_plan p = plan_reduce(rpg, C, groups);
    if (nparts_out) *nparts_out = p.blocks_per_group;
    VG_CHECK_ARG(partial != nullptr && capacity >= p.blocks_per_group * groups, VG_EINVAL);
    dim3 grid(p.blocks_per_group * p.groups, p.col_blocks);
    if (dtype == VG_F32)
        vg_launch_timed(4, (col_reduce_kernel<VG_F32, MODE>), grid, dim3(256), 0, s, x, dy, scale, shift, mean, invstd,
                           rows, C, act, slope, partial, p.rows_per_block, rpg, p.blocks_per_group, gstride);
    else
        vg_launch_timed(4, (col_reduce_kernel<VG_BF16, MODE>), grid, dim3(256), 0, s, x, dy, scale, shift, mean, invstd,
                           rows, C, act, slope, partial, p.rows_per_block, rpg, p.blocks_per_group, gstride);
    return VG_LAUNCH_RC();
}

}  // namespace

extern "C" int vg_bn_finalize(const float* stats, int nparts, int C, int64_t count, const float* gamma,
                              const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                              float* mean, float* invstd, float* scale, float* shift, void* stream) {
    VG_CHECK_ARG(stats && nparts > 0 && C > 0 && count > 0 && mean && invstd && scale && shift, VG_EINVAL);
    VG_CHECK_ARG(slab_fits(nparts, C), VG_ENOSUP);
    VG_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), VG_EINVAL);
    vg_launch_timed(4, bn_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_PL), 0, vg_stream(stream), stats, nparts, C,
                       (double)count, gamma, beta, running_mean, running_var, momentum, eps, mean, invstd, scale,
                       shift);
    return VG_LAUNCH_RC();
}

extern "C" int vg_bn_finalize_grouped(const float* stats, int nparts_per_group, int groups, int C,
                                      int64_t count_per_group, const float* gamma, const float* beta,
                                      float* running_mean, float* running_var, float momentum, float eps,
                                      float* coeffs, void* stream) {
    VG_CHECK_ARG(stats && coeffs && nparts_per_group > 0 && groups > 0 && C > 0 && count_per_group > 0, VG_EINVAL);
    VG_CHECK_ARG(slab_fits(nparts_per_group, C), VG_ENOSUP);
    VG_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), VG_EINVAL);
    vg_launch_timed(4, bn_finalize_grouped_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_PL), 0,
                       vg_stream(stream), stats, nparts_per_group, groups, C, (double)count_per_group, gamma, beta,
                       running_mean, running_var, momentum, eps, coeffs);
    return VG_LAUNCH_RC();
}

extern "C" int vg_bn_backward_finalize_grouped(const float* partial, int nparts_per_group, int groups, int C,
                                               int64_t count_per_group, const float* gamma, const float* coeffs,
                                               float* dgamma, float* dbeta, int accumulate, float* coef,
                                               void* stream) {
    VG_CHECK_ARG(partial && coeffs && coef && nparts_per_group > 0 && groups > 0 && C > 0 && count_per_group > 0,
                 VG_EINVAL);
    VG_CHECK_ARG(slab_fits(nparts_per_group, C), VG_ENOSUP);
    vg_launch_timed(4, bn_bwd_finalize_grouped_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_PL), 0,
                       vg_stream(stream), partial, nparts_per_group, groups, C, (double)count_per_group, gamma, coeffs,
                       dgamma, dbeta, accumulate, coef);
    return VG_LAUNCH_RC();
}

extern "C" int vg_slab_sums(const float* slabs, int nparts, int C, double* sums, void* stream) {
    VG_CHECK_ARG(slabs && sums && nparts > 0 && C > 0, VG_EINVAL);
    VG_CHECK_ARG(slab_fits(nparts, C), VG_ENOSUP);
    vg_launch_timed(4, slab_sums_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_PL), 0, vg_stream(stream),
                       slabs, nparts, C, sums);
    return VG_LAUNCH_RC();
}

extern "C" int vg_bn_finalize_sums(const double* sums, int C, int64_t count, const float* gamma, const float* beta,
                                   float* running_mean, float* running_var, float momentum, float eps, float* mean,
                                   float* invstd, float* scale, float* shift, void* stream) {
    VG_CHECK_ARG(sums && C > 0 && count > 0 && mean && invstd && scale && shift, VG_EINVAL);
    VG_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), VG_EINVAL);
    vg_launch_timed(4, bn_finalize_sums_kernel, dim3((C + 255) / 256), dim3(256), 0, vg_stream(stream), sums, C,
                       (double)count, gamma, beta, running_mean, running_var, momentum, eps, mean, invstd, scale,
                       shift);
    return VG_LAUNCH_RC();
}

extern "C" int vg_bn_backward_finalize_sums(const double* global_sums, const double* local_sums, int C, int64_t count,
                                            const float* gamma, const float* invstd, float* dgamma, float* dbeta,
                                            int accumulate, float* coef, void* stream) {
    VG_CHECK_ARG(global_sums && local_sums && C > 0 && count > 0 && invstd && coef, VG_EINVAL);
    vg_launch_timed(4, bn_bwd_finalize_sums_kernel, dim3((C + 255) / 256), dim3(256), 0, vg_stream(stream),
                       global_sums, local_sums, C, (double)count, gamma, invstd, dgamma, dbeta, accumulate, coef);
    return VG_LAUNCH_RC();
}

extern "C" int vg_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, float eps, int C, float* scale, float* shift,
                                 void* stream) {
    VG_CHECK_ARG(running_mean && running_var && scale && shift && C > 0, VG_EINVAL);
    vg_launch_timed(4, bn_eval_kernel, dim3((C + 63) / 64), dim3(64), 0, vg_stream(stream), gamma, beta, running_mean,
                       running_var, eps, C, scale, shift);
    return VG_LAUNCH_RC();
}

extern "C" int vg_bn_launch_plan(int kind, int64_t rows, int C, int groups, int dtype, int aligned16, int nparts_per_group,
                                 vg_bn_plan* out) {
    VG_CHECK_ARG(out != nullptr && rows > 0 && C > 0, VG_EINVAL);
    VG_CHECK_ARG(kind >= VG_BN_PLAN_REDUCE && kind <= VG_BN_PLAN_FUSED, VG_EINVAL);
    VG_CHECK_ARG(dtype == VG_F32 || dtype == VG_BF16, VG_ENOSUP);
    VG_CHECK_ARG(C % 4 == 0, VG_EALIGN);
    VG_CHECK_ARG(groups >= 1 && rows % groups == 0, VG_EINVAL);
    if (kind == VG_BN_PLAN_REDUCE) *out = plan_reduce(rows / groups, C, groups);
    else if (kind == VG_BN_PLAN_FUSED) *out = plan_fused(nparts_per_group, groups, C, rows, dtype);
    else *out = plan_stream(kind, dtype, rows, C, groups, aligned16 != 0);
    return 0;
}

extern "C" int vg_bn_finalize_act_forward(const void* x, void* y, const float* stats, int nparts_per_group, int groups,
                                          int C, int64_t rows, const float* gamma, const float* beta,
                                          float* running_mean, float* running_var, float momentum, float eps,
                                          float* coeffs, int act, float slope, int dtype, void* stream) {
    VG_CHECK_ARG(x && y && stats && coeffs && rows > 0 && C > 0, VG_EINVAL);
    VG_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), VG_EINVAL);
    VG_CHECK_ARG(vg_aligned16(x) && vg_aligned16(y), VG_EALIGN);
    const vg_bn_plan p = plan_fused(nparts_per_group, groups, C, rows, dtype);
    if (!p.fused || !slab_fits(nparts_per_group, C)) return VG_ENOSUP;
    const int64_t rpg = rows / groups;
    vg_launch_timed(4, bn_fin_act_fwd_kernel, dim3(p.blocks_per_group, p.col_blocks, p.groups), dim3(FF_TH), 0, vg_stream(stream),
                       reinterpret_cast<const uint16_t*>(x), reinterpret_cast<uint16_t*>(y), stats, nparts_per_group, groups,
                       C, (double)rpg, gamma, beta, running_mean, running_var, momentum, eps, coeffs, rpg, p.rows_per_block, act,
                       slope);
    return VG_LAUNCH_RC();
}

extern "C" int vg_bn_backward_finalize_apply(const void* x, const void* dy, void* dx, const float* partial,
                                             int nparts_per_group, int groups, int C, int64_t rows, const float* gamma,
                                             const float* coeffs, float* dgamma, float* dbeta, int accumulate, int act,
                                             float slope, int dtype, void* stream) {
    VG_CHECK_ARG(x && dy && dx && partial && coeffs && rows > 0 && C > 0, VG_EINVAL);
    VG_CHECK_ARG(vg_aligned16(x) && vg_aligned16(dy) && vg_aligned16(dx), VG_EALIGN);
    const vg_bn_plan p = plan_fused(nparts_per_group, groups, C, rows, dtype);
    if (!p.fused || !slab_fits(nparts_per_group, C)) return VG_ENOSUP;
    const int64_t rpg = rows / groups;
    vg_launch_timed(4, bn_bwd_fin_apply_kernel, dim3(p.blocks_per_group, p.col_blocks, p.groups), dim3(FF_TH), 0, vg_stream(stream),
                       reinterpret_cast<const uint16_t*>(x), reinterpret_cast<const uint16_t*>(dy),
                       reinterpret_cast<uint16_t*>(dx), partial, nparts_per_group, groups, C, (double)rpg, gamma, coeffs,
                       dgamma, dbeta, accumulate, rpg, p.rows_per_block, act, slope);
    return VG_LAUNCH_RC();
}

extern "C" int vg_bn_act_forward_fp8(const void* x, void* y, void* y8, const float* scale, const float* shift, int64_t rows,
                                     int C, int act, float slope, int groups, int64_t gstride, int dtype, void* stream);

extern "C" int vg_bn_act_forward(const void* x, void* y, const float* scale, const float* shift, int64_t rows, int C,
                                 int act, float slope, int groups, int64_t gstride, int dtype, void* stream) {
    return vg_bn_act_forward_fp8(x, y, nullptr, scale, shift, rows, C, act, slope, groups, gstride, dtype, stream);
}

extern "C" int vg_bn_act_forward_fp8(const void* x, void* y, void* y8, const float* scale, const float* shift, int64_t rows,
                                     int C, int act, float slope, int groups, int64_t gstride, int dtype, void* stream) {
    int rc = check_rows_c(x, rows, C, dtype);
    if (rc) return rc;
    VG_CHECK_ARG(y != nullptr && (scale == nullptr) == (shift == nullptr), VG_EINVAL);
    VG_CHECK_ARG(groups >= 1 && rows % groups == 0, VG_EINVAL);
    VG_CHECK_ARG(y8 == nullptr || (dtype == VG_BF16 && (reinterpret_cast<uintptr_t>(y8) & 3u) == 0), VG_EINVAL);
    const int64_t rpg = rows / groups;
    const hipStream_t s = vg_stream(stream);
    uint8_t* twin = reinterpret_cast<uint8_t*>(y8);
    // 16-byte vectors of bf16 need 8 | C and 16-byte aligned tensors (8-byte aligned twin); otherwise 8-byte vectors
    const vg_bn_plan p = plan_stream(VG_BN_PLAN_FORWARD, dtype, rows, C, groups,
                                     vg_aligned16(x) && vg_aligned16(y) && (reinterpret_cast<uintptr_t>(y8) & 7u) == 0);
    const bool wide = p.vec == 8;
    const dim3 grid(p.blocks_per_group, p.col_blocks, p.groups);
    if (dtype == VG_F32)
        vg_launch_timed(4, (bn_act_fwd_kernel<VG_F32, 4>), grid, dim3(256), 0, s, x, y, scale, shift, rows, C, act, slope,
                           rpg, p.rows_per_block, gstride, twin);
    else if (wide)
        vg_launch_timed(4, (bn_act_fwd_kernel<VG_BF16, 8>), grid, dim3(256), 0, s, x, y, scale, shift, rows, C, act, slope,
                           rpg, p.rows_per_block, gstride, twin);
    else
        vg_launch_timed(4, (bn_act_fwd_kernel<VG_BF16, 4>), grid, dim3(256), 0, s, x, y, scale, shift, rows, C, act, slope,
                           rpg, p.rows_per_block, gstride, twin);
    return VG_LAUNCH_RC();
}

extern "C" int vg_channel_stats(const void* x, int64_t rows, int C, float* stats, int stats_capacity,
                                int* nparts_out, int dtype, void* stream) {
    int rc = check_rows_c(x, rows, C, dtype);
    if (rc) return rc;
    return launch_reduce<0>(x, nullptr, nullptr, nullptr, nullptr, nullptr, rows, C, 0, 0.f, stats, stats_capacity,
                            nparts_out, dtype, vg_stream(stream));
}

extern "C" int vg_bn_act_backward_reduce(const void* x, const void* dy, const float* scale, const float* shift,
                                         const float* mean, const float* invstd, int64_t rows, int C, int act,
                                         float slope, float* partial, int partial_capacity, int* nparts_out,
                                         int groups, int64_t gstride, int dtype, void* stream) {
    int rc = check_rows_c(x, rows, C, dtype);
    if (rc) return rc;
    VG_CHECK_ARG(dy && scale && shift && mean && invstd, VG_EINVAL);
    return launch_reduce<1>(x, dy, scale, shift, mean, invstd, rows, C, act, slope, partial, partial_capacity,
                            nparts_out, dtype, vg_stream(stream), groups, gstride);
}

extern "C" int vg_bn_backward_finalize(const float* partial, int nparts, int C, int64_t count, const float* gamma,
                                       const float* invstd, float* dgamma, float* dbeta, int accumulate, float* coef,
                                       void* stream) {
    VG_CHECK_ARG(partial && nparts > 0 && C > 0 && count > 0 && invstd && coef, VG_EINVAL);
    VG_CHECK_ARG(slab_fits(nparts, C), VG_ENOSUP);
    vg_launch_timed(4, bn_bwd_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_PL), 0, vg_stream(stream), partial, nparts, C,
                       (double)count, gamma, invstd, dgamma, dbeta, accumulate, coef);
    return VG_LAUNCH_RC();
}

extern "C" int vg_bn_act_backward_apply(const void* x, const void* dy, void* dx, const float* scale,
                                        const float* shift, const float* mean, const float* invstd, const float* coef,
                                        int64_t rows, int C, int act, float slope, int groups, int64_t gstride,
                                        int64_t cstride, int dtype, void* stream) {
    int rc = check_rows_c(x, rows, C, dtype);
    if (rc) return rc;
    VG_CHECK_ARG(dy && dx && scale && shift && mean && invstd && coef, VG_EINVAL);
    VG_CHECK_ARG(groups >= 1 && rows % groups == 0, VG_EINVAL);
    const int64_t rpg = rows / groups;
    const hipStream_t s = vg_stream(stream);
    const vg_bn_plan p = plan_stream(VG_BN_PLAN_APPLY, dtype, rows, C, groups,
                                     vg_aligned16(x) && vg_aligned16(dy) && vg_aligned16(dx));
    const bool wide = p.vec == 8;
    const dim3 grid(p.blocks_per_group, p.col_blocks, p.groups);
    if (dtype == VG_F32)
        vg_launch_timed(4, (bn_act_bwd_apply_kernel<VG_F32, 4>), grid, dim3(256), 0, s, x, dy, dx, scale, shift, mean, invstd,
                           coef, rows, C, act, slope, rpg, p.rows_per_block, gstride, cstride);
    else if (wide)
        vg_launch_timed(4, (bn_act_bwd_apply_kernel<VG_BF16, 8>), grid, dim3(256), 0, s, x, dy, dx, scale, shift, mean, invstd,
                           coef, rows, C, act, slope, rpg, p.rows_per_block, gstride, cstride);
    else
        vg_launch_timed(4, (bn_act_bwd_apply_kernel<VG_BF16, 4>), grid, dim3(256), 0, s, x, dy, dx, scale, shift, mean, invstd,
                           coef, rows, C, act, slope, rpg, p.rows_per_block, gstride, cstride);
    return VG_LAUNCH_RC();
}

extern "C" int vg_act_backward(const void* x, const void* dy, void* dx, int64_t n, int act, float slope, int dtype,
                               void* stream) {
    VG_CHECK_ARG(x && dy && dx && n > 0 && n % 4 == 0, VG_EINVAL);
    VG_CHECK_ARG(dtype == VG_F32 || dtype == VG_BF16, VG_ENOSUP);
    const int64_t nvec = n / 4;
    if (dtype == VG_F32)
        vg_launch_timed(4, act_bwd_kernel<VG_F32>, dim3(ew_blocks(nvec)), dim3(256), 0, vg_stream(stream), x, dy, dx,
                           nvec, act, slope);
    else
        vg_launch_timed(4, act_bwd_kernel<VG_BF16>, dim3(ew_blocks(nvec)), dim3(256), 0, vg_stream(stream), x, dy, dx,
                           nvec, act, slope);
    return VG_LAUNCH_RC();
}

extern "C" int vg_bias_grad(const void* dy, int64_t rows, int C, int NC, float* dbias, int accumulate, float* ws,
                            int ws_capacity, int dtype, void* stream) {
    int rc = check_rows_c(dy, rows, C, dtype);
    if (rc) return rc;
    VG_CHECK_ARG(dbias && ws && NC > 0 && NC <= C, VG_EINVAL);
    VG_CHECK_ARG(slab_fits(plan_reduce(rows, C, 1).blocks_per_group, C), VG_ENOSUP);
    int nparts = 0;
    rc = launch_reduce<0>(dy, nullptr, nullptr, nullptr, nullptr, nullptr, rows, C, 0, 0.f, ws, ws_capacity, &nparts,
                          dtype, vg_stream(stream));
    if (rc) return rc;
    vg_launch_timed(4, bias_finalize_kernel, dim3((C + FIN_CH - 1) / FIN_CH), dim3(FIN_CH * FIN_PL), 0, vg_stream(stream), ws, nparts, C, NC,
                       dbias, accumulate);
    return VG_LAUNCH_RC();
}
