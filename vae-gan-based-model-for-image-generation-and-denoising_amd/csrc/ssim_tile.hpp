// The SSIM tile pass: the one statement of what ssimloss.hip (single scale, forward and backward in one launch) and
// msssim.hip (every level of the pyramid, forward and backward launches) do to a 32 x 32 tile of one plane.  Included by
// both inside their anonymous namespace, after common.hpp and <cmath>.  The kernels keep their own __shared__ arrays,
// their index computation and their stores; the pieces below work on the LDS pointers they are handed:
//
//   ssim_window        the normalised 11-tap Gaussian (sigma 1.5), built in f64 on the host
//   ssim_stage_shift   52 x 52 of u and v into LDS, minus ONE constant per tile and input; returns the constants
//   ssim_own_pixels    the thread's own four pixels of the tile (u - cu, v - cv), for the last step
//   ssim_fwd_rows      forward row pass: five moments, [52][42]
//   ssim_fwd_cols      forward column pass [42][42], the pointwise step (S or cs), the three derivative maps; returns the
//                      thread's f64 sum of the map over the tile's own interior pixels
//   ssim_tile_sum      that sum over the workgroup, as the f32 partial
//   ssim_bwd_rows      backward row pass: the three derivative maps, [42][32]
//   ssim_bwd_cols      backward column pass: wsum[3][4] of the thread's own four pixels
//   ssim_grad_pixel    coef (w * Dm + 2 u w * Du + v w * Dc) of one pixel
//
// With u = (a + 1) / 2, v = (b + 1) / 2, g the window, w = g (x) g, over the interior pixels p in [5, H - 5) x [5, W - 5):
//   mu_u = sum w u, mu_v = sum w v, s_uu = sum w u^2 - mu_u^2, s_vv likewise, s_uv = sum w u v - mu_u mu_v
//   A1 = 2 mu_u mu_v + c1, A2 = 2 s_uv + c2, B1 = mu_u^2 + mu_v^2 + c1, B2 = s_uu + s_vv + c2
//   S  = (A1 / B1)(A2 / B2):  Du = -S / B2,  Dc = 2 (A1 / B1) / B2,
//                             Dm = (2 mu_v A2 / B2 - 2 mu_u S) / B1 - 2 (mu_u - cu) Du - (mu_v - cv) Dc
//   cs = A2 / B2:             Du = -cs / B2, Dc = 2 / B2, Dm = -(2 (mu_u - cu) Du + (mu_v - cv) Dc)
//                             (the terms through the means' own ratio are absent)
//   d map / d a (q) = 1/2 [ (w * Dm)(q) + 2 (u(q) - cu) (w * Du)(q) + (v(q) - cv) (w * Dc)(q) ]     for EVERY pixel q of the plane
// (* = the transposed, full correlation with w; the D maps are zero outside the interior.)
//
// Shape: a workgroup of 256 threads owns a 32 x 32 tile.  It stages the tile and its 10-pixel halo of u and v (52 x 52 each)
// in LDS, runs the five forward maps as a row pass (52 x 42, three columns per thread) and a column pass (42 x 42, three
// rows per thread), forms the map and the three derivative maps of the 42 x 42 pixels within 5 of its tile -- over the
// staged inputs, which only the tile's own pixels are read from again, and those are in registers by then -- and runs them
// through a row pass (42 x 32) and a column pass (32 x 32, four rows per thread).  Every output pixel has exactly one owner:
// no atomics, the same bits run to run.  The map is summed over the interior pixels INSIDE the tile (each belongs to one
// tile) in f64, one f32 partial per workgroup.
//
// Cancellation: sum w u^2 - mu^2 of the raw values loses ~1e-7 against c2 = 9e-4 on flat windows (pointwise.hip's
// ssim_kernel centres per output pixel, which is not separable).  A variance does not move with the origin: the workgroup
// subtracts ONE constant per tile and input (the mean of the staged pixels) before the moments, so a flat tile has
// exactly zero variance, and the gradient is evaluated in the shifted variables too:
//   Dm' = 2 mu_v A2 / (B1 B2) - 2 mu_u A1 A2 / (B1^2 B2) - 2 (mu_u - cu) Du - (mu_v - cv) Dc,   u(q) - cu, v(q) - cv for u(q), v(q)
// -- the same sum, with products of small numbers where the raw form cancels products of large ones.  S is formed as
// (A1 / B1)(A2 / B2) and the pointwise step runs without fma contraction, so that identical images give cs = S = 1 exactly
// (at every level of a pyramid) and a gradient of zero or rounding residue (see the comment in ssim_fwd_cols; DESIGN.md
// section 4.4f has what was measured).
//
// LDS of a kernel that holds both regions: 2 x 52 x 53 + 5 x 52 x 43 floats = 66.8 KB -> two workgroups per CU.

constexpr int NT = 256;                 // threads per workgroup
constexpr int TS = 32;                  // tile of output pixels (TS x TS)
constexpr int KW = 11, HW5 = 5;         // window, half window
constexpr int RI = TS + 4 * HW5;        // 52: staged inputs (tile + 10 each side)
constexpr int RS = TS + 2 * HW5;        // 42: SSIM / derivative maps (tile + 5 each side)
constexpr int RIP = RI + 1, RSP = RS + 1, TSP = TS + 1;      // padded LDS rows
static_assert(RS % 3 == 0 && TS % 4 == 0 && (TS / 4) * TS == NT, "thread maps below");
static_assert(3 * RS * RSP <= 2 * RI * RIP && 3 * RS * TSP <= 5 * RI * RSP, "aliased LDS regions");

// The two LDS regions of a tile kernel, in floats:
//   SSIM_LDS_IN    u - cu, v - cv [2][RI][RIP]; later the three derivative maps [3][RS][RSP]
//   SSIM_LDS_TMP   row-pass results [5][RI][RSP]; later the backward's [3][RS][TSP]
constexpr int SSIM_LDS_IN = 2 * RI * RIP, SSIM_LDS_TMP = 5 * RI * RSP;

struct Gauss11 { float g[KW]; };

inline Gauss11 ssim_window() {
    Gauss11 gw;
    double g[KW], gs = 0.0;
    for (int k = 0; k < KW; ++k) gs += (g[k] = std::exp(-((k - HW5) * (k - HW5)) / (2.0 * 1.5 * 1.5)));
    for (int k = 0; k < KW; ++k) gw.g[k] = (float)(g[k] / gs);
    return gw;
}

struct SsimShift { float cu, cv; };

// ---- stage the tile at (ty0, tx0) of the H x W plane pa / pb and its halo; pixels outside the plane read 0 and are never
// used by an interior window.  su, sv: [RI][RIP] each; on return they hold u - cu, v - cv and the workgroup is in step.
__device__ __forceinline__ SsimShift ssim_stage_shift(const float* pa, const float* pb, int H, int W,
                                                      int ty0, int tx0, float* su, float* sv, float (*redf)[2]) {
    const int tid = threadIdx.x;
    float tu = 0.f, tv = 0.f;
    for (int e = tid; e < RI * RI; e += NT) {
        const int i = e / RI, j = e % RI;
        const int y = ty0 - 2 * HW5 + i, x = tx0 - 2 * HW5 + j;
        float u = 0.f, v = 0.f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            u = (pa[(int64_t)y * W + x] + 1.f) * 0.5f;
            v = (pb[(int64_t)y * W + x] + 1.f) * 0.5f;
            tu += u;
            tv += v;
        }
        su[i * RIP + j] = u;
        sv[i * RIP + j] = v;
    }
    tu = wave_sum(tu);
    tv = wave_sum(tv);
    if ((tid & 63) == 0) { redf[tid >> 6][0] = tu; redf[tid >> 6][1] = tv; }
    __syncthreads();
    const int ny = min(ty0 + TS + 2 * HW5, H) - max(ty0 - 2 * HW5, 0), nx = min(tx0 + TS + 2 * HW5, W) - max(tx0 - 2 * HW5, 0);
    const float inv_cnt = 1.f / (float)(ny * nx);
    const float cu = (redf[0][0] + redf[1][0] + redf[2][0] + redf[3][0]) * inv_cnt;
    const float cv = (redf[0][1] + redf[1][1] + redf[2][1] + redf[3][1]) * inv_cnt;
    for (int e = tid; e < RI * RI; e += NT) {          // the elements this thread wrote itself
        const int i = e / RI, j = e % RI;
        su[i * RIP + j] -= cu;
        sv[i * RIP + j] -= cv;
    }
    __syncthreads();
    return {cu, cv};
}

// the thread's own four pixels (column qc, rows qr0 .. qr0 + 3 of the tile): u - cu, v - cv, kept for the last step
__device__ __forceinline__ void ssim_own_pixels(const float* su, const float* sv, int qc, int qr0, float (&uq)[4], float (&vq)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uq[j] = su[(qr0 + j + 2 * HW5) * RIP + qc + 2 * HW5];
        vq[j] = sv[(qr0 + j + 2 * HW5) * RIP + qc + 2 * HW5];
    }
}

// ---- forward row pass: su, sv -> tmp [5][RI rows][RS columns], three adjacent columns per thread.  own_only: only the
// items that feed the tile's own pixels (rows [5, 47) and columns [5, 37) of the row pass) -- for a launch that only sums
// the map.  The caller synchronises; su and sv are dead after that.
__device__ __forceinline__ void ssim_fwd_rows(const float* su, const float* sv, float* tmp, const Gauss11& gw, bool own_only) {
    for (int it = threadIdx.x; it < RI * (RS / 3); it += NT) {
        const int r = it / (RS / 3), c0 = (it % (RS / 3)) * 3;
        if (own_only && (r < HW5 || r >= RI - HW5 || c0 + 2 < HW5 || c0 >= HW5 + TS)) continue;
        float xu[KW + 2], xv[KW + 2];
#pragma unroll
        for (int k = 0; k < KW + 2; ++k) {
            xu[k] = su[r * RIP + c0 + k];
            xv[k] = sv[r * RIP + c0 + k];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
            for (int k = 0; k < KW; ++k) {
                const float wu = gw.g[k] * xu[j + k], wv = gw.g[k] * xv[j + k];
                m0 += wu;
                m1 += wv;
                m2 += wu * xu[j + k];
                m3 += wv * xv[j + k];
                m4 += wu * xv[j + k];
            }
            const int o = r * RSP + c0 + j;
            tmp[o] = m0;
            tmp[RI * RSP + o] = m1;
            tmp[2 * RI * RSP + o] = m2;
            tmp[3 * RI * RSP + o] = m3;
            tmp[4 * RI * RSP + o] = m4;
        }
    }
}

// ---- forward column pass, the map and its derivative maps: [RS][RS], three adjacent rows per thread.  cs_only: the
// contrast-structure map A2 / B2 in place of S.  write_d: the maps Dm, Du, Dc go to sD [3][RS][RSP] (zero outside the
// plane's interior).  own_only as above.  Returns the thread's sum of the map over the tile's own interior pixels.
__device__ __forceinline__ double ssim_fwd_cols(const float* tmp, float* sD, const Gauss11& gw, int H, int W, int ty0, int tx0,
                                                SsimShift sh, bool cs_only, bool write_d, bool own_only) {
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    const float cu = sh.cu, cv = sh.cv;
    double acc = 0.0;
    for (int it = threadIdx.x; it < (RS / 3) * RS; it += NT) {
        const int c = it % RS, r0 = (it / RS) * 3;
        if (own_only && (c < HW5 || c >= HW5 + TS || r0 + 2 < HW5 || r0 >= HW5 + TS)) continue;
        float m[5][3];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            float x[KW + 2];
#pragma unroll
            for (int k = 0; k < KW + 2; ++k) x[k] = tmp[(q * RI + r0 + k) * RSP + c];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < KW; ++k) s += gw.g[k] * x[j + k];
                m[q][j] = s;
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i = r0 + j;
            const int y = ty0 - HW5 + i, x = tx0 - HW5 + c;
            float dm = 0.f, du = 0.f, dc = 0.f;
            if (y >= HW5 && y < H - HW5 && x >= HW5 && x < W - HW5) {
                // Contraction OFF and the ratios A1 / B1, A2 / B2 formed first: for a == b (a perfect reconstruction) A1 and
                // B1, A2 and B2 are then the same roundings of the same numbers, S is exactly 1, dc = -2 du and dm = 0 --
                // the gradient of identical images stays at zero or rounding residue, and that of nearly identical
                // ones cancels what it should.  (An fma in one of two matching expressions leaves half an ulp of each
                // behind.)  The same holds at every level of a pyramid, in the cs form as in the full one.
#pragma clang fp contract(off)
                const float mus = m[0][j], mvs = m[1][j];              // shifted means
                const float suu = m[2][j] - mus * mus, svv = m[3][j] - mvs * mvs, suv = m[4][j] - mus * mvs;
                const float A2 = 2.f * suv + c2, B2 = (suu + svv) + c2;
                const float r2 = A2 / B2;
                float val;
                if (cs_only) {
                    val = r2;
                    du = -r2 / B2;
                    dc = 2.f / B2;
                    dm = -(2.f * mus * du + mvs * dc);
                } else {
                    const float mu = mus + cu, mv = mvs + cv;
                    const float A1 = 2.f * (mu * mv) + c1, B1 = (mu * mu + mv * mv) + c1;
                    const float r1 = A1 / B1;
                    val = r1 * r2;
                    du = -val / B2;
                    dc = 2.f * r1 / B2;
                    dm = (2.f * mv * r2 - 2.f * mu * val) / B1 - (2.f * mus * du + mvs * dc);
                }
                if (i >= HW5 && i < HW5 + TS && c >= HW5 && c < HW5 + TS) acc += (double)val;    // the tile's own pixel
            }
            if (write_d) {
                sD[i * RSP + c] = dm;
                sD[RS * RSP + i * RSP + c] = du;
                sD[2 * RS * RSP + i * RSP + c] = dc;
            }
        }
    }
    return acc;
}

// the workgroup's sum of acc in a fixed order, as the f32 partial (every thread gets it; the workgroup is in step after)
__device__ __forceinline__ float ssim_tile_sum(double acc, double* redd) {
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) redd[threadIdx.x >> 6] = acc;
    __syncthreads();
    return (float)(redd[0] + redd[1] + redd[2] + redd[3]);
}

// ---- backward row pass: sD -> tmp [3][RS rows][TS tile columns], four adjacent columns per thread.  The caller synchronises.
// The item loop has at most two trips (336 items, 256 threads) and is unrolled by request: in the kernels that held this
// pass themselves the compiler did so unasked; left as a loop here, the calls at 256 x 256 were 0.6 - 0.9 % slower
// (DESIGN.md section 4.4f).
__device__ __forceinline__ void ssim_bwd_rows(const float* sD, float* tmp, const Gauss11& gw) {
#pragma unroll
    for (int it = threadIdx.x; it < RS * (TS / 4); it += NT) {
        const int r = it / (TS / 4), c0 = (it % (TS / 4)) * 4;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float x[KW + 3];
#pragma unroll
            for (int k = 0; k < KW + 3; ++k) x[k] = sD[q * RS * RSP + r * RSP + c0 + k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < KW; ++k) s += gw.g[k] * x[j + k];
                tmp[(q * RS + r) * TSP + c0 + j] = s;
            }
        }
    }
}

// ---- backward column pass: w * Dm, w * Du, w * Dc at the thread's own four pixels
__device__ __forceinline__ void ssim_bwd_cols(const float* tmp, const Gauss11& gw, int qc, int qr0, float (&wsum)[3][4]) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        float x[KW + 3];
#pragma unroll
        for (int k = 0; k < KW + 3; ++k) x[k] = tmp[(q * RS + qr0 + k) * TSP + qc];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < KW; ++k) s += gw.g[k] * x[j + k];
            wsum[q][j] = s;
        }
    }
}

// coef times the gradient sum of own pixel j (w * Dc = -2 w * Du exactly where a == b: no contraction here either)
__device__ __forceinline__ float ssim_grad_pixel(float coef, const float (&wsum)[3][4], const float (&uq)[4], const float (&vq)[4],
                                                 int j) {
#pragma clang fp contract(off)
    return coef * (wsum[0][j] + (2.f * uq[j] * wsum[1][j] + vq[j] * wsum[2][j]));
}
