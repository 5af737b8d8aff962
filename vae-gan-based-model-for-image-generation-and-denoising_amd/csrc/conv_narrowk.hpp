// Narrow-K direct convolution: the image-side layers whose INPUT has 3 (padded 8) channels, i.e. one pixel = one
// 16-byte unit = one 8-element MFMA k-group -- the Discriminator's first Conv2d(3 -> C, k4 s2 p1) (gan_code.py:61),
// the Encoder's first Conv2d(3 -> 32, k4 s2 p0) (main_vae.py:23) and the data gradient of the Generator's last
// ConvTranspose2d(C -> 3, k3 s1 p1) (gan_code.py:49), a 3x3 convolution of the 3-channel image gradient.
// Included by conv_gemm.hip (inside its anonymous namespace); same descriptor (vg_gg_desc), same packed weights.
//
// These layers are HBM-bound (<= 20 FLOP/B): K = taps x 8 is 72..128, the output is N = 32..64
// channels wide.  The generic gather-GEMM stages A through LDS with per-16-byte bounds tests and an LDS-staged C tile
// sized for 128-wide problems; here
//   * the whole weight operand lives in registers (N/16 x K/32 fragments, <= 64 VGPRs),
//   * an A fragment IS a gather of 16 pixels x 4 taps (lane = (pixel, tap)): loaded straight from L1/L2 into VGPRs,
//     16 independent loads in flight per lane, no LDS, no barrier in the main part,
//   * a workgroup owns 256 consecutive output pixels x all N channels: its C tile is one contiguous run of the NHWC
//     output (256 x N x 2 bytes), written with 16-byte stores after a transpose through LDS,
//   * bias, (Leaky)ReLU of a BatchNorm-less layer and the per-channel BatchNorm partial sums ride in the epilogue,
//     one slab row per workgroup exactly as gg_kernel emits them (bn_act.hip reads either).

constexpr int NK_GP = 4;               // 16-pixel MFMA row groups per wave, worked as two halves
constexpr int NK_BM = 64 * NK_GP;

inline bool narrowk_enabled() { return vg_sw().edge != 0; }      // VG_EDGE (common.hpp: switches are read once at load)

// host: does the descriptor have the narrow-K form?
inline bool narrowk_ok(const vg_gg_desc* d, int dtype) {
    if (dtype != VG_BF16 || !narrowk_enabled()) return false;
    if (d->IC != 8 || d->nphase != 1 || d->mask_x != nullptr) return false;
    if (d->N % 16 != 0 || d->N < 16 || d->N > 64 || d->OC != d->N) return false;
    if (d->Kp % 32 != 0 || d->Kp > 128 || d->Kp < d->TH * d->TW * 8 || d->TW > 4) return false;
    if ((int64_t)d->B * d->GH * d->GW >= (1 << 24)) return false;                             // float-reciprocal divisions
    if ((int64_t)d->B * d->IH * d->IW >= (1 << 28)) return false;                             // 32-bit byte offsets into the input
    if (!gg_flat(*d)) return false;
    return true;
}

__device__ __forceinline__ int nk_fdiv(int a, int b, float inv) {      // a / b for 0 <= a < 2^24, inv = 1.0f / b
    int q = (int)((float)a * inv);
    const int r = a - q * b;
    if (r < 0) --q;
    else if (r >= b) ++q;
    return q;
}

template <int V> struct NkC { static constexpr int value = V; };

// ---- one tile per workgroup: launches that offer no more tiles than workgroups are resident at once ----
template <int NT, int KC>                       // N = 16 * NT output channels, Kp = 32 * KC
__global__ __launch_bounds__(256) void ggn_kernel(const vg_gg_desc d) {
    // per-wave C staging [64 pixels][N] bf16 (+16 B pad per pixel row) | stats scratch [4 waves][N][2]
    constexpr int N = NT * 16, CP = N * 2 + 16;
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * 16 * NK_GP * CP + 4 * N * 2 * 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int M = d.B * d.GH * d.GW, GHW = d.GH * d.GW;
    const int m0 = blockIdx.x * NK_BM + wave * 16 * NK_GP;
    const int ntap = d.TH * d.TW;
    // no integer divisions in the address generation (they, not the loads, were the critical path of the first cut):
    // m -> (b, gy, gx) through float reciprocals (m < 2^24), tap -> (ta, tb) through an 8-bit fixed-point reciprocal
    const float inv_ghw = 1.0f / (float)GHW, inv_gw = 1.0f / (float)d.GW;
    const int tw_inv = (256 + d.TW - 1) / d.TW;               // exact for taps < 16, TW <= 4

    constexpr int SEGS = NT * 16 * 2 / 16;                                    // 16-byte segments per pixel

    // ---- weights: all of them, in registers ----
    bf16x8 bw[NT][KC];
    float bv[NT];                                             // the bias rides with the weights: loaded in the epilogue it was a
    const unsigned char* Wb = reinterpret_cast<const unsigned char*>(d.W);      // second exposed round trip after the MFMAs
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int kc = 0; kc < KC; ++kc)
            bw[nt][kc] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(
                Wb + ((int64_t)(nt * 16 + fr) * d.Kp + kc * 32 + fg * 8) * 2));
        bv[nt] = d.bias != nullptr ? d.bias[nt * 16 + fr] : 0.f;
    }

    // ---- A fragments: lane (fr, fg) = (pixel m0 + 16g + fr, tap 4kc + fg) -> one 16-byte input pixel ----
    const unsigned char* Xb = reinterpret_cast<const unsigned char*>(d.X);
    u32x4 a[NK_GP][KC];
#pragma unroll
    for (int g = 0; g < NK_GP; ++g) {
        const int m = m0 + g * 16 + fr;
        int b = 0, gy = -(1 << 20), gx = 0;
        if (m < M) {
            b = nk_fdiv(m, GHW, inv_ghw);
            const int r = m - b * GHW;
            gy = nk_fdiv(r, d.GW, inv_gw);
            gx = r - gy * d.GW;
        }
        const int iy0 = gy * d.SY + d.y0[0], ix0 = gx * d.SX + d.x0[0];
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
            const int t = kc * 4 + fg;
            const int ta = (t * tw_inv) >> 8, tb = t - ta * d.TW;
            const int iy = iy0 + d.DY * ta, ix = ix0 + d.DX * tb;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (t < ntap && (unsigned)iy < (unsigned)d.IH && (unsigned)ix < (unsigned)d.IW)
                v = *reinterpret_cast<const u32x4*>(Xb + ((int64_t)(b * d.IH + iy) * d.IW + ix) * 16);
            a[g][kc] = v;
        }
    }
    f32x4 acc[NK_GP][NT];
#pragma unroll
    for (int g = 0; g < NK_GP; ++g)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KC; ++kc)
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[g][kc]), bw[nt][kc], c, 0, 0, 0);
            acc[g][nt] = c;
        }

    // ---- epilogue: lane holds rows (pixels) 16g + 4fg + r, column n = 16nt + fr ----
    auto epilogue = [&](auto act_c) {                           // the activation is uniform: chosen once, outside the element loops
        constexpr int ACT = decltype(act_c)::value;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int g = 0; g < NK_GP; ++g)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[g][nt][r] = act_fwd(acc[g][nt][r] + bv[nt], ACT, d.act_slope);
    };
    if (d.act == VG_ACT_RELU) epilogue(NkC<VG_ACT_RELU>{});
    else if (d.act == VG_ACT_LRELU) epilogue(NkC<VG_ACT_LRELU>{});
    else epilogue(NkC<VG_ACT_NONE>{});
    if (d.stats != nullptr) {
        float* red = reinterpret_cast<float*>(smem + 4 * 16 * NK_GP * CP);  // [wave][N][2]
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int g = 0; g < NK_GP; ++g)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (m0 + g * 16 + fg * 4 + r < M) {
                        const float v = acc[g][nt][r];
                        s1 += v;
                        s2 += v * v;
                    }
            gg_quad_sum(s1);
            gg_quad_sum(s2);
            if (fg == 0) {
                red[(wave * N + nt * 16 + fr) * 2 + 0] = s1;
                red[(wave * N + nt * 16 + fr) * 2 + 1] = s2;
            }
        }
        __syncthreads();
        if (tid < N) {
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { s1 += red[(w * N + tid) * 2]; s2 += red[(w * N + tid) * 2 + 1]; }
            d.stats[((int64_t)blockIdx.x * 2 + 0) * d.N + tid] = s1;
            d.stats[((int64_t)blockIdx.x * 2 + 1) * d.N + tid] = s2;
        }
    }
    // C tile: each wave transposes its own 64 x N block through LDS and writes one contiguous run of the output
    unsigned char* cw = smem + wave * 16 * NK_GP * CP;
#pragma unroll
    for (int g = 0; g < NK_GP; ++g)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                *reinterpret_cast<uint16_t*>(cw + (g * 16 + fg * 4 + r) * CP + (nt * 16 + fr) * 2) =
                    ElemT<VG_BF16>::from_f32(acc[g][nt][r]);
    __syncthreads();
    unsigned char* Yb = reinterpret_cast<unsigned char*>(d.Y);
#pragma unroll
    for (int it = 0; it < 16 * NK_GP * SEGS / 64; ++it) {
        const int u = lane + 64 * it;
        const int row = u / SEGS, seg = u - row * SEGS;
        const int m = m0 + row;
        if (m < M) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(cw + row * CP + seg * 16);
            *reinterpret_cast<u32x4*>(Yb + (int64_t)m * (N * 2) + seg * 16) = v;
        }
    }
}

// ---- the streaming form: launches with more tiles than resident workgroups ----
// How a workgroup spends its life (ggn_kernel is one serial chain per tile: weight and A loads, one wait, the MFMAs, epilogue,
// stores; two workgroups per CU start in lockstep, and a launch of several rounds of them costs rounds x one such life):
//   * persistent: the grid is min(tiles, resident workgroups) (VG_NK_WGS caps it further); weights and bias are loaded ONCE per
//     workgroup, which then walks tiles blockIdx.x, + gridDim.x, ...  A tile stays 256 output pixels and one statistics slab row.
//   * a wave works its 64 pixels as two halves of 32 in sequence: the A operand of the NEXT half (of this tile, or of the
//     workgroup's next tile) is loaded before the current half's MFMAs, epilogue and stores, so loads are always in flight.
//     Two A buffers of a half, one accumulator block of a half and the weights fit the registers of two waves per SIMD.
//   * no workgroup barrier but the one of the statistics (their LDS scratch alternates between two copies by tile, so one
//     barrier per tile is enough); the C transpose is per wave.
// Arithmetic and its order are the first cut's: per output the MFMA chain over kc; bias, activation; the statistics add a
// lane's values in the order g, r (both halves into the same accumulator), then lanes by shfl_xor 16 and 32, then waves 0..3.
template <int NT, int KC>                       // N = 16 * NT output channels, Kp = 32 * KC
__global__ __launch_bounds__(256, 2) void ggn_stream_kernel(const vg_gg_desc d, const int tiles) {
    // per-wave C staging [32 pixels][N] bf16 (+16 B pad per pixel row) | stats scratch [2 copies][4 waves][N][2]
    constexpr int N = NT * 16, CP = N * 2 + 16;
    constexpr int HG = NK_GP / 2, HROWS = 16 * HG;            // 16-pixel MFMA row groups / pixels per half
    static_assert(NK_GP % 2 == 0, "two halves per wave");
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * HROWS * CP + 2 * 4 * N * 2 * 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int M = d.B * d.GH * d.GW, GHW = d.GH * d.GW;
    const int ntap = d.TH * d.TW;
    // no integer divisions in the address generation (they, not the loads, were the critical path of the first cut):
    // m -> (b, gy, gx) through float reciprocals (m < 2^24), tap -> (ta, tb) through an 8-bit fixed-point reciprocal
    const float inv_ghw = 1.0f / (float)GHW, inv_gw = 1.0f / (float)d.GW;
    const int tw_inv = (256 + d.TW - 1) / d.TW;               // exact for taps < 16, TW <= 4

    constexpr int SEGS = NT * 16 * 2 / 16;                                    // 16-byte segments per pixel

    // ---- weights and bias: all of them, in registers, once per workgroup ----
    bf16x8 bw[NT][KC];
    float bv[NT];
    const unsigned char* Wb = reinterpret_cast<const unsigned char*>(d.W);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
        for (int kc = 0; kc < KC; ++kc)
            bw[nt][kc] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(
                Wb + ((int64_t)(nt * 16 + fr) * d.Kp + kc * 32 + fg * 8) * 2));
        bv[nt] = d.bias != nullptr ? d.bias[nt * 16 + fr] : 0.f;
    }

    // ---- A fragments of one half: lane (fr, fg) = (pixel mh + 16g + fr, tap 4kc + fg) -> one 16-byte input pixel.
    //      mh >= M (a tile beyond the last): nothing is read ----
    const unsigned char* Xb = reinterpret_cast<const unsigned char*>(d.X);
    auto load_half = [&](u32x4 (&a)[HG][KC], unsigned& keep, int mh) {
        keep = 0u;
        int fgv = fg, frv = fr;                                 // opaque per call: what is derived from them is recomputed here,
        asm volatile("" : "+v"(fgv), "+v"(frv));                // not kept in registers across the whole tile loop
#pragma unroll
        for (int g = 0; g < HG; ++g) {
            const int m = mh + g * 16 + frv;
            int b = 0, gy = -(1 << 20), gx = 0;
            if (m < M) {
                b = nk_fdiv(m, GHW, inv_ghw);
                const int r = m - b * GHW;
                gy = nk_fdiv(r, d.GW, inv_gw);
                gx = r - gy * d.GW;
            }
            const int iy0 = gy * d.SY + d.y0[0], ix0 = gx * d.SX + d.x0[0];
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                const int t = kc * 4 + fgv;
                const int ta = (t * tw_inv) >> 8, tb = t - ta * d.TW;
                const int iy = iy0 + d.DY * ta, ix = ix0 + d.DX * tb;
                // no branch around the load (a padding tap or a pixel beyond M reads input pixel 0 and is zeroed afterwards):
                // with a fixed number of loads in flight the wait in front of a half's MFMAs can leave the later ones out
                const bool in = t < ntap && (unsigned)iy < (unsigned)d.IH && (unsigned)ix < (unsigned)d.IW;
                const unsigned px = in ? (unsigned)((b * d.IH + iy) * d.IW + ix) : 0u;   // < 2^28 (narrowk_ok): 32-bit byte offset
                a[g][kc] = *reinterpret_cast<const u32x4*>(Xb + px * 16u);
                keep |= (unsigned)in << (g * KC + kc);          // (arithmetic, not a branch: the compiler would move the load into it)
            }
        }
    };

    float s1[NT], s2[NT];                                     // a lane's statistics of the current tile
    unsigned char* cw = smem + wave * HROWS * CP;             // this wave's C staging
    unsigned char* Yb = reinterpret_cast<unsigned char*>(d.Y);

    // ---- one half: MFMAs; then epilogue, statistics terms, transpose through LDS, stores.  Lane holds rows (pixels)
    //      16g + 4fg + r, column n = 16nt + fr ----
    f32x4 acc[HG][NT];
    auto mfma_half = [&](u32x4 (&a)[HG][KC], unsigned keep) {
        __builtin_amdgcn_sched_barrier(0);                      // the zeroing below is where the loads are waited for: not earlier
#pragma unroll
        for (int g = 0; g < HG; ++g) {
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {                   // (in place: the buffer is reloaded right after)
                const u32x4 z = {0u, 0u, 0u, 0u};
                a[g][kc] = (keep >> (g * KC + kc)) & 1u ? a[g][kc] : z;
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kc = 0; kc < KC; ++kc)
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a[g][kc]), bw[nt][kc], c, 0, 0, 0);
                acc[g][nt] = c;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto finish_half = [&](int mh) {
        auto epilogue = [&](auto act_c) {                       // the activation is uniform: chosen once, outside the element loops
            constexpr int ACT = decltype(act_c)::value;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int g = 0; g < HG; ++g)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[g][nt][r] = act_fwd(acc[g][nt][r] + bv[nt], ACT, d.act_slope);
        };
        if (d.act == VG_ACT_RELU) epilogue(NkC<VG_ACT_RELU>{});
        else if (d.act == VG_ACT_LRELU) epilogue(NkC<VG_ACT_LRELU>{});
        else epilogue(NkC<VG_ACT_NONE>{});
        if (d.stats != nullptr) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int g = 0; g < HG; ++g)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (mh + g * 16 + fg * 4 + r < M) {
                            const float v = acc[g][nt][r];
                            s1[nt] += v;
                            s2[nt] += v * v;
                        }
        }
        // C: the wave transposes its 32 x N block through its own LDS and writes one contiguous run of the output.  Only this
        // wave touches cw: its LDS operations complete in order, the fences keep the compiler from moving them across
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        int lv = lane;                                          // (opaque: see load_half)
        asm volatile("" : "+v"(lv));
        const int frw = lv & 15, fgw = lv >> 4;
#pragma unroll
        for (int g = 0; g < HG; ++g)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    *reinterpret_cast<uint16_t*>(cw + (g * 16 + fgw * 4 + r) * CP + (nt * 16 + frw) * 2) =
                        ElemT<VG_BF16>::from_f32(acc[g][nt][r]);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int it = 0; it < HROWS * SEGS / 64; ++it) {
            const int u = lv + 64 * it;
            const int row = u / SEGS, seg = u - row * SEGS;
            const int m = mh + row;
            if (m < M) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(cw + row * CP + seg * 16);
                *reinterpret_cast<u32x4*>(Yb + (int64_t)m * (N * 2) + seg * 16) = v;
            }
        }
    };

    // two halves ahead: a half's A registers are free once its MFMAs are issued, and are reloaded at once for the same half of
    // the workgroup's next tile, under this half's epilogue and stores and the whole other half
    u32x4 a0[HG][KC], a1[HG][KC];
    unsigned k0, k1;                                          // which of them are real (bit g * KC + kc)
    const int wm = wave * 16 * NK_GP;                         // the wave's first pixel within a tile
    load_half(a0, k0, blockIdx.x * NK_BM + wm);
    load_half(a1, k1, blockIdx.x * NK_BM + wm + HROWS);
    int par = 0;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x, par ^= 1) {
        const int m0 = tile * NK_BM + wm, m1 = (tile + (int)gridDim.x) * NK_BM + wm;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) { s1[nt] = 0.f; s2[nt] = 0.f; }
        mfma_half(a0, k0);
        load_half(a0, k0, m1);
        finish_half(m0);
        mfma_half(a1, k1);
        load_half(a1, k1, m1 + HROWS);
        finish_half(m0 + HROWS);
        if (d.stats != nullptr) {
            float* red = reinterpret_cast<float*>(smem + 4 * HROWS * CP) + par * (4 * N * 2);  // [wave][N][2]
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                float t1 = s1[nt], t2 = s2[nt];
                gg_quad_sum(t1);
                gg_quad_sum(t2);
                if (fg == 0) {
                    red[(wave * N + nt * 16 + fr) * 2 + 0] = t1;
                    red[(wave * N + nt * 16 + fr) * 2 + 1] = t2;
                }
            }
            __syncthreads();                                    // (uniform: every wave walks the same tiles)
            if (tid < N) {
                float t1 = 0.f, t2 = 0.f;
#pragma unroll
                for (int w = 0; w < 4; ++w) { t1 += red[(w * N + tid) * 2]; t2 += red[(w * N + tid) * 2 + 1]; }
                d.stats[((int64_t)tile * 2 + 0) * d.N + tid] = t1;
                d.stats[((int64_t)tile * 2 + 1) * d.N + tid] = t2;
            }
        }
    }
}

inline int nk_device_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0;
        hipDeviceProp_t p;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
        if (n <= 0) n = 1;
    }
    return n;
}

inline int launch_narrowk(const vg_gg_desc* d, hipStream_t s) {
    const int M = d->B * d->GH * d->GW;
    const int tiles = (M + NK_BM - 1) / NK_BM;
    const int resident = 2 * nk_device_cus();                  // two workgroups per CU at once (<= 256 VGPRs, 4 waves each)
    const int cap = vg_sw().nk_wgs;                            // VG_NK_WGS (tests: several tiles per workgroup at small sizes)
    // the streaming form is adopted where it was measured faster: 64 output channels (two waves per SIMD
    // either way) and more tiles than resident workgroups.  With one tile each it is the same chain in two halves, and the
    // narrower instantiations keep more one-tile workgroups resident than the streaming form's two per CU.  A cap forces it.
    const int NT = d->N / 16, KC = d->Kp / 32;
    const bool stream = cap > 0 || (NT == 4 && tiles > resident);
    int wgs = stream ? (cap > 0 && cap < resident ? cap : resident) : tiles;
    if (tiles < wgs) wgs = tiles;
    dim3 grid(wgs), block(256);
#define NK_LAUNCH(A, B) do { if (stream) vg_launch_timed(2, (ggn_stream_kernel<A, B>), grid, block, 0, s, *d, tiles); \
                             else vg_launch_timed(2, (ggn_kernel<A, B>), grid, block, 0, s, *d); } while (0)
    if (NT == 1) { if (KC == 1) NK_LAUNCH(1, 1); else if (KC == 2) NK_LAUNCH(1, 2); else if (KC == 3) NK_LAUNCH(1, 3); else NK_LAUNCH(1, 4); }
    else if (NT == 2) { if (KC == 1) NK_LAUNCH(2, 1); else if (KC == 2) NK_LAUNCH(2, 2); else if (KC == 3) NK_LAUNCH(2, 3); else NK_LAUNCH(2, 4); }
    else if (NT == 3) { if (KC == 1) NK_LAUNCH(3, 1); else if (KC == 2) NK_LAUNCH(3, 2); else if (KC == 3) NK_LAUNCH(3, 3); else NK_LAUNCH(3, 4); }
    else { if (KC == 1) NK_LAUNCH(4, 1); else if (KC == 2) NK_LAUNCH(4, 2); else if (KC == 3) NK_LAUNCH(4, 3); else NK_LAUNCH(4, 4); }
#undef NK_LAUNCH
    return VG_LAUNCH_RC();
}
