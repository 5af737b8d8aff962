// Tiled denoising of images larger than the network (include/vaegan_hip.h "Tiled denoising"; host plan: tiling.py).
//   vg_tile_gather   tiles [t0, t0 + B) of the global tile list N * ny * nx, cut from the resident u8 set or from an f32 NCHW
//                    batch, written as the Encoder's NHWC input (pad channels zero)
//   vg_tile_blend    the f32 NCHW image from the f32 NCHW reconstruction tiles, in gather form: each output element sums its
//                    covering tiles in the contract's order with coefficients the host normalised -- no atomics, no
//                    zero-fill, no division, the same bits on every launch
// Both are pure data movement, HBM-bound.  The origin and coefficient tables are device memory the host cannot see at launch:
// every index read from them is range-checked in integer arithmetic before an address is formed from it, so no content of a
// table can cause an out-of-range access (the promise vg_region_mse_forward_backward makes for rects).
#include "common.hpp"

namespace {

struct TileGeom {
    int C, H, W, S, ny, nx;
};

// Workgroups of 64 x 4 threads: a wave runs along 64 consecutive x, the four waves take four consecutive rows.  Everything that
// needs a division (which tile, which image, which channel plane) is the same for the whole workgroup and comes from
// blockIdx, so it is computed once on the scalar unit; a thread only adds its own (x, y).
constexpr int TILE_BX = 64, TILE_BY = 4;

// grid (B, ceil(S / 4), ceil(S / 64)): workgroup (b, .., ..) works on tile t0 + b; thread (lx, ly) on one pixel of it.  The u8
// source is read as consecutive C-byte pixels and the f32 source as C coalesced rows; the pixel leaves as whole 16-byte units,
// 1 KiB per wave where S >= 64.
// U8: src u8 [N][H][W][C], exactly vg_gather_normalize_u8's arithmetic; else src f32 [N][C][H][W], copied.
template <int DT, bool U8>
__global__ __launch_bounds__(256) void tile_gather_kernel(const void* __restrict__ src, const int32_t* __restrict__ oy,
                                                          const int32_t* __restrict__ ox, TileGeom g, int64_t t0, int CP,
                                                          void* __restrict__ out) {
    constexpr int V = ElemT<DT>::per16;                 // channels per 16-byte unit: 4 (f32) | 8 (bf16)
    const int lx = blockIdx.z * TILE_BX + threadIdx.x, ly = blockIdx.y * TILE_BY + threadIdx.y;
    if (lx >= g.S || ly >= g.S) return;
    const int per_img = g.ny * g.nx;
    const int64_t HW = (int64_t)g.H * g.W;
    const int64_t t = t0 + blockIdx.x;
    const int64_t n = t / per_img;
    const int k = (int)(t - n * per_img);
    const int ky = k / g.nx, kx = k - ky * g.nx;
    const int y0 = oy[ky], x0 = ox[kx];
    const bool inside = y0 >= 0 && y0 <= g.H - g.S && x0 >= 0 && x0 <= g.W - g.S;         // a table entry off the image: zeros
    const int64_t hw = (int64_t)(y0 + ly) * g.W + (x0 + lx);
    const int64_t i = ((int64_t)blockIdx.x * g.S + ly) * g.S + lx;                         // output pixel
    for (int c0 = 0; c0 < CP; c0 += V) {
        float v[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int c = c0 + j;
            v[j] = 0.f;
            if (c < g.C && inside) {
                if constexpr (U8) {
                    const float u = (float)reinterpret_cast<const uint8_t*>(src)[(n * HW + hw) * g.C + c];
                    v[j] = __fdiv_rn(__fsub_rn(__fdiv_rn(u, 255.0f), 0.5f), 0.5f);
                } else {
                    v[j] = reinterpret_cast<const float*>(src)[(n * g.C + c) * HW + hw];
                }
            }
        }
        if constexpr (DT == VG_F32) {
            store4<VG_F32>(out, i * CP + c0, float4{v[0], v[1], v[2], v[3]});
        } else {
            u32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                o[j] = (uint32_t)ElemT<VG_BF16>::from_f32(v[2 * j]) | ((uint32_t)ElemT<VG_BF16>::from_f32(v[2 * j + 1]) << 16);
            *reinterpret_cast<u32x4*>(reinterpret_cast<uint16_t*>(out) + i * CP + c0) = o;
        }
    }
}

typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));     // 16 bytes at any 4-byte boundary

struct BlendTables {
    const int32_t* __restrict__ oy; const int32_t* __restrict__ ox;
    const int32_t* __restrict__ first_y; const int32_t* __restrict__ count_y; const float* __restrict__ coef_y;
    const int32_t* __restrict__ first_x; const int32_t* __restrict__ count_x; const float* __restrict__ coef_x;
    int wy, wx;
};

constexpr int TILE_ROWS = 8;                            // consecutive output rows per wave of the blend

// grid (N C, ceil(H / 32), ceil(ceil(W / 4) / 64)): workgroup (n c, .., ..) works on one channel plane; thread q of wave dy on
// the group of 4 consecutive x starting at 4 q, in TILE_ROWS consecutive rows.  What depends on x alone is read ONCE per
// thread and kept in registers over the rows: the cover range, and -- where the group lies whole inside its tiles (the four x
// are in the image, covered by the same tiles, each of which holds all four; always so where the origins and S are multiples of
// 4) -- each tile's offset and the group's coefficients.  A row then costs its y entries (the same for the whole wave: y comes
// from blockIdx and the wave's number), one 16-byte read per covering tile, at 4-byte alignment since tile rows start at
// arbitrary x origins, all of a tile row's reads issued before the first is used, and the store.  A group that straddles a tile
// edge, and every group where the x table is wider than 4 (WXC == 0), reads one float at a time with every index checked.
// VEC: one aligned 16-byte store (W % 4 == 0, out 16-byte aligned), 1 KiB per wave; else up to 4 scalar stores.
// Order (the contract): per ky ascending, inner = ((0 + cx_0 r_0) + cx_1 r_1) + ... over kx ascending; acc = (acc + cy inner);
// every product and sum rounded on its own.
template <bool VEC, int WXC>
__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ tiles, const BlendTables tb, TileGeom g,
                                                         float* __restrict__ out) {
#pragma clang fp contract(off)                                      // the contract rounds every product and sum on its own
    const int x0 = (blockIdx.z * TILE_BX + threadIdx.x) * 4;
    // a wave is one row of the 64 x 4 workgroup: threadIdx.y is the same in all its lanes
    const int ybeg = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * TILE_BY + threadIdx.y) * TILE_ROWS);
    if (x0 >= g.W || ybeg >= g.H) return;
    const int yend = ybeg + TILE_ROWS < g.H ? ybeg + TILE_ROWS : g.H;
    const int SS = g.S * g.S, per_img = g.ny * g.nx;
    const int64_t nc = blockIdx.x;                                  // (n, c)
    const int64_t n = nc / g.C;
    const int c = (int)(nc - n * g.C);
    int fx[4], cx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int x = x0 + e < g.W ? x0 + e : g.W - 1;              // past the row's end: computed like the last pixel, not stored
        fx[e] = tb.first_x[x];
        const int q = tb.count_x[x];
        cx[e] = q < 0 ? 0 : (q > tb.wx ? tb.wx : q);
    }
    constexpr int NR = WXC > 0 ? WXC : 1;
    bool whole = WXC > 0 && x0 + 3 < g.W && cx[0] >= 1 && fx[1] == fx[0] && fx[2] == fx[0] && fx[3] == fx[0] &&
                 cx[1] == cx[0] && cx[2] == cx[0] && cx[3] == cx[0];
    int64_t off[NR];                                               // tile (ky, 0)'s row -> the group's four values in tile (ky, kx)
    float cf[NR][4];
#pragma unroll
    for (int jx = 0; jx < NR; ++jx) {
        off[jx] = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) cf[jx][e] = 0.f;
        if (whole && jx < cx[0]) {
            const int kx = fx[0] + jx;
            whole = kx >= 0 && kx < g.nx;
            if (whole) {
                const int lx = x0 - tb.ox[kx];
                whole = lx >= 0 && lx + 3 < g.S;
                off[jx] = (int64_t)kx * g.C * SS + lx;
#pragma unroll
                for (int e = 0; e < 4; ++e) cf[jx][e] = tb.coef_x[(int64_t)(x0 + e) * tb.wx + jx];
            }
        }
    }
#pragma unroll
    for (int jx = 1; jx < NR; ++jx)
        if (jx >= cx[0]) off[jx] = off[0];                           // unused slots re-read slot 0 (never out of range) and are not summed
    for (int y = ybeg; y < yend; ++y) {
        const int fy = tb.first_y[y];
        int cy = tb.count_y[y];
        cy = cy < 0 ? 0 : (cy > tb.wy ? tb.wy : cy);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int jy = 0; jy < cy; ++jy) {
            const int ky = fy + jy;
            if (ky < 0 || ky >= g.ny) continue;
            const int ly = y - tb.oy[ky];
            if (ly < 0 || ly >= g.S) continue;
            const float wy = tb.coef_y[(int64_t)y * tb.wy + jy];
            const float* trow = tiles + ((n * per_img + (int64_t)ky * g.nx) * g.C + c) * SS + (int64_t)ly * g.S;   // tile (ky, 0)
            if (whole) {
                f32x4_u r[NR];
#pragma unroll
                for (int jx = 0; jx < NR; ++jx) r[jx] = *reinterpret_cast<const f32x4_u*>(trow + off[jx]);
                float inner[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int jx = 0; jx < NR; ++jx)
#pragma unroll
                    for (int e = 0; e < 4; ++e) inner[e] = jx < cx[0] ? inner[e] + cf[jx][e] * r[jx][e] : inner[e];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = acc[e] + wy * inner[e];
                continue;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int x = x0 + e < g.W ? x0 + e : g.W - 1;
                float inner = 0.f;
                for (int jx = 0; jx < cx[e]; ++jx) {
                    const int kx = fx[e] + jx;
                    if (kx < 0 || kx >= g.nx) continue;
                    const int lx = x - tb.ox[kx];
                    if (lx < 0 || lx >= g.S) continue;
                    const float r = trow[(int64_t)kx * g.C * SS + lx];
                    inner = inner + tb.coef_x[(int64_t)x * tb.wx + jx] * r;
                }
                acc[e] = acc[e] + wy * inner;
            }
        }
        float* dst = out + (nc * g.H + y) * g.W + x0;
        if constexpr (VEC) {
            *reinterpret_cast<float4*>(dst) = float4{acc[0], acc[1], acc[2], acc[3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x0 + e < g.W) dst[e] = acc[e];
        }
    }
}

// grid.y and grid.z hold at most 65535 workgroups each (H <= 262140 and W <= 16776960 keep the blend far inside); S * S stays an int
inline bool tile_geom_ok(int N, int C, int H, int W, int S, int ny, int nx) {
    return N >= 1 && C >= 1 && S >= 1 && H >= S && W >= S && ny >= 1 && nx >= 1 && ny <= H - S + 1 && nx <= W - S + 1 &&
           (int64_t)N * ny * nx < ((int64_t)1 << 31) && (int64_t)N * C < ((int64_t)1 << 31) && S <= 32768 && H <= 262140 &&
           W <= 16776960;
}

}  // namespace

extern "C" int vg_tile_gather(const uint8_t* src_u8, const float* src_f32, int N, int C, int H, int W, int S, int ny, int nx,
                              const int32_t* oy, const int32_t* ox, int64_t t0, int B, void* out, int CP, int dtype,
                              void* stream) {
    VG_CHECK_ARG(dtype == VG_F32 || dtype == VG_BF16, VG_ENOSUP);
    VG_CHECK_ARG(((src_u8 != nullptr) != (src_f32 != nullptr)) && oy && ox && out, VG_EINVAL);
    VG_CHECK_ARG(tile_geom_ok(N, C, H, W, S, ny, nx) && B >= 1 && t0 >= 0 && t0 + B <= (int64_t)N * ny * nx, VG_EINVAL);
    VG_CHECK_ARG(CP >= C, VG_EINVAL);
    VG_CHECK_ARG(CP % (dtype == VG_F32 ? 4 : 8) == 0 && vg_aligned16(out), VG_EALIGN);
    VG_CHECK_ARG((reinterpret_cast<uintptr_t>(src_f32) & 3u) == 0 && (reinterpret_cast<uintptr_t>(oy) & 3u) == 0 &&
                 (reinterpret_cast<uintptr_t>(ox) & 3u) == 0, VG_EALIGN);
    const TileGeom g{C, H, W, S, ny, nx};
    hipStream_t s = vg_stream(stream);
    const dim3 grid(B, (S + TILE_BY - 1) / TILE_BY, (S + TILE_BX - 1) / TILE_BX), block(TILE_BX, TILE_BY);
    if (dtype == VG_F32 && src_u8) hipLaunchKernelGGL((tile_gather_kernel<VG_F32, true>), grid, block, 0, s, src_u8, oy, ox, g, t0, CP, out);
    else if (dtype == VG_F32) hipLaunchKernelGGL((tile_gather_kernel<VG_F32, false>), grid, block, 0, s, src_f32, oy, ox, g, t0, CP, out);
    else if (src_u8) hipLaunchKernelGGL((tile_gather_kernel<VG_BF16, true>), grid, block, 0, s, src_u8, oy, ox, g, t0, CP, out);
    else hipLaunchKernelGGL((tile_gather_kernel<VG_BF16, false>), grid, block, 0, s, src_f32, oy, ox, g, t0, CP, out);
    return VG_LAUNCH_RC();
}

extern "C" int vg_tile_blend(const float* tiles, float* out, int N, int C, int H, int W, int S, int ny, int nx,
                             const int32_t* oy, const int32_t* ox, const int32_t* first_y, const int32_t* count_y,
                             const float* coef_y, int wy, const int32_t* first_x, const int32_t* count_x, const float* coef_x,
                             int wx, void* stream) {
    VG_CHECK_ARG(tiles && out && tiles != out && oy && ox && first_y && count_y && coef_y && first_x && count_x && coef_x,
                 VG_EINVAL);
    VG_CHECK_ARG(tile_geom_ok(N, C, H, W, S, ny, nx), VG_EINVAL);
    VG_CHECK_ARG(wy >= 1 && wy <= VG_TILE_MAX_COVER && wx >= 1 && wx <= VG_TILE_MAX_COVER, VG_EINVAL);
    for (const void* p : {(const void*)tiles, (const void*)out, (const void*)oy, (const void*)ox, (const void*)first_y,
                          (const void*)count_y, (const void*)coef_y, (const void*)first_x, (const void*)count_x,
                          (const void*)coef_x})
        VG_CHECK_ARG((reinterpret_cast<uintptr_t>(p) & 3u) == 0, VG_EALIGN);
    const TileGeom g{C, H, W, S, ny, nx};
    const BlendTables tb{oy, ox, first_y, count_y, coef_y, first_x, count_x, coef_x, wy, wx};
    const int groups_per_row = (W + 3) / 4;
    hipStream_t s = vg_stream(stream);
    const int rows_per_wg = TILE_BY * TILE_ROWS;
    const dim3 grid(N * C, (H + rows_per_wg - 1) / rows_per_wg, (groups_per_row + TILE_BX - 1) / TILE_BX), block(TILE_BX, TILE_BY);
    const bool vec = W % 4 == 0 && vg_aligned16(out);
#define BLEND_LAUNCH(WXC)                                                                                              \
    do {                                                                                                               \
        if (vec) hipLaunchKernelGGL((tile_blend_kernel<true, WXC>), grid, block, 0, s, tiles, tb, g, out);            \
        else hipLaunchKernelGGL((tile_blend_kernel<false, WXC>), grid, block, 0, s, tiles, tb, g, out);               \
    } while (0)
    switch (wx) {                                       // x tables of up to 4 slots: offsets and coefficients held in registers
    case 1: BLEND_LAUNCH(1); break;
    case 2: BLEND_LAUNCH(2); break;
    case 3: BLEND_LAUNCH(3); break;
    case 4: BLEND_LAUNCH(4); break;
    default: BLEND_LAUNCH(0); break;
    }
#undef BLEND_LAUNCH
    return VG_LAUNCH_RC();
}
