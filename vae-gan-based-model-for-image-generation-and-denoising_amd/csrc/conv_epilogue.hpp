// What the gather-GEMM kernels share after their main loops.  Included by conv_gemm.hip (inside its anonymous namespace),
// ahead of gg_kernel and of conv_patch.hpp / conv_phase4.hpp / conv_narrowk.hpp.
//
//   gg_flat          the one definition of "the output pixels are the GEMM rows, in order" (host and device)
//   gg_out_pixel     GEMM row -> output pixel through the phase's sub-pixel mapping
//   gg_tile_of_block XCD-aware (m tile, n tile) of a workgroup
//   gg_quad_sum      sum over the four 16-lane groups of a wave
//   mask_segment     activation backward on one 16-byte run of channels
//   gg_epilogue      the epilogue of gg_kernel (un-split) and ggp_kernel: bias, activation, BatchNorm partial sums,
//                    C tile through LDS, 16-byte channel runs to the NHWC output
// ggq_kernel and the ggn kernels keep their own staging (four phases side by side / per-wave contiguous runs) and take
// only the small helpers.

__host__ __device__ __forceinline__ bool gg_flat(const vg_gg_desc& d) {
    return d.nphase == 1 && d.OSY == 1 && d.OSX == 1 && d.GH == d.OH && d.GW == d.OW;
}

// output pixel index of GEMM row m of `phase` (-1: past M, or a sub-pixel position outside the output)
__device__ __forceinline__ int gg_out_pixel(const vg_gg_desc& __restrict__ d, bool flat, int phase, int m, int M, int GHW) {
    int op = -1;
    if (m < M) {
        if (flat) {
            op = m;
        } else {
            const int b = m / GHW;
            const int rem = m - b * GHW;
            const int gy = rem / d.GW;
            const int gx = rem - gy * d.GW;
            const int oy = gy * d.OSY + d.ooy[phase];
            const int ox = gx * d.OSX + d.oox[phase];
            if (oy < d.OH && ox < d.OW) op = (b * d.OH + oy) * d.OW + ox;
        }
    }
    return op;
}

// XCD-aware tile order (cdna_hip_programming.md T1): workgroups are dealt round-robin over the 8 XCDs, each with a
// private L2.  The launch is 1-D in (m tile, n tile); id -> (xcd = id % 8, slot = id / 8) and the slots of one XCD walk
// ALL n tiles of an m tile before moving on, so the gathered A rows of an m tile are fetched into one XCD's L2 once and
// re-used by its other n tiles (speed only; any placement is correct).
// n_major (weights larger than the input, conv_gemm.hip n_major()): an XCD owns n tiles (n % 8 == xcd) and walks all m
// tiles of one before the next, so it streams 1/8 of the WEIGHTS and all of the (smaller) input.
// n-major where flags & n_major_bit (gg_kernel: its launch argument and GG_N_MAJOR; ggp_kernel: PatchGeo::n_major and
// every bit).  The test stays in here: formed at the call it compiles to one scalar instruction more ahead of
// gg_kernel's main loop.
struct GgTile { int bx, by; };          // (m tile, n tile)

template <int BN>
__device__ __forceinline__ GgTile gg_tile_of_block(int N, int flags, int n_major_bit) {
    int bx, by;
    const int n_tiles = (N + BN - 1) / BN;
    const int id = blockIdx.x;
    const int xcd = id & 7, slot = id >> 3;
    if (flags & n_major_bit) {
        const int mt = (int)gridDim.x / n_tiles;
        bx = slot % mt;
        by = (slot / mt) * 8 + xcd;
    } else {
        by = slot % n_tiles;
        bx = (slot / n_tiles) * 8 + xcd;
    }
    return GgTile{bx, by};
}

// lane (fr, fg) holds a partial sum of column fr: the total over fg = 0..3, in every lane
__device__ __forceinline__ void gg_quad_sum(float& a) {
    a += __shfl_xor(a, 16);
    a += __shfl_xor(a, 32);
}

// activation backward fused into a data-gradient epilogue (vg_gg_desc::mask_x): v = dL/d(activated output) segment
// (16 bytes, storage dtype), x = the layer's activated output at the same place; returns v * act'(x), rounded again
template <int DT>
__device__ __forceinline__ u32x4 mask_segment(u32x4 v, const u32x4& x, int act, float slope) {
    if constexpr (DT == VG_BF16) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float xl = __uint_as_float(x[k] << 16), xh = __uint_as_float(x[k] & 0xffff0000u);
            const float gl = __uint_as_float(v[k] << 16), gh = __uint_as_float(v[k] & 0xffff0000u);
            const uint32_t lo = ElemT<VG_BF16>::from_f32(act_bwd(xl, gl, act, slope));
            const uint32_t hi = ElemT<VG_BF16>::from_f32(act_bwd(xh, gh, act, slope));
            v[k] = lo | (hi << 16);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = __float_as_uint(act_bwd(__uint_as_float(x[k]), __uint_as_float(v[k]), act, slope));
    }
    return v;
}

// The epilogue of a BM x BN tile held as 16x16 MFMA accumulators by WM x WN waves (NT threads; wave (wm, wn) owns rows
// wm * BM/WM .., columns wn * BN/WN ..; lane (fr, fg) holds rows fg*4 + r of column fr of each 16x16 tile).
//   (1) output-pixel table, filled once per workgroup (no per-element integer division for the sub-pixel scatter);
//   (2) + bias, fused activation of a layer without BatchNorm;
//   (3) BatchNorm partial statistics straight from the accumulators (valid rows / real channels only):
//       wave -> LDS [WM][BN][2] -> slab row (phase * m_tiles + bx) of d.stats (deterministic, no atomics);
//   (4) the C tile goes through LDS (pitch CPITCH, in NPASS blocks of BM / NPASS rows where it exceeds the buffers) so
//       that every lane writes one 16-byte run of channels of one output pixel (NHWC) instead of 2/4-byte scatters.
// smem: the kernel's stage buffers, free once every wave is past its main loop (the barrier after (2)); it holds the
// statistics scratch, then the C tile.  opix_tab: BM ints that (3) and (4) do not overwrite.  Both belong to the
// kernel's single __shared__ object.  UNROLL: the store loop of (4) as whole, fully unrolled iterations (ggp_kernel)
// or as a counted loop (gg_kernel).
// d: the kernel's own by-value parameter, as a __restrict__ reference (unqualified, its fields are loaded again after
// every LDS store; by value, the dynamic d.ooy[phase] puts the descriptor on the stack).  GgWhere: where the thread and
// its tile stand, as the kernel already holds them (DESIGN.md section 4.1 has the measurements behind both).
struct GgWhere {
    int tid, wm, wn, fr, fg;            // thread, its wave's place in the WM x WN grid, its lane's row / k group
    int phase, bx, m_tiles;             // the statistics slab row is phase * m_tiles + bx
    int M, GHW, m0, n0;                 // GEMM rows, grid pixels per image, first row / column of the tile
};

template <int DTO, int BM, int BN, int WM, int WN, int NT, int NPASS, int CPITCH, bool UNROLL, int TM, int TN>
__device__ __forceinline__ void gg_epilogue(const vg_gg_desc& __restrict__ d, f32x4 (&acc)[TM][TN], unsigned char* smem, int* opix_tab,
                                            const GgWhere at) {
    typedef ElemT<DTO> EO;
    constexpr int ESZO = EO::size;
    constexpr int RPW = BM / WM, CPW = BN / WN;        // rows / columns per wave
    static_assert(TM == RPW / 16 && TN == CPW / 16 && WM * WN * 64 == NT, "accumulator shape");
    const int tid = at.tid, wm = at.wm, wn = at.wn, fr = at.fr, fg = at.fg;
    const int phase = at.phase, bx = at.bx, m_tiles = at.m_tiles, M = at.M, GHW = at.GHW, m0 = at.m0, n0 = at.n0;

    const bool flat = gg_flat(d);
    for (int r = tid; r < BM; r += NT) opix_tab[r] = gg_out_pixel(d, flat, phase, m0 + r, M, GHW);
    float biasv[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nc = n0 + wn * CPW + j * 16 + fr;
        biasv[j] = (d.bias != nullptr && nc < d.N) ? d.bias[nc] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] += biasv[j];
    if (d.act != VG_ACT_NONE) {                        // activation of a layer without BatchNorm, fused
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = act_fwd(acc[i][j][r], d.act, d.act_slope);
    }
    __syncthreads();                                   // opix_tab visible; main-loop LDS reads are done

    if (d.stats != nullptr) {
        float* red = reinterpret_cast<float*>(smem);   // [WM][BN][2]
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = wm * RPW + i * 16 + fg * 4 + r;
                    if (opix_tab[row] >= 0) {
                        const float v = acc[i][j][r];
                        a += v;
                        b += v * v;
                    }
                }
            gg_quad_sum(a);
            gg_quad_sum(b);
            if (fg == 0) {
                const int c = wn * CPW + j * 16 + fr;
                red[(wm * BN + c) * 2 + 0] = a;
                red[(wm * BN + c) * 2 + 1] = b;
            }
        }
        __syncthreads();
        if (tid < BN && n0 + tid < d.N) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int w = 0; w < WM; ++w) { a += red[(w * BN + tid) * 2]; b += red[(w * BN + tid) * 2 + 1]; }
            const int64_t part = (int64_t)phase * m_tiles + bx;
            d.stats[(part * 2 + 0) * d.N + n0 + tid] = a;
            d.stats[(part * 2 + 1) * d.N + n0 + tid] = b;
        }
        __syncthreads();
    }

    constexpr int PROWS = BM / NPASS;
    constexpr int SEGS = BN * ESZO / 16;                // 16-byte segments per tile row
    static_assert(NPASS == 1 || NPASS == WM, "a pass is the rows of one wave row");
    static_assert(!UNROLL || (PROWS * SEGS) % NT == 0, "whole store iterations");
    unsigned char* Yb = reinterpret_cast<unsigned char*>(d.Y);
    const int oc_bytes = d.OC * ESZO;
#pragma unroll
    for (int pass = 0; pass < NPASS; ++pass) {
        const bool mine = (NPASS == 1) || (wm == pass);
        if (mine) {
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = wm * RPW + i * 16 + fg * 4 + r - pass * PROWS;
                        const int col = wn * CPW + j * 16 + fr;
                        typename EO::type* dst = reinterpret_cast<typename EO::type*>(smem + row * CPITCH) + col;
                        *dst = EO::from_f32(acc[i][j][r]);
                    }
        }
        __syncthreads();
        auto store_run = [&](int u) {
            const int row = u / SEGS, seg = u - row * SEGS;
            const int op = opix_tab[pass * PROWS + row];
            const int cb = n0 * ESZO + seg * 16;        // byte offset of this segment inside the output pixel
            if (op >= 0 && cb < oc_bytes) {
                u32x4 v = *reinterpret_cast<const u32x4*>(smem + row * CPITCH + seg * 16);
                if (d.mask_x != nullptr)
                    v = mask_segment<DTO>(v, *reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(d.mask_x) +
                                                                           (int64_t)op * oc_bytes + cb), d.mask_act, d.mask_slope);
                *reinterpret_cast<u32x4*>(Yb + (int64_t)op * oc_bytes + cb) = v;
            }
        };
        if constexpr (UNROLL) {
#pragma unroll
            for (int it = 0; it < (PROWS * SEGS) / NT; ++it) store_run(tid + it * NT);
        } else {
            for (int u = tid; u < PROWS * SEGS; u += NT) store_run(u);
        }
        if (pass + 1 < NPASS) __syncthreads();
    }
}
