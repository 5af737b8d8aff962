// Patch gather-GEMM: the 2x2-tap / stride-2 4x4-tap convolution forms with the input patch of a tile resident in LDS.
// Included by conv_gemm.hip (inside its anonymous namespace).  bf16, LDS-DMA, 128 x 128 (4 waves) or 256 x 128
// (8 waves) output tile.
//
// Why.  gg_kernel re-gathers the A operand once per filter tap: a 128-row tile moves 4 x 128 pixels x 64 B per
// 32-channel chunk for a 2x2-tap form although those rows are the SAME input pixels shifted by one.  The kernel
// sits on the per-CU L2->LDS fill rate, so bytes per FLOP are what bounds it.  Here a tile's
// input patch -- (R+1) x (GW+1) pixels for R whole grid rows -- is fetched ONCE per 32-channel chunk (<= 192 pixels
// instead of 512) and the four taps read it at four shifted positions; only the weight tiles still stream per tap.
// LDS fill per (chunk, 4 taps): <= 12 KB patch + 32 KB weights, against 32 + 32 KB.
//
// Forms (vg_gg_desc):
//   * one phase of the 4-phase transposed form: TH = TW = 2, SY = SX = 1, DY, DX = +-1 (blockIdx.z = phase);
//   * the direct stride-2 4x4 convolution: TH = TW = 4, SY = SX = 2, DY = DX = 1, split into its 4 input-parity
//     classes, each of which IS a 2x2-tap stride-1 form on the parity-subsampled input.
// Tile = 128 consecutive grid pixels = IMGS images x R whole grid rows (GW a power of two, 4 ... 64).
//
// Pipeline per workgroup: chunks j = (class, 32-channel chunk); patch(j) lives in pbuf[j & 1] and is fetched while
// chunk j-1 is multiplied (its DMA rounds spread over that chunk's stages); weight tiles alternate between two slots of
// TPS taps, one stage ahead.  One s_barrier per stage; everything issued during a stage is drained at the next.

struct PatchGeo {
    int R, IMGS, PW, PIMG, NPP;     // grid rows per image in a tile, images per tile, patch width, pixels per image, total
    int ncy, ncx, nct;              // parity classes per dimension, 32-channel chunks per (class, tap)
    int n_major;                    // XCD-major over n tiles (conv_gemm.hip n_major())
};

// Taps per barrier stage / weight-ring slots: 2 taps x 2 slots (56.5 KB, 2 workgroups per CU, half the barriers per FLOP
// of 1 tap x 3 slots -- the shape that won for gg_kernel and wgrad); the 8-wave tiles take all 4 taps per barrier.
constexpr int GP_BN = 128;

// Waves per SIMD the register allocation must leave room for: the narrow variants whose stage buffers are exactly 40 KB
// (128 rows) / 80 KB (256 rows) run FOUR / TWO workgroups per CU = 4 waves per SIMD (<= 128 registers).
constexpr int gp_min_waves(int WM, int BN, int NR_) {
    if (WM == 4) return BN <= 64 ? 4 : 2;
    return (2 * (NR_ ? NR_ : 4) * 4096 + 256 * BN <= 40960) ? 4 : 1;
}

// WM = 2: 128-row tile, 4 waves, patch <= 256 pixels (4 DMA rounds) or <= 192 (NR_ = 3); LDS = 2 patch buffers + 2 weight
//         slots of 2 taps: 64.5 KB at BN = 128 (2 workgroups per CU), 48 KB at BN = 64, exactly 40 KB for BN = 64 with 3
//         rounds and for BN = 32 (FOUR workgroups per CU, <= 128 registers: gp_min_waves).
// WM = 4, BN = 64: 256 x 64, 8 waves, 80 KB, TWO workgroups per CU (<= 128 registers), for launches with >= 512 such tiles.
// WM = 4: 256-row tile, 8 waves sharing every weight tile (half the weight traffic per FLOP), patch <= 384 pixels,
//         all four taps of a chunk per barrier, 113 KB LDS: ONE workgroup (8 waves, up to 256 registers each) per CU.
//         History: with a 128-register cap (two workgroups per CU) it spilled and lost 30 %; at one workgroup per CU
//         with two taps per barrier it was on par; with four taps per barrier it wins where the launch has >= 384
//         tiles (G3 fprop 742 -> 780, G4 dgrad 689 -> 750 TFLOP/s) and loses at 256 tiles (G2 fprop 835 -> 806).

template <int WM, int BN = GP_BN, int NR_ = 0>       // NR_: patch DMA rounds (0 = by tile shape); 3 where the patch has <= 192 pixels
__global__ __launch_bounds__(128 * WM, gp_min_waves(WM, BN, NR_)) void ggp_kernel(const vg_gg_desc d, const PatchGeo g) {
    // BN = 128: wave tile 64 x 64; BN = 64 (layers with <= 64 output channels): wave tile 64 x 32; BN = 32: 64 x 16
    constexpr int BM = 64 * WM, WN = 2, TM = 4, TN = BN / 32, NT = 128 * WM, BST = BN * 64, WNC = BN / 2;
    // patch DMA rounds: 192 (3) or 256 (4) pixels per 128 rows; WM == 4: 3 rounds of 512 lanes = 384 pixels
    constexpr int NR = NR_ ? NR_ : (WM == 4 ? 3 : 4);
    constexpr int GP_PBUF = NR * NT * 16;           // NR rounds of NT lanes x 16 B
    constexpr int TPS = WM == 4 ? 4 : 2;            // taps per barrier stage (8 waves: all 4 taps of a chunk)
    constexpr int NB = 2, BSTAGE = TPS * BST;       // the main loop alternates two weight slots
    constexpr int BJ = (BN * 4 + NT - 1) / NT;      // weight-tile DMA instructions per wave and tap (2 / 1)
    // 256 x 64: the 64-row weight tile needs only 256 of the 512 lanes -> waves 4-7 skip the weight DMA (legal here:
    // no counted vmcnt waits, every stage drains with vmcnt(0))
    constexpr bool B_HALF = (BN * 4 < NT);
    static_assert(BN == 128 || BN == 64 || BN == 32, "supported shapes");
    // [patch buffers 2 x 12|16|24 KB][2 weight slots of TPS taps][output-pixel table]
    // OVL (narrow tiles; 64 wide with 3 patch rounds and 32 wide: exactly 40 KB of stage buffers): the epilogue's output-pixel table lives in
    // the weight-ring slot the LAST stage does not read, so that FOUR workgroups fit a CU's 160 KB (the kernel is bound
    // by the LDS-DMA bytes in flight per CU: short-K tiles wait ~1 us for every stage they issue, section 9).
    constexpr bool OVL = BN <= 64;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * GP_PBUF + NB * BSTAGE + (OVL ? 0 : BM * 4)];
    unsigned char* const pbuf = smem;
    unsigned char* const bring = smem + 2 * GP_PBUF;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const int wm = wave / WN, wn = wave % WN;
    const int phase = blockIdx.z;
    const GgTile tile = gg_tile_of_block<BN>(d.N, g.n_major, ~0);
    const int bx = tile.bx, by = tile.by;
    const int M = d.B * d.GH * d.GW;
    const int GHW = d.GH * d.GW;
    const int m_tiles_ = M / BM;                               // eligibility: M % 128 == 0
    if (bx >= m_tiles_) return;
    const int m0 = bx * BM, n0 = by * BN;
    const int b0 = m0 / GHW;
    const int gy0 = (m0 - b0 * GHW) / d.GW;                    // 0 for multi-image tiles

    const unsigned char* Xb = reinterpret_cast<const unsigned char*>(d.X);
    const unsigned char* Wb = reinterpret_cast<const unsigned char*>(d.W);
    const unsigned char* Zp = reinterpret_cast<const unsigned char*>(d.zeros);
    const uint32_t pix_bytes = (uint32_t)d.IC * 2u;
    const uint32_t wrow_bytes = (uint32_t)d.Kp * 2u;
    const int ncls = g.ncy * g.ncx;
    const int J = ncls * g.nct;                                 // chunks
    // stage s of the main loop reads ring slot s & 1; J * (4 / TPS) stages -> the other slot is free from the last barrier on
    int* const opix_tab = reinterpret_cast<int*>(OVL ? bring + ((J * (4 / TPS)) & 1) * BSTAGE : smem + 2 * GP_PBUF + NB * BSTAGE);

    // ---- weight-tile DMA lanes: rows lrow, lrow + 64; source unit swizzled by the row (as gg_kernel) ----
    const int lrow = tid >> 2;
    const int qb = (tid & 3) ^ ((-(lrow >> 2)) & 3);
    const unsigned char* b_base[BJ];
    uint32_t b_live[BJ];
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
        const int n = n0 + lrow + (NT / 4) * j;
        const bool ok = n < d.N;
        b_base[j] = ok ? Wb + ((int64_t)phase * d.N + n) * wrow_bytes + qb * 16 : Zp;
        b_live[j] = ok ? 1u : 0u;
    }
    // ---- patch DMA lanes: LDS slot sidx = NT*r + tid -> pixel pp = sidx >> 2, stored unit sidx & 3.  The lane's
    // pixel coordinates are recomputed at every class change (<= 4 times per kernel) rather than kept in registers.
    // Unit swizzle of the patch image: unit u of pixel pp sits in slot u ^ ((pp >> 1) & 3).  The four taps read the
    // patch at offsets 0, 1, PW, PW + 1 (PW odd), so a fragment's 16 pixels start at ANY alignment; with this key a
    // ds_read_b128 of 16 consecutive pixels is conflict-free at every offset (4 LDS cycles; the row-tile key
    // (-(pp >> 2)) & 3 of gg_kernel cost 7.5-7.75 here: SQ_LDS_BANK_CONFLICT was 37-53 % of SQ_LDS_IDX_ACTIVE).
    const unsigned char* a_cur[NR];
    uint32_t a_live = 0;                                         // bit r: round r reads real data (else the zero page)
    auto patch_sources = [&](int cl) {
        const int py = cl / g.ncx, px = cl - py * g.ncx;
        // class (py, px): input pixel of patch position (pr, pc) is ((gy0 + pr)*SY + cy, pc*SX + cx)
        const int cy = d.y0[phase] + d.DY * py - (d.DY < 0 ? d.SY : 0);
        const int cx = d.x0[phase] + d.DX * px - (d.DX < 0 ? d.SX : 0);
        a_live = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int sidx = NT * r + tid;
            const int pp = sidx >> 2;
            const int q = (sidx & 3) ^ ((pp >> 1) & 3);
            const int img = pp / g.PIMG;
            const int rem = pp - img * g.PIMG;
            const int pr = rem / g.PW;
            const int pc = rem - pr * g.PW;
            const int b = b0 + img;
            const int iy = (gy0 + pr) * d.SY + cy;
            const int ix = pc * d.SX + cx;
            const bool ok = pp < g.NPP && b < d.B && (unsigned)iy < (unsigned)d.IH && (unsigned)ix < (unsigned)d.IW;
            a_cur[r] = ok ? Xb + ((uint32_t)((b * d.IH + iy) * d.IW + ix) * pix_bytes + (uint32_t)q * 16u) : Zp;
            a_live |= ok ? (1u << r) : 0u;
        }
    };
    // issue-side cursors
    int pj_cl = 0, pj_c = 0;                                    // (class, chunk) of the NEXT patch to fetch
    auto issue_patch_round = [&](int buf, int r) {              // r is a compile-time constant at every call site
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)a_cur[r],
                                         (__attribute__((address_space(3))) void*)(pbuf + buf * GP_PBUF + (NT * r + 64 * wave_u) * 16),
                                         16, 0, 0);
        a_cur[r] += (a_live >> r & 1u) * 64u;
    };
    auto patch_advance = [&]() {                                // after the 3 rounds of one patch
        if (++pj_c == g.nct) { pj_c = 0; ++pj_cl; if (pj_cl < ncls) patch_sources(pj_cl); }
    };
    int bs_cl = 0, bs_c = 0, bs_k = 0;                          // (class, chunk, tap-in-class) of the NEXT weight stage
    auto issue_b = [&](int buf) {                                // the TPS taps of one stage
#pragma unroll
        for (int tp = 0; tp < TPS; ++tp) {
            const int py = bs_cl / g.ncx, px = bs_cl - py * g.ncx;
            const int t = ((bs_k >> 1) * g.ncy + py) * d.TW + ((bs_k & 1) * g.ncx + px);
            const uint32_t koff = ((uint32_t)t * (uint32_t)d.IC + (uint32_t)bs_c * 32u) * 2u;
            if (!(B_HALF && wave_u >= (BN * 4) / 64)) {
#pragma unroll
                for (int j = 0; j < BJ; ++j) {
                    const unsigned char* src = b_base[j] + (b_live[j] ? koff : 0u);
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                     (__attribute__((address_space(3))) void*)(bring + buf * BSTAGE + tp * BST + ((NT / 4) * j + 16 * wave_u) * 64),
                                                     16, 0, 0);
                }
            }
            if (++bs_k == 4) { bs_k = 0; if (++bs_c == g.nct) { bs_c = 0; ++bs_cl; } }
        }
    };

    // ---- fragment addressing ----
    const int fr = lane & 15, fg = lane >> 4;
    int ppbase[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int r = wm * 64 + i * 16 + fr;
        const int per_img = g.R * d.GW;
        const int img = r / per_img;
        const int rr = r - img * per_img;
        const int ry = rr / d.GW;
        ppbase[i] = img * g.PIMG + ry * g.PW + (rr - ry * d.GW);
    }
    const int sh_y1 = d.DY > 0 ? 1 : 0, sh_x1 = d.DX > 0 ? 1 : 0;   // patch shift of local tap a = 1 (a = 0: the other)

    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    auto compute = [&](int pb, int bb, int k) {
        const int a = k >> 1, b = k & 1;
        const int shy = a ? sh_y1 : 1 - sh_y1, shx = b ? sh_x1 : 1 - sh_x1;
        const int tapoff = shy * g.PW + shx;
        const unsigned char* sa = pbuf + pb * GP_PBUF;
        const unsigned char* sb = bring + bb * BSTAGE + (k % TPS) * BST;
        u32x4 fa[TM], fb[TN];
        auto ld_a = [&](int i) {
            const int pp = ppbase[i] + tapoff;
            fa[i] = *reinterpret_cast<const u32x4*>(sa + pp * 64 + ((fg ^ ((pp >> 1) & 3)) << 4));
        };
        auto ld_b = [&](int j) {
            const int r = wn * WNC + j * 16 + fr;
            fb[j] = *reinterpret_cast<const u32x4*>(sb + r * 64 + ((fg ^ ((-(r >> 2)) & 3)) << 4));
        };
#define GP_MFMA(i, j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, fa[i]), \
                                                                  __builtin_bit_cast(bf16x8, fb[j]), acc[i][j], 0, 0, 0)
        if constexpr (TN == 4) {
            ld_a(0); ld_b(0); ld_b(1); ld_a(1); ld_b(2); ld_a(2); ld_b(3); ld_a(3);
            // MFMAs in the order their fragments arrive (fa0 fb0 | fb1 | fa1 | fb2 | fa2 | fb3 | fa3) ...
            GP_MFMA(0, 0);
            GP_MFMA(0, 1);
            GP_MFMA(1, 0); GP_MFMA(1, 1);
            GP_MFMA(0, 2); GP_MFMA(1, 2);
            GP_MFMA(2, 0); GP_MFMA(2, 1); GP_MFMA(2, 2);
            GP_MFMA(0, 3); GP_MFMA(1, 3); GP_MFMA(2, 3);
            GP_MFMA(3, 0); GP_MFMA(3, 1); GP_MFMA(3, 2); GP_MFMA(3, 3);
            // ... and a scheduling pipeline that interleaves the ds_read_b128s with them instead of "all reads, wait
            // for everything, all MFMAs" (0x100 = DS read, 0x008 = MFMA): two reads stay in flight ahead of the MFMA
            // that needs them
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0); __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x008, 10, 0);
        } else if constexpr (TN == 1) {
            ld_a(0); ld_b(0); ld_a(1); ld_a(2); ld_a(3);
            GP_MFMA(0, 0); GP_MFMA(1, 0); GP_MFMA(2, 0); GP_MFMA(3, 0);
        } else {
            ld_a(0); ld_b(0); ld_b(1); ld_a(1); ld_a(2); ld_a(3);
            GP_MFMA(0, 0); GP_MFMA(0, 1);
            GP_MFMA(1, 0); GP_MFMA(1, 1);
            GP_MFMA(2, 0); GP_MFMA(2, 1);
            GP_MFMA(3, 0); GP_MFMA(3, 1);
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0); __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        }
#undef GP_MFMA
    };

    // ---- prologue: patch(0) (3 rounds), then the first weight stage(s) ----
    patch_sources(0);
#pragma unroll
    for (int r = 0; r < NR; ++r) issue_patch_round(0, r);
    patch_advance();
    // ---- TPS taps per barrier, two weight slots: everything issued during a stage is drained at the next ----
    constexpr int SPC = 4 / TPS;                            // stages per chunk
    issue_b(0);
    const int S2 = J * SPC;
    int bb = 0, s = 0;
    for (int j = 0; j < J; ++j) {
        const int pb = j & 1;
        const bool more_p = j + 1 < J;
#pragma unroll
        for (int h = 0; h < SPC; ++h, ++s) {
            VG_WAITCNT_VM(0);
            __builtin_amdgcn_s_barrier();
            if (more_p) {
#pragma unroll
                for (int r = 0; r < NR; ++r)
                    if (r >= (h * NR) / SPC && r < ((h + 1) * NR) / SPC) issue_patch_round(pb ^ 1, r);
                if (h == SPC - 1) patch_advance();
            }
            if (s + 1 < S2) issue_b(bb ^ 1);
#pragma unroll
            for (int t = 0; t < TPS; ++t) compute(pb, bb, h * TPS + t);
            bb ^= 1;
        }
    }

    // ---------------- epilogue (conv_epilogue.hpp; one staging pass, fully unrolled store loop) ----------------
    constexpr int CPITCH = BN * 2 + 16;                // BM rows x 272 B = 34 | 68 KB <= the 48 | 72 KB of stage buffers
    static_assert(BM * CPITCH <= 2 * GP_PBUF + NB * BSTAGE, "C tile does not fit in LDS");
    static_assert(!OVL || (BM * CPITCH <= 2 * GP_PBUF && WM * BN * 8 <= 2 * GP_PBUF), "C tile / statistics scratch would overwrite the overlaid pixel table");
    gg_epilogue<VG_BF16, BM, BN, WM, WN, NT, 1, CPITCH, true>(d, acc, smem, opix_tab, GgWhere{tid, wm, wn, fr, fg, phase, bx, m_tiles_, M, GHW, m0, n0});
}

inline bool use_patch() { return vg_sw().gg_patch != 0; }      // VG_GG_PATCH (common.hpp: switches are read once at load)

// Does the descriptor have one of the two patch forms, and does a bm-row tiling (128 or 256) line up?
inline bool patch_geometry(const vg_gg_desc* d, int bm, PatchGeo* g) {
    const bool transposed = d->TH == 2 && d->TW == 2 && d->SY == 1 && d->SX == 1 && (d->DY == 1 || d->DY == -1) &&
                            (d->DX == 1 || d->DX == -1);
    const bool direct2 = d->TH == 4 && d->TW == 4 && d->SY == 2 && d->SX == 2 && d->DY == 1 && d->DX == 1 &&
                         d->nphase == 1;
    if (!transposed && !direct2) return false;
    if (d->IC % 32 != 0 || d->Kp != d->TH * d->TW * d->IC) return false;
    const int GW = d->GW, GH = d->GH;
    if (GW < 4 || GW > 64 || (GW & (GW - 1)) || (GH & (GH - 1))) return false;
    const int64_t M = (int64_t)d->B * GH * GW;
    if (M % bm != 0) return false;
    int R, IMGS;
    if (GH * GW >= bm) { IMGS = 1; R = bm / GW; if (R < 1 || GH % R) return false; }
    else { IMGS = bm / (GH * GW); R = GH; }
    g->R = R; g->IMGS = IMGS; g->PW = GW + 1; g->PIMG = (R + 1) * (GW + 1); g->NPP = IMGS * g->PIMG;
    if (g->NPP > (bm == 256 ? 384 : 256)) return false;
    g->ncy = d->TH / 2; g->ncx = d->TW / 2; g->nct = d->IC / 32;
    return true;
}
