// Resize + CenterCrop of the HBM-resident u8 image set (dataset_code.py:26-30, CelebADatasetV0's transforms.Resize +
// transforms.CenterCrop): PIL's 8-bit bilinear resampler (ImagingResample, triangle filter) restated as integer arithmetic
// over two host-built coefficient tables; the contract is in include/vaegan_hip.h, "Resize".  Output equals PIL's byte for
// byte.  One launch, two passes through LDS, no intermediate in HBM:
//   a workgroup owns one image and a band of output rows.  It stages the input rows the band's vertical taps read -- only
//   the columns the crop window's horizontal taps read -- into LDS with dword loads, RS rows at a time, runs the horizontal
//   pass from that staging area into an LDS image [rows][cw][C] in u8, and after a barrier runs the vertical pass from the
//   LDS image and stores the band, which is one contiguous run of dst, as dwords.
// A skipped pass (null table) runs as the one-tap identity k = 2^PB, which the pass arithmetic maps to the byte itself.
#include "common.hpp"

namespace {

constexpr int PB = 22;                       // PIL's PRECISION_BITS = 32 - 8 - 2
constexpr int RESIZE_THREADS = 256;
constexpr int RESIZE_ROWS = 4;               // input rows one thread carries through the horizontal taps of its column
constexpr int LDS_SOFT = 40 * 1024;          // 4 workgroups per CU (160 KiB); the band height aims at this
constexpr int LDS_HARD = 64 * 1024;          // >= 2 workgroups per CU; beyond it the geometry is not served
constexpr int MIN_WGS = 512;                 // 2 workgroups on each of the 256 CUs before bands stop shrinking

struct ResizeArgs {
    const uint8_t* src;
    const int64_t* idx;
    int64_t N, total;                        // total = N * Hin * Win * C bytes
    int Hin, Win;
    const int32_t *kh, *bh, *kv, *bv;
    int ksh, ksv, top, left;
    uint8_t* dst;
    int ch, cw;
    int band, nbands, rows_max;              // output rows per band, bands per image, most input rows a band reads
    int c0, ncolsB;                          // first input column read, bytes read per input row
    int SP, IP, RS;                          // staging / LDS-image row pitch in bytes (multiples of 4), staged rows per round
    int dword_out;                           // cw * C % 4 == 0 and dst 4-byte aligned: the band is stored as dwords
};

struct ResizePlan { int band, nbands, rows_max, c0, ncolsB, SP, IP, RS; int64_t lds; };

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> PB, 0), 255); }

template <int C>
__global__ __launch_bounds__(RESIZE_THREADS) void resize_u8_kernel(ResizeArgs a) {
    extern __shared__ uint32_t lds32[];
    uint8_t* inter = reinterpret_cast<uint8_t*>(lds32);                 // [rows_max][IP]
    uint32_t* stage32 = lds32 + (((size_t)a.rows_max * a.IP) >> 2);     // [RS][SP], read and written as dwords only
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.nbands;
    const int y0 = (blockIdx.x - b * a.nbands) * a.band;
    const int y1 = min(y0 + a.band, a.ch);
    int64_t n = a.idx ? a.idx[b] : (int64_t)b;
    if (n < 0 || n >= a.N) n = 0;                                       // never read outside the set (host validates too)
    // input rows [r0, r1) the band reads; the clamps only bite if the device tables differ from the host's validated copy
    int r0 = a.bv ? a.bv[2 * y0] : a.top + y0;
    int r1 = a.bv ? a.bv[2 * (y1 - 1)] + a.bv[2 * (y1 - 1) + 1] : a.top + y1;
    r0 = min(max(r0, 0), a.Hin - 1);
    r1 = min(max(r1, r0 + 1), min(a.Hin, r0 + a.rows_max));
    const int nrows = r1 - r0;
    const int64_t img = n * ((int64_t)a.Hin * a.Win * C);
    const int SPd = a.SP >> 2;
    const int c1 = a.c0 + a.ncolsB / C;                                 // one past the last input column staged

    for (int cr = 0; cr < nrows; cr += a.RS) {
        const int rc = min(a.RS, nrows - cr);
        // stage rc input rows: dword loads from the dword at or below each row window's first byte
        for (int i = tid; i < rc * SPd; i += RESIZE_THREADS) {
            const int row = i / SPd, d = i - row * SPd;
            const int64_t rb = img + ((int64_t)(r0 + cr + row) * a.Win + a.c0) * C;
            const int64_t ab = (rb & ~(int64_t)3) + 4 * (int64_t)d;
            if (ab < rb + a.ncolsB) {
                uint32_t v;
                if (ab + 4 <= a.total) {
                    v = *reinterpret_cast<const uint32_t*>(a.src + ab);
                } else {                                                // the set's last dword may be a partial one
                    v = 0;
                    for (int k = 0; k < 4; ++k)
                        if (ab + k < a.total) v |= (uint32_t)a.src[ab + k] << (8 * k);
                }
                stage32[row * SPd + d] = v;
            }
        }
        __syncthreads();
        // horizontal pass: one thread = one output column x of RESIZE_ROWS staged rows (a coefficient is loaded once for them)
        const int ngroups = (rc + RESIZE_ROWS - 1) / RESIZE_ROWS;
        for (int i = tid; i < ngroups * a.cw; i += RESIZE_THREADS) {
            const int g = i / a.cw, x = i - g * a.cw;
            int xmin = a.bh ? a.bh[2 * x] : a.left + x;
            int nt = a.bh ? a.bh[2 * x + 1] : 1;
            xmin = min(max(xmin, a.c0), c1 - 1);
            nt = min(nt, min(a.bh ? a.ksh : 1, c1 - xmin));
            int base[RESIZE_ROWS], acc[RESIZE_ROWS][C];
#pragma unroll
            for (int rr = 0; rr < RESIZE_ROWS; ++rr) {
                const int row = min(g * RESIZE_ROWS + rr, rc - 1);
                const uint32_t shift = ((uint32_t)img + ((uint32_t)(r0 + cr + row) * (uint32_t)a.Win + (uint32_t)a.c0) * C) & 3u;
                base[rr] = row * a.SP + (int)shift + (xmin - a.c0) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) acc[rr][c] = 1 << (PB - 1);
            }
            for (int t = 0; t < nt; ++t) {
                const int k = a.kh ? a.kh[x * a.ksh + t] : (1 << PB);
#pragma unroll
                for (int rr = 0; rr < RESIZE_ROWS; ++rr) {
                    // the C <= 4 bytes of a tap lie in two adjacent dwords: two aligned reads, one funnel shift
                    const int p = base[rr] + t * C;
                    const uint32_t lo = stage32[p >> 2], hi = stage32[(p >> 2) + 1];
                    const uint32_t px = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (p & 3)));
#pragma unroll
                    for (int c = 0; c < C; ++c) acc[rr][c] += (int)((px >> (8 * c)) & 255u) * k;
                }
            }
#pragma unroll
            for (int rr = 0; rr < RESIZE_ROWS; ++rr) {
                const int row = g * RESIZE_ROWS + rr;
                if (row < rc) {
                    uint8_t* o = inter + (cr + row) * a.IP + x * C;
#pragma unroll
                    for (int c = 0; c < C; ++c) o[c] = (uint8_t)clip8(acc[rr][c]);
                }
            }
        }
        __syncthreads();
    }

    // vertical pass from the LDS image; the band's rows are adjacent in dst
    const int rowB = a.cw * C;
    const int nb = (y1 - y0) * rowB;
    uint8_t* out = a.dst + ((int64_t)b * a.ch + y0) * rowB;
    if (a.dword_out) {
        for (int q = tid; q < (nb >> 2); q += RESIZE_THREADS) {
            const int yy = (4 * q) / rowB, j = 4 * q - yy * rowB;
            const int y = y0 + yy;
            int ymin = a.bv ? a.bv[2 * y] : a.top + y;
            int nt = a.bv ? a.bv[2 * y + 1] : 1;
            ymin = min(max(ymin, r0), r1 - 1);
            nt = min(nt, min(a.bv ? a.ksv : 1, r1 - ymin));
            int a0 = 1 << (PB - 1), a1 = a0, a2 = a0, a3 = a0;
            const uint32_t* col = lds32 + (((ymin - r0) * a.IP + j) >> 2);
            const int IPd = a.IP >> 2;
            for (int t = 0; t < nt; ++t) {
                const int k = a.kv ? a.kv[y * a.ksv + t] : (1 << PB);
                const uint32_t w = col[t * IPd];
                a0 += (int)(w & 255u) * k;
                a1 += (int)((w >> 8) & 255u) * k;
                a2 += (int)((w >> 16) & 255u) * k;
                a3 += (int)(w >> 24) * k;
            }
            // The clipped bytes pass through an empty asm statement before they are packed: hipcc (ROCm 7.2) turns
            // clip8(a0) | clip8(a1) << 8 into v_ashr_pk_u8_i32 and assumes bits 31:16 of its result are zero; on the MI355X
            // they are not, and byte 2 of every stored dword came out OR-ed with them (found against the fixture).
            int c0 = clip8(a0), c1 = clip8(a1), c2 = clip8(a2), c3 = clip8(a3);
            asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
            const uint32_t o = (uint32_t)c0 | ((uint32_t)c1 << 8) | ((uint32_t)c2 << 16) | ((uint32_t)c3 << 24);
            *reinterpret_cast<uint32_t*>(out + 4 * (int64_t)q) = o;
        }
    } else {
        for (int e = tid; e < nb; e += RESIZE_THREADS) {
            const int yy = e / rowB, j = e - yy * rowB;
            const int y = y0 + yy;
            int ymin = a.bv ? a.bv[2 * y] : a.top + y;
            int nt = a.bv ? a.bv[2 * y + 1] : 1;
            ymin = min(max(ymin, r0), r1 - 1);
            nt = min(nt, min(a.bv ? a.ksv : 1, r1 - ymin));
            int acc = 1 << (PB - 1);
            const uint8_t* col = inter + (ymin - r0) * a.IP + j;
            for (int t = 0; t < nt; ++t) acc += (int)col[t * a.IP] * (a.kv ? a.kv[y * a.ksv + t] : (1 << PB));
            out[e] = (uint8_t)clip8(acc);
        }
    }
}

// bounds [out][2] = (xmin, n) as data.resample_coeffs makes them, restricted to the crop window: inside the input, at
// most ksize taps, windows moving forward (the band's row range and the staged column range are read off the ends)
bool bounds_ok(const int32_t* bd, int out, int ksize, int in_size) {
    if (ksize < 1) return false;
    int prev_lo = 0, prev_hi = 0;
    for (int i = 0; i < out; ++i) {
        const int lo = bd[2 * i], nt = bd[2 * i + 1];
        if (lo < 0 || nt < 1 || nt > ksize || lo > in_size - nt) return false;
        if (lo < prev_lo || lo + nt < prev_hi) return false;
        prev_lo = lo;
        prev_hi = lo + nt;
    }
    return true;
}

int band_rows(const int32_t* bv, int ch, int band) {
    if (!bv) return band < ch ? band : ch;
    int m = 0;
    for (int y0 = 0; y0 < ch; y0 += band) {
        const int y1 = (y0 + band < ch ? y0 + band : ch) - 1;
        const int r = bv[2 * y1] + bv[2 * y1 + 1] - bv[2 * y0];
        if (r > m) m = r;
    }
    return m;
}

// 0: served (plan filled), VG_EINVAL: arguments outside the contract or a geometry whose LDS image does not fit
int resize_plan(int Hin, int Win, int C, const int32_t* bh, int ksh, const int32_t* bv, int ksv, int top, int left, int ch,
                int cw, int B, int band, ResizePlan* p) {
    VG_CHECK_ARG(Hin > 0 && Win > 0 && C >= 1 && C <= 4 && ch > 0 && cw > 0 && B > 0 && band >= 0, VG_EINVAL);
    VG_CHECK_ARG((int64_t)Hin * Win * C < (1ll << 31) && (int64_t)ch * cw * C < (1ll << 31), VG_EINVAL);
    if (bh) VG_CHECK_ARG(bounds_ok(bh, cw, ksh, Win), VG_EINVAL);
    else VG_CHECK_ARG(left >= 0 && cw <= Win - left, VG_EINVAL);        // crop wider than the (unresized) image: rejected
    if (bv) VG_CHECK_ARG(bounds_ok(bv, ch, ksv, Hin), VG_EINVAL);
    else VG_CHECK_ARG(top >= 0 && ch <= Hin - top, VG_EINVAL);
    p->c0 = bh ? bh[0] : left;
    const int c1 = bh ? bh[2 * (cw - 1)] + bh[2 * (cw - 1) + 1] : left + cw;
    p->ncolsB = (c1 - p->c0) * C;
    // + 3: a row window may start 3 bytes into a dword; + 8: the dword pair read at a row's last tap stays inside the row
    p->SP = ((p->ncolsB + 3 + 3) / 4) * 4 + 8;
    p->IP = ((cw * C + 3) / 4) * 4;
    auto fit = [&](int bd, int limit) {
        const int rows = band_rows(bv, ch, bd);
        const int64_t inter = (int64_t)rows * p->IP;
        const int least = rows < RESIZE_ROWS ? rows : RESIZE_ROWS;
        if (inter + (int64_t)least * p->SP > limit) return false;
        int rs = (int)((limit - inter) / p->SP);
        if (rs >= rows) rs = rows;
        else rs -= rs % RESIZE_ROWS;
        if (rs > 16 && rs < rows) rs = 16;
        p->band = bd < ch ? bd : ch;
        p->rows_max = rows;
        p->RS = rs;
        p->lds = inter + (int64_t)rs * p->SP;
        return true;
    };
    bool ok = false;
    if (band > 0) {
        ok = fit(band, LDS_HARD);                                       // the caller's band height, or nothing
    } else {
        const int limits[2] = {LDS_SOFT, LDS_HARD};
        for (int li = 0; li < 2 && !ok; ++li) {
            int bd = 32;
            while (bd > 1 && !fit(bd, limits[li])) bd >>= 1;
            ok = fit(bd, limits[li]);
            // a small batch: shorter bands (more re-read rows) until the launch offers every CU two workgroups
            while (ok && bd > 8 && (int64_t)B * ((ch + bd - 1) / bd) < MIN_WGS) {
                bd >>= 1;
                ok = fit(bd, limits[li]);
            }
        }
    }
    VG_CHECK_ARG(ok, VG_EINVAL);
    p->nbands = (ch + p->band - 1) / p->band;
    VG_CHECK_ARG((int64_t)B * p->nbands < (1ll << 31), VG_EINVAL);
    return 0;
}

}  // namespace

extern "C" int64_t vg_resize_u8_lds_bytes(int Hin, int Win, int C, const int32_t* bh_host, int ksize_h, const int32_t* bv_host,
                                          int ksize_v, int top, int left, int ch, int cw, int B, int band) {
    ResizePlan p;
    const int rc = resize_plan(Hin, Win, C, bh_host, ksize_h, bv_host, ksize_v, top, left, ch, cw, B, band, &p);
    return rc ? rc : p.lds;
}

extern "C" int vg_resize_u8_band(int Hin, int Win, int C, const int32_t* bh_host, int ksize_h, const int32_t* bv_host,
                                 int ksize_v, int top, int left, int ch, int cw, int B, int band) {
    ResizePlan p;
    const int rc = resize_plan(Hin, Win, C, bh_host, ksize_h, bv_host, ksize_v, top, left, ch, cw, B, band, &p);
    return rc ? rc : p.band;
}

extern "C" int vg_resize_u8(const uint8_t* src, int64_t N, int Hin, int Win, int C, const int64_t* idx, int B,
                            const int32_t* kh, const int32_t* bh, const int32_t* bh_host, int ksize_h, const int32_t* kv,
                            const int32_t* bv, const int32_t* bv_host, int ksize_v, int top, int left, uint8_t* dst, int ch,
                            int cw, int band, void* stream) {
    VG_CHECK_ARG(src && dst && N > 0 && B > 0, VG_EINVAL);
    VG_CHECK_ARG(idx || (int64_t)B <= N, VG_EINVAL);
    // a pass has all three of its tables or none
    VG_CHECK_ARG((kh != nullptr) == (bh != nullptr) && (bh != nullptr) == (bh_host != nullptr), VG_EINVAL);
    VG_CHECK_ARG((kv != nullptr) == (bv != nullptr) && (bv != nullptr) == (bv_host != nullptr), VG_EINVAL);
    ResizePlan p;
    const int rc = resize_plan(Hin, Win, C, bh_host, ksize_h, bv_host, ksize_v, top, left, ch, cw, B, band, &p);
    if (rc) return rc;
    VG_CHECK_ARG(vg_aligned16(kh) && vg_aligned16(bh) && vg_aligned16(kv) && vg_aligned16(bv), VG_EALIGN);
    VG_CHECK_ARG((reinterpret_cast<uintptr_t>(src) & 3u) == 0 && (reinterpret_cast<uintptr_t>(idx) & 7u) == 0, VG_EALIGN);
    ResizeArgs a;
    a.src = src; a.idx = idx; a.N = N; a.total = N * ((int64_t)Hin * Win * C);
    a.Hin = Hin; a.Win = Win;
    a.kh = kh; a.bh = bh; a.kv = kv; a.bv = bv;
    a.ksh = ksize_h; a.ksv = ksize_v; a.top = top; a.left = left;
    a.dst = dst; a.ch = ch; a.cw = cw;
    a.band = p.band; a.nbands = p.nbands; a.rows_max = p.rows_max;
    a.c0 = p.c0; a.ncolsB = p.ncolsB; a.SP = p.SP; a.IP = p.IP; a.RS = p.RS;
    a.dword_out = ((cw * C) % 4 == 0 && (reinterpret_cast<uintptr_t>(dst) & 3u) == 0) ? 1 : 0;
    const dim3 grid((unsigned)((int64_t)B * p.nbands)), block(RESIZE_THREADS);
    hipStream_t st = vg_stream(stream);
    switch (C) {
        case 1: hipLaunchKernelGGL(resize_u8_kernel<1>, grid, block, (size_t)p.lds, st, a); break;
        case 2: hipLaunchKernelGGL(resize_u8_kernel<2>, grid, block, (size_t)p.lds, st, a); break;
        case 3: hipLaunchKernelGGL(resize_u8_kernel<3>, grid, block, (size_t)p.lds, st, a); break;
        default: hipLaunchKernelGGL(resize_u8_kernel<4>, grid, block, (size_t)p.lds, st, a); break;
    }
    return VG_LAUNCH_RC();
}
