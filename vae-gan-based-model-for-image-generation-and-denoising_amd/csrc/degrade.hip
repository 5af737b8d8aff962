// Degraded-pair data path (dataset_code.py:13-65, CelebADatasetV0.add_noise / add_random_rectangle): ONE pass over the
// HBM-resident u8 image set writes the clean batch, the degraded batch (random rectangle of uniform noise, Gaussian noise
// with a per-image standard deviation, clamp to [-1, 1]) and, optionally, the degraded batch in the engine's NHWC layout.
// Streaming kernel: at S = 64, C = 3 an image is 12 KB read and 96 KB (+ 64 KB NHWC bf16) written.  The draw contract
// (which Philox word feeds which number) is stated in include/vaegan_hip.h, "Degraded pairs".
// Noise models (vg_gather_degrade_u8_ex): both gather kernels are templated on <KIND, IMP> -- the factor the normal is
// scaled by (1, g, sqrt(g)) and whether impulses are laid on top.  <VG_NOISE_GAUSSIAN, false> is the reference's model and
// the only instantiation vg_gather_degrade_u8 launches; every line the other models add sits behind `if constexpr`.
#include "common.hpp"
#include "noise.hpp"

namespace {

struct DegradeGeom { int rect, min_size, max_size, x0, x1, y0, y1; };
struct DegradeImage { float s; int rh, rw, x, y; };        // one image's parameters (draw VG_DRAW_DEGRADE_PARAMS)

// u = (w >> 8) * 2^-24 in [0, 1): exact in f32 (24 significant bits)
__device__ __forceinline__ float u01_from_word(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }
// integer in [lo, hi), hi > lo: lo + floor(u * (hi - lo)) in integer arithmetic
__device__ __forceinline__ int int_from_word(uint32_t w, int lo, int hi) {
    return lo + (int)(((unsigned long long)(w >> 8) * (unsigned long long)(uint32_t)(hi - lo)) >> 24);
}

// Uniform over the image (and over the workgroup: every argument derives from blockIdx and kernel arguments, so the
// compiler keeps the two Philox blocks on the scalar unit).
__device__ __forceinline__ DegradeImage degrade_image(unsigned long long seed, unsigned long long pos, const DegradeGeom& g) {
    uint32_t w[4];
    philox4x32_10(seed, pos, VG_DRAW_DEGRADE_PARAMS, 0ull, w);
    DegradeImage p;
    p.s = u01_from_word(w[0]);
    p.rh = p.rw = p.x = p.y = 0;
    if (g.rect) {
        p.rh = int_from_word(w[1], g.min_size, g.max_size + 1);
        p.rw = int_from_word(w[2], g.min_size, g.max_size + 1);
        p.x = int_from_word(w[3], g.x0, g.x1 - p.rw);
        uint32_t v[4];
        philox4x32_10(seed, pos, VG_DRAW_DEGRADE_PARAMS, 1ull, v);
        p.y = int_from_word(v[0], g.y0, g.y1 - p.rh);
    }
    return p;
}

// ToTensor (u / 255), then Normalize((0.5,), (0.5,)) when `normalize`: the arithmetic of gather_u8_kernel (pointwise.hip)
__device__ __forceinline__ float byte_to_float(uint32_t u, int normalize) {
    const float t = __fdiv_rn((float)u, 255.0f);
    return normalize ? __fdiv_rn(__fsub_rn(t, 0.5f), 0.5f) : t;
}
// add_noise: (rectangle pixel: 2u - 1 replaces the image) + (n * s) * noise_max_std, clamp; every product and sum rounded
// on its own, as the f32 tensor expressions of the reference round.  hipcc contracts a * b + c into an FMA by default, and
// the __f*_rn intrinsics are inline functions of plain operators to it, so the expressions are written with operators
// under a pragma that switches contraction off for them (the pragma binds lexically, not through calls).
__device__ __forceinline__ float degrade_value(float clean, bool in_rect, uint32_t fill_word, float n, float s, float nms) {
#pragma clang fp contract(off)
    const float base = in_rect ? u01_from_word(fill_word) * 2.0f - 1.0f : clean;
    const float t = base + (n * s) * nms;
    return fminf(fmaxf(t, -1.0f), 1.0f);
}
// The signal-dependent models: the same sum with the noise term scaled by f = g (speckle) or sqrt(g) (shot), g the base
// value mapped to [0, 1] -- (n * s) * nms stays the standard deviation at white.  max(., 0): with normalize == 0 a
// rectangle fill 2u - 1 can be negative.  The quotient divides by 2 or 1 and is exact.  The root is the correctly rounded one:
// sqrtf, which hipcc expands to v_sqrt_f32 plus the fma correction steps (-fhip-fp32-correctly-rounded-divide-sqrt, its
// default).  NOT __fsqrt_rn: in this toolchain's headers that name is the native root, 1 ulp, unless the rounded OCML
// operations are compiled in -- the bitwise test of the shot model caught the difference.
template <int KIND>
__device__ __forceinline__ float degrade_value_scaled(float clean, bool in_rect, uint32_t fill_word, float n, float s, float nms,
                                                      int normalize) {
#pragma clang fp contract(off)
    const float base = in_rect ? u01_from_word(fill_word) * 2.0f - 1.0f : clean;
    const float lo = normalize ? -1.0f : 0.0f, span = normalize ? 2.0f : 1.0f;
    const float g = fmaxf((base - lo) / span, 0.0f);
    const float f = KIND == VG_NOISE_SPECKLE ? g : sqrtf(g);
    const float t = base + ((n * s) * nms) * f;
    return fminf(fmaxf(t, -1.0f), 1.0f);
}
template <int KIND>
__device__ __forceinline__ float degrade_model_value(float clean, bool in_rect, uint32_t fill_word, float n, float s, float nms,
                                                     int normalize) {
    if constexpr (KIND == VG_NOISE_GAUSSIAN) return degrade_value(clean, in_rect, fill_word, n, s, nms);
    else return degrade_value_scaled<KIND>(clean, in_rect, fill_word, n, s, nms, normalize);
}
// Impulses (salt and pepper) of one image: element e is hit when u01(word(VG_DRAW_DEGRADE_IMPULSE, e)) < p_b, p_b = s * impulse_max_p,
// and becomes 1 when u01(word(VG_DRAW_DEGRADE_SALT, e)) < salt_ratio, else the value mapping's black.
struct DegradeImpulse { float max_p, salt_ratio; };
__device__ __forceinline__ uint32_t word_of(const uint32_t (&w)[4], uint32_t sel) {
    return sel == 0 ? w[0] : sel == 1 ? w[1] : sel == 2 ? w[2] : w[3];
}

// Four consecutive pixels of a row per thread (W % 4 == 0, C <= 4): C dword loads of the 4 * C source bytes, one Philox
// block per channel for the four normals (and one more for the fill uniforms where the quad touches the rectangle),
// float4 stores to every plane of clean / noisy, one pixel store per NHWC pixel.  bpi: workgroups per image.
template <int C, int DT, int KIND, bool IMP>
__global__ __launch_bounds__(256) void gather_degrade_x4_kernel(const uint8_t* __restrict__ images,
                                                                const int64_t* __restrict__ idx, int64_t N, int W, int HW,
                                                                int bpi, unsigned long long seed, unsigned long long pos0,
                                                                float nms, int normalize, DegradeGeom g,
                                                                float* __restrict__ clean, float* __restrict__ noisy,
                                                                void* __restrict__ nhwc, int CP, DegradeImpulse imp) {
    const int b = blockIdx.x / bpi;
    const int q = (blockIdx.x - b * bpi) * 256 + threadIdx.x;
    const int Q = HW >> 2;
    if (q >= Q) return;
    const unsigned long long pos = pos0 + (unsigned long long)b;
    const DegradeImage im = degrade_image(seed, pos, g);
    int64_t n = idx[b];
    if (n < 0 || n >= N) n = 0;                        // never read outside the dataset (host validates too)
    const int p = q << 2;
    const int h = p / W;
    const int w0 = p - h * W;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(images + (n * HW + p) * C);
    uint32_t raw[C];
#pragma unroll
    for (int k = 0; k < C; ++k) raw[k] = src[k];
    const bool touches = h >= im.y && h < im.y + im.rh && w0 + 4 > im.x && w0 < im.x + im.rw;
    float v[4][4];                                     // [pixel][channel], the degraded values
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (c < C) {
            const unsigned long long blk = (unsigned long long)c * (unsigned long long)Q + (unsigned long long)q;
            const Normal4 nz = philox_randn4(seed, pos, VG_DRAW_DEGRADE_NORMAL, blk);
            uint32_t fw[4] = {0u, 0u, 0u, 0u};
            if (touches) philox4x32_10(seed, pos, VG_DRAW_DEGRADE_FILL, blk, fw);
            float cl[4];
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                const int k = px * C + c;              // byte k of the 4 * C loaded
                cl[px] = byte_to_float((raw[k >> 2] >> (8 * (k & 3))) & 0xffu, normalize);
                const bool in_rect = touches && w0 + px >= im.x && w0 + px < im.x + im.rw;
                v[px][c] = degrade_model_value<KIND>(cl[px], in_rect, fw[px], nz.v[px], im.s, nms, normalize);
            }
            if constexpr (IMP) {                       // the impulse words of the quad: one block, as the fill's
                const float p_b = __fmul_rn(im.s, imp.max_p);
                uint32_t iw[4];
                philox4x32_10(seed, pos, VG_DRAW_DEGRADE_IMPULSE, blk, iw);
                bool hit[4], any = false;
#pragma unroll
                for (int px = 0; px < 4; ++px) { hit[px] = u01_from_word(iw[px]) < p_b; any = any || hit[px]; }
                if (any) {
                    uint32_t sw[4];
                    philox4x32_10(seed, pos, VG_DRAW_DEGRADE_SALT, blk, sw);
#pragma unroll
                    for (int px = 0; px < 4; ++px)
                        if (hit[px]) v[px][c] = u01_from_word(sw[px]) < imp.salt_ratio ? 1.0f : (normalize ? -1.0f : 0.0f);
                }
            }
            const int64_t dst = ((int64_t)b * C + c) * HW + p;
            *reinterpret_cast<float4*>(clean + dst) = float4{cl[0], cl[1], cl[2], cl[3]};
            *reinterpret_cast<float4*>(noisy + dst) = float4{v[0][c], v[1][c], v[2][c], v[3][c]};
        } else {
#pragma unroll
            for (int px = 0; px < 4; ++px) v[px][c] = 0.f;
        }
    }
    if (nhwc == nullptr) return;
    const int64_t pix0 = (int64_t)b * HW + p;
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        if (DT == VG_BF16 && CP == 8) {                // 8 bf16 channels = one 16-byte pixel
            u32x4 o;
            o[0] = (uint32_t)ElemT<VG_BF16>::from_f32(v[px][0]) | ((uint32_t)ElemT<VG_BF16>::from_f32(v[px][1]) << 16);
            o[1] = (uint32_t)ElemT<VG_BF16>::from_f32(v[px][2]) | ((uint32_t)ElemT<VG_BF16>::from_f32(v[px][3]) << 16);
            o[2] = 0u; o[3] = 0u;
            *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned char*>(nhwc) + (pix0 + px) * 16) = o;
        } else {
            store4<DT>(nhwc, (pix0 + px) * CP, float4{v[px][0], v[px][1], v[px][2], v[px][3]});
            for (int c0 = 4; c0 < CP; c0 += 4) store4<DT>(nhwc, (pix0 + px) * CP + c0, float4{0.f, 0.f, 0.f, 0.f});
        }
    }
}

// One pixel per thread, any W and C: the same expressions element by element (philox_randn is the one-element form of
// philox_randn4; a fill uniform is word e & 3 of block e >> 2), so both kernels write the same bits.
template <int DT, int KIND, bool IMP>
__global__ __launch_bounds__(256) void gather_degrade_kernel(const uint8_t* __restrict__ images,
                                                             const int64_t* __restrict__ idx, int64_t N, int C, int W, int HW,
                                                             int bpi, unsigned long long seed, unsigned long long pos0,
                                                             float nms, int normalize, DegradeGeom g,
                                                             float* __restrict__ clean, float* __restrict__ noisy,
                                                             void* __restrict__ nhwc, int CP, DegradeImpulse imp) {
    const int b = blockIdx.x / bpi;
    const int p = (blockIdx.x - b * bpi) * 256 + threadIdx.x;
    if (p >= HW) return;
    const unsigned long long pos = pos0 + (unsigned long long)b;
    const DegradeImage im = degrade_image(seed, pos, g);
    int64_t n = idx[b];
    if (n < 0 || n >= N) n = 0;
    const int h = p / W;
    const int w = p - h * W;
    const uint8_t* src = images + (n * HW + p) * C;
    const bool in_rect = h >= im.y && h < im.y + im.rh && w >= im.x && w < im.x + im.rw;
    const int cend = nhwc ? CP : C;                    // CP >= C, CP % 4 == 0
    for (int c0 = 0; c0 < cend; c0 += 4) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + k;
            v[k] = 0.f;
            if (c < C) {
                const unsigned long long e = (unsigned long long)c * (unsigned long long)HW + (unsigned long long)p;
                const float cl = byte_to_float(src[c], normalize);
                uint32_t fw[4] = {0u, 0u, 0u, 0u};
                if (in_rect) philox4x32_10(seed, pos, VG_DRAW_DEGRADE_FILL, e >> 2, fw);
                const uint32_t sel = (uint32_t)(e & 3ull);
                const uint32_t fword = sel == 0 ? fw[0] : sel == 1 ? fw[1] : sel == 2 ? fw[2] : fw[3];
                v[k] = degrade_model_value<KIND>(cl, in_rect, fword, philox_randn(seed, pos, VG_DRAW_DEGRADE_NORMAL, e), im.s, nms,
                                                 normalize);
                if constexpr (IMP) {
                    uint32_t iw[4];
                    philox4x32_10(seed, pos, VG_DRAW_DEGRADE_IMPULSE, e >> 2, iw);
                    if (u01_from_word(word_of(iw, sel)) < __fmul_rn(im.s, imp.max_p)) {
                        uint32_t sw[4];
                        philox4x32_10(seed, pos, VG_DRAW_DEGRADE_SALT, e >> 2, sw);
                        v[k] = u01_from_word(word_of(sw, sel)) < imp.salt_ratio ? 1.0f : (normalize ? -1.0f : 0.0f);
                    }
                }
                const int64_t dst = ((int64_t)b * C + c) * HW + p;
                clean[dst] = cl;
                noisy[dst] = v[k];
            }
        }
        if (nhwc) store4<DT>(nhwc, ((int64_t)b * HW + p) * CP + c0, float4{v[0], v[1], v[2], v[3]});
    }
}

__global__ __launch_bounds__(256) void degrade_params_kernel(unsigned long long seed, unsigned long long pos0, int B, float nms,
                                                             DegradeGeom g, float* __restrict__ out, float impulse_max_p,
                                                             int kind) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const DegradeImage im = degrade_image(seed, pos0 + (unsigned long long)b, g);
    float* o = out + (int64_t)b * 8;
    o[0] = im.s; o[1] = __fmul_rn(im.s, nms);
    o[2] = (float)im.rh; o[3] = (float)im.rw; o[4] = (float)im.x; o[5] = (float)im.y;
    o[6] = __fmul_rn(im.s, impulse_max_p); o[7] = (float)kind;      // the reference's model: s * 0 = +0 and 0, as ever
}

__global__ __launch_bounds__(256) void rand_u01_fill_kernel(float* __restrict__ out, int64_t n,
                                                            const unsigned long long* __restrict__ rng, uint32_t draw) {
    const unsigned long long seed = rng[0], step = rng[1];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t w[4];
        philox4x32_10(seed, step, draw, (unsigned long long)i >> 2, w);
        const uint32_t sel = (uint32_t)(i & 3);
        out[i] = u01_from_word(sel == 0 ? w[0] : sel == 1 ? w[1] : sel == 2 ? w[2] : w[3]);
    }
}

// bounds as data.degrade_bounds makes them; the sampled ranges must not be empty and the rectangle must lie in the image
bool geom_ok(const DegradeGeom& g, int H, int W) {
    if (!g.rect) return true;
    return g.min_size >= 0 && g.max_size >= g.min_size && g.x0 >= 0 && g.y0 >= 0 && g.x1 - g.max_size > g.x0 &&
           g.y1 - g.max_size > g.y0 && g.x1 - 1 <= W && g.y1 - 1 <= H;
}

// every position pos0 .. pos0 + B - 1 (B > 0) below 2^56: the counter word that carries pos >> 32 keeps its low byte for the
// draw id, and a position of 2^56 would wrap onto position 0
bool positions_ok(uint64_t pos0, int B) { return (pos0 >> 56) == 0 && ((pos0 + (uint64_t)(B - 1)) >> 56) == 0; }

}  // namespace

extern "C" int vg_rand_u01(float* out, int64_t n, const uint64_t* rng, int draw, void* stream) {
    VG_CHECK_ARG(out && rng && n > 0 && draw >= 0 && draw < 256, VG_EINVAL);
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(rand_u01_fill_kernel, dim3((unsigned)blocks), dim3(256), 0, vg_stream(stream), out, n,
                       (const unsigned long long*)rng, (uint32_t)draw);
    return VG_LAUNCH_RC();
}

namespace {

struct GatherArgs {
    const uint8_t* images; int64_t N; const int64_t* idx; int B, C, H, W; uint64_t seed, pos0; float noise_max_std;
    int normalize; DegradeGeom g; float* clean; float* noisy; void* nhwc; int CP, dtype; void* stream;
};

// the launch of one model: the argument checks of both entry points, then the quad or the scalar kernel of <KIND, IMP>
template <int KIND, bool IMP>
int gather_degrade_launch(const GatherArgs& a, DegradeImpulse imp) {
    const uint8_t* images = a.images;
    const int64_t* idx = a.idx;
    const int64_t N = a.N;
    const int B = a.B, C = a.C, H = a.H, W = a.W, normalize = a.normalize, CP = a.CP;
    int dtype = a.dtype;
    const DegradeGeom g = a.g;
    float *clean = a.clean, *noisy = a.noisy;
    void* nhwc = a.nhwc;
    const float noise_max_std = a.noise_max_std;
    VG_CHECK_ARG(images && idx && clean && noisy && N > 0 && B > 0 && C > 0 && H > 0 && W > 0 && positions_ok(a.pos0, B) &&
                 (int64_t)H * W < (1ll << 30) && geom_ok(g, H, W), VG_EINVAL);
    if (nhwc) {
        VG_CHECK_ARG(dtype == VG_F32 || dtype == VG_BF16, VG_ENOSUP);
        VG_CHECK_ARG(CP >= C && CP % 4 == 0, VG_EINVAL);
        VG_CHECK_ARG(vg_aligned16(nhwc), VG_EALIGN);
    } else {
        dtype = VG_F32;
    }
    const int HW = H * W;
    const unsigned long long s = a.seed, p0 = a.pos0;
    const bool quad = W % 4 == 0 && C <= 4 && vg_aligned16(clean) && vg_aligned16(noisy) &&
                      (reinterpret_cast<uintptr_t>(images) & 3u) == 0;
    const int units = quad ? HW / 4 : HW;
    const int bpi = (units + 255) / 256;
    VG_CHECK_ARG((int64_t)B * bpi < (1ll << 31), VG_EINVAL);
    const dim3 grid((unsigned)((int64_t)B * bpi)), block(256);
    hipStream_t st = vg_stream(a.stream);
#define DEGRADE_X4(CC)                                                                                                     \
    do {                                                                                                                   \
        if (dtype == VG_F32)                                                                                               \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(gather_degrade_x4_kernel<CC, VG_F32, KIND, IMP>), grid, block, 0, st, images, idx, N, W,  \
                               HW, bpi, s, p0, noise_max_std, normalize, g, clean, noisy, nhwc, CP, imp);                  \
        else                                                                                                               \
            hipLaunchKernelGGL(HIP_KERNEL_NAME(gather_degrade_x4_kernel<CC, VG_BF16, KIND, IMP>), grid, block, 0, st, images, idx, N, W, \
                               HW, bpi, s, p0, noise_max_std, normalize, g, clean, noisy, nhwc, CP, imp);                  \
    } while (0)
    if (quad) {
        switch (C) {
            case 1: DEGRADE_X4(1); break;
            case 2: DEGRADE_X4(2); break;
            case 3: DEGRADE_X4(3); break;
            default: DEGRADE_X4(4); break;
        }
    } else if (dtype == VG_F32) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gather_degrade_kernel<VG_F32, KIND, IMP>), grid, block, 0, st, images, idx, N, C, W, HW,
                           bpi, s, p0, noise_max_std, normalize, g, clean, noisy, nhwc, CP, imp);
    } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gather_degrade_kernel<VG_BF16, KIND, IMP>), grid, block, 0, st, images, idx, N, C, W, HW,
                           bpi, s, p0, noise_max_std, normalize, g, clean, noisy, nhwc, CP, imp);
    }
#undef DEGRADE_X4
    return VG_LAUNCH_RC();
}

// kind in 0..2, both probabilities finite and in [0, 1] (a NaN fails every comparison)
bool model_ok(int kind, float impulse_max_p, float salt_ratio) {
    return kind >= VG_NOISE_GAUSSIAN && kind <= VG_NOISE_SHOT && impulse_max_p >= 0.f && impulse_max_p <= 1.f &&
           salt_ratio >= 0.f && salt_ratio <= 1.f;
}

}  // namespace

extern "C" int vg_degrade_params(uint64_t seed, uint64_t pos0, int B, float noise_max_std, int rect, int H, int W,
                                 int min_size, int max_size, int x0, int x1, int y0, int y1, float* out, void* stream) {
    return vg_degrade_params_ex(seed, pos0, B, noise_max_std, rect, H, W, min_size, max_size, x0, x1, y0, y1, out,
                                VG_NOISE_GAUSSIAN, 0.f, 0.5f, stream);
}

extern "C" int vg_degrade_params_ex(uint64_t seed, uint64_t pos0, int B, float noise_max_std, int rect, int H, int W,
                                    int min_size, int max_size, int x0, int x1, int y0, int y1, float* out, int kind,
                                    float impulse_max_p, float salt_ratio, void* stream) {
    const DegradeGeom g{rect ? 1 : 0, min_size, max_size, x0, x1, y0, y1};
    VG_CHECK_ARG(out && B > 0 && H > 0 && W > 0 && positions_ok(pos0, B) && geom_ok(g, H, W), VG_EINVAL);
    VG_CHECK_ARG(model_ok(kind, impulse_max_p, salt_ratio), VG_EINVAL);
    hipLaunchKernelGGL(degrade_params_kernel, dim3((B + 255) / 256), dim3(256), 0, vg_stream(stream),
                       (unsigned long long)seed, (unsigned long long)pos0, B, noise_max_std, g, out, impulse_max_p, kind);
    return VG_LAUNCH_RC();
}

extern "C" int vg_gather_degrade_u8(const uint8_t* images, int64_t N, const int64_t* idx, int B, int C, int H, int W,
                                    uint64_t seed, uint64_t pos0, float noise_max_std, int rect, int normalize,
                                    int min_size, int max_size, int x0, int x1, int y0, int y1, float* clean,
                                    float* noisy, void* nhwc, int CP, int dtype, void* stream) {
    const GatherArgs a{images, N, idx, B, C, H, W, seed, pos0, noise_max_std, normalize,
                       DegradeGeom{rect ? 1 : 0, min_size, max_size, x0, x1, y0, y1}, clean, noisy, nhwc, CP, dtype, stream};
    return gather_degrade_launch<VG_NOISE_GAUSSIAN, false>(a, DegradeImpulse{0.f, 0.f});
}

extern "C" int vg_gather_degrade_u8_ex(const uint8_t* images, int64_t N, const int64_t* idx, int B, int C, int H, int W,
                                       uint64_t seed, uint64_t pos0, float noise_max_std, int rect, int normalize,
                                       int min_size, int max_size, int x0, int x1, int y0, int y1, float* clean,
                                       float* noisy, void* nhwc, int CP, int dtype, int kind, float impulse_max_p,
                                       float salt_ratio, void* stream) {
    VG_CHECK_ARG(model_ok(kind, impulse_max_p, salt_ratio), VG_EINVAL);
    const GatherArgs a{images, N, idx, B, C, H, W, seed, pos0, noise_max_std, normalize,
                       DegradeGeom{rect ? 1 : 0, min_size, max_size, x0, x1, y0, y1}, clean, noisy, nhwc, CP, dtype, stream};
    const DegradeImpulse imp{impulse_max_p, salt_ratio};
    if (impulse_max_p > 0.f) {
        switch (kind) {
            case VG_NOISE_GAUSSIAN: return gather_degrade_launch<VG_NOISE_GAUSSIAN, true>(a, imp);
            case VG_NOISE_SPECKLE: return gather_degrade_launch<VG_NOISE_SPECKLE, true>(a, imp);
            default: return gather_degrade_launch<VG_NOISE_SHOT, true>(a, imp);
        }
    }
    switch (kind) {
        case VG_NOISE_GAUSSIAN: return gather_degrade_launch<VG_NOISE_GAUSSIAN, false>(a, imp);   // the old entry's kernels
        case VG_NOISE_SPECKLE: return gather_degrade_launch<VG_NOISE_SPECKLE, false>(a, imp);
        default: return gather_degrade_launch<VG_NOISE_SHOT, false>(a, imp);
    }
}

