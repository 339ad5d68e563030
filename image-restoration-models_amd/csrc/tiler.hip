// Device side of the tiled-patch loop (src/utils.py:353-454): cut an HWC
// uint8/uint16 image into equal-shape tiles (normalise, optional seeded noise,
// reflect pad to a multiple of 8 as utils.pad does), and blend the per-tile
// predictions back with the Gaussian window, divide by the weight map and
// requantise - all with the reference's float32 operation order so the result
// is bit-identical to the numpy code given identical predictions.
#include "irm_frame.h"

struct ExtractArgs {
    const void* img;       // [H][W][C] u8 or u16
    TileCut g;
    int is_u16;
    float scale;           // 255 or 65535
    float mean, inv_std;   // DeblurGANv2 normalize: v = (raw - mean) * inv_std on the RAW integer value; 0,1 = off
};

__global__ __launch_bounds__(256) void tile_extract_kernel(ExtractArgs a) {
    irm_extract_element(a.g, [&](long src) {
        const float raw = a.is_u16 ? (float)reinterpret_cast<const unsigned short*>(a.img)[src]
                                   : (float)reinterpret_cast<const unsigned char*>(a.img)[src];
        const bool albu = a.inv_std != 1.0f || a.mean != 0.0f;
        // utils.py:159-171, or albumentations Normalize (aug.py:31-39): (x - mean*255) * (1 / (std*255))
        return albu ? __fmul_rn(__fsub_rn(raw, a.mean), a.inv_std) : __fdiv_rn(raw, a.scale);
    });
}

extern "C" int irm_tile_extract(const void* img, int is_u16, const int* origins, const double* noise,
                                float* tiles, int H, int W, int C, int th, int tw, int ph, int pw, int T,
                                float mean, float inv_std, int pad_zero, hipStream_t stream) {
    const ExtractArgs a{img, {origins, noise, tiles, H, W, C, th, tw, ph, pw, T, pad_zero}, is_u16,
                        is_u16 ? 65535.0f : 255.0f, mean, inv_std};
    if (!irm_tile_cut_ok(img, a.g)) return IRM_EINVAL;
    hipLaunchKernelGGL(tile_extract_kernel, dim3(irm_tile_cut_blocks(a.g)), dim3(256), 0, stream, a);
    return irm_launch_status();
}

// ---------------------------------------------------------------------------
struct BlendArgs {
    TileBlend g;
    void* out;             // [H][W][Co] u8 / u16
    const void* target;    // optional [H][W][Co] for the squared error
    unsigned long long* sse;   // optional single accumulator (integer: order independent)
    int is_u16;
    float post_scale, post_shift;   // postprocess v*scale+shift (DeblurGANv2 (x+1)/2); 1,0 = off
};

// One workgroup blends BLEND_PER_WG consecutive output elements (256 threads x 8 rounds) and adds its squared error
// with ONE integer atomic: a frame of 1280x720x3 bytes takes 1 350 atomics on the single accumulator instead of one
// per wave (43 200 same-address atomics serialised at the L2: 0.5 ms of a 57 ms frame).  Integer sums: order independent.
#define BLEND_PER_WG 2048

// SCALED (irm_window_blend_scaled): every extent is already at output scale; only the origins are scaled in the walk.
template <bool SCALED>
__global__ __launch_bounds__(256) void blend_kernel(BlendArgs a) {
    const long total = (long)a.g.H * a.g.W * a.g.Co;
    unsigned long long err = 0;
    const bool albu = a.post_scale != 1.0f || a.post_shift != 0.0f;
    const float peak = a.is_u16 ? 65535.0f : 255.0f;
#pragma unroll 1
    for (int round = 0; round < BLEND_PER_WG / 256; ++round) {
        const long idx = (long)blockIdx.x * BLEND_PER_WG + round * 256 + threadIdx.x;
        if (idx >= total) break;
        float v = irm_blend_element<SCALED>(a.g, idx, [&](float p) {
            return albu ? __fmul_rn(__fadd_rn(p, a.post_shift), a.post_scale) : p;
        });
        v = rintf(fminf(fmaxf(__fmul_rn(v, peak), 0.0f), peak));   // clip, round half to even
        const unsigned q = (unsigned)v;
        if (a.is_u16) reinterpret_cast<unsigned short*>(a.out)[idx] = (unsigned short)q;
        else reinterpret_cast<unsigned char*>(a.out)[idx] = (unsigned char)q;
        if (a.target && a.sse) {
            const int tv = a.is_u16 ? reinterpret_cast<const unsigned short*>(a.target)[idx]
                                    : reinterpret_cast<const unsigned char*>(a.target)[idx];
            const long d = (long)q - tv;
            err += (unsigned long long)(d * d);
        }
    }
    if (a.target && a.sse) {
        // the workgroup's sum, then one integer atomic per workgroup
        __shared__ unsigned long long part[4];
        const unsigned long long s = irm_block_reduce256<FrSum>(err, part);
        if (threadIdx.x == 0 && s) atomicAdd(a.sse, s);
    }
}

template <bool SCALED>
static int launch_blend(BlendArgs a, hipStream_t stream) {
    if (!irm_tile_blend_plan(a.g, a.out, SCALED)) return IRM_EINVAL;
    const long total = (long)a.g.H * a.g.W * a.g.Co;
    hipLaunchKernelGGL(blend_kernel<SCALED>, dim3((unsigned)((total + BLEND_PER_WG - 1) / BLEND_PER_WG)), dim3(256), 0, stream, a);
    return irm_launch_status();
}

extern "C" int irm_window_blend(const float* pred, const int* origins, const float* window, void* out,
                                int is_u16, const void* target, unsigned long long* sse, int H, int W, int Co,
                                int Cp, int th, int tw, int ph, int pw, int ps, int T, float post_scale,
                                float post_shift, hipStream_t stream) {
    return launch_blend<false>({{pred, origins, window, H, W, Co, Cp, th, tw, ph, pw, ps, T, 1}, out, target, sse, is_u16,
                                post_scale, post_shift}, stream);
}

// Super-resolution blend: geometry in input pixels, predictions / window / output at scale s (see irm_hip.h).
extern "C" int irm_window_blend_scaled(const float* pred, const int* origins, const float* window, void* out,
                                       int is_u16, const void* target, unsigned long long* sse, int H, int W, int Co,
                                       int Cp, int th, int tw, int ph, int pw, int ps, int T, int scale,
                                       float post_scale, float post_shift, hipStream_t stream) {
    return launch_blend<true>({{pred, origins, window, H, W, Co, Cp, th, tw, ph, pw, ps, T, scale}, out, target, sse,
                               is_u16, post_scale, post_shift}, stream);
}
