// Float32 frames on the device side of the tiled-patch loop (src/utils.py:353-454): the per-frame min / max that
// utils.normalize (159-171) and the final clip (450-454) need, tile extraction from a float32 HWC frame and the window
// blend into a float32 HWC frame.  Indexing, padding, noise and accumulation are the tile walk of irm_frame.h that
// tiler.hip's integer kernels use too; here are the float32 sample rule and sink.  The value range comes from a
// 3-float device buffer {lo, hi, mul}, so nothing here waits for the host.
#include "irm_frame.h"

// ---------------------------------------------------------------------------
// min / max of n floats: no atomics, per-workgroup partials in ws ([nwg][2]), one finishing workgroup.  Both are
// order independent, so the result is bitwise the sequential one for finite input.
#define MINMAX_MAX_WG 1024
#define MINMAX_PER_WG 8192          // elements a workgroup should at least have before another one is started

__device__ __forceinline__ void minmax_wg(float mn, float mx, float* lo, float* hi) {
    __shared__ float part[2][4];
    mn = irm_block_reduce256<FrMin>(mn, part[0]);
    mx = irm_block_reduce256<FrMax>(mx, part[1]);
    if (threadIdx.x == 0) {
        *lo = mn;
        *hi = mx;
    }
}

// head: elements before the first 16-byte boundary (0..3, at most n); nv: float4 units after them; the rest is the tail
__global__ __launch_bounds__(256) void minmax_partial_kernel(const float* __restrict__ img, long n, int head, long nv,
                                                             float* __restrict__ ws) {
    float mn = INFINITY, mx = -INFINITY;
    const float4* p = reinterpret_cast<const float4*>(img + head);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
        const float4 v = p[i];
        mn = fminf(fminf(mn, v.x), fminf(v.y, fminf(v.z, v.w)));
        mx = fmaxf(fmaxf(mx, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
    if (blockIdx.x == 0 && threadIdx.x < 8) {               // scalar head and tail: at most 3 elements each
        const long t = threadIdx.x;
        const long i = t < head ? t : (long)head + 4 * nv + (t - head);
        if (i < n) { mn = fminf(mn, img[i]); mx = fmaxf(mx, img[i]); }
    }
    minmax_wg(mn, mx, ws + 2 * blockIdx.x, ws + 2 * blockIdx.x + 1);
}

__global__ __launch_bounds__(256) void minmax_finish_kernel(const float* __restrict__ ws, int nwg, float* __restrict__ range) {
    float mn = INFINITY, mx = -INFINITY;
    for (int i = threadIdx.x; i < nwg; i += 256) {
        mn = fminf(mn, ws[2 * i]);
        mx = fmaxf(mx, ws[2 * i + 1]);
    }
    __shared__ float res[2];
    minmax_wg(mn, mx, &res[0], &res[1]);
    if (threadIdx.x == 0) {
        range[0] = res[0];
        range[1] = res[1];
        range[2] = res[1];
    }
}

extern "C" int irm_frame_minmax_f32(const float* img, long n, float* range, float* ws, long ws_floats,
                                    hipStream_t stream) {
    if (!img || !range || !ws || n <= 0 || ws_floats < 2) return IRM_EINVAL;
    if (reinterpret_cast<uintptr_t>(img) & 3) return IRM_EINVAL;
    long head = ((16 - (long)(reinterpret_cast<uintptr_t>(img) & 15)) & 15) >> 2;
    if (head > n) head = n;
    const long nv = (n - head) >> 2;
    long nwg = (n + MINMAX_PER_WG - 1) / MINMAX_PER_WG;
    if (nwg > MINMAX_MAX_WG) nwg = MINMAX_MAX_WG;
    if (nwg > ws_floats / 2) nwg = ws_floats / 2;
    hipLaunchKernelGGL(minmax_partial_kernel, dim3((unsigned)nwg), dim3(256), 0, stream, img, n, (int)head, nv, ws);
    const int rc = irm_launch_status();
    if (rc != IRM_OK) return rc;
    hipLaunchKernelGGL(minmax_finish_kernel, dim3(1), dim3(256), 0, stream, ws, (int)nwg, range);
    return irm_launch_status();
}

// ---------------------------------------------------------------------------
struct ExtractF32Args {
    const float* img;      // [H][W][C]
    const float* range;    // {lo, hi, mul} on the device: divide by hi where hi > 1 (utils.normalize)
    TileCut g;
};

__global__ __launch_bounds__(256) void tile_extract_f32_kernel(ExtractF32Args a) {
    irm_extract_element(a.g, [&](long src) {
        const float raw = a.img[src];
        const float hi = a.range[1];
        return hi > 1.0f ? __fdiv_rn(raw, hi) : raw;        // utils.py:159-171
    });
}

extern "C" int irm_tile_extract_f32(const float* img, const float* range, const int* origins, const double* noise,
                                    float* tiles, int H, int W, int C, int th, int tw, int ph, int pw, int T,
                                    int pad_zero, hipStream_t stream) {
    const ExtractF32Args a{img, range, {origins, noise, tiles, H, W, C, th, tw, ph, pw, T, pad_zero}};
    if (!range || !irm_tile_cut_ok(img, a.g)) return IRM_EINVAL;
    hipLaunchKernelGGL(tile_extract_f32_kernel, dim3(irm_tile_cut_blocks(a.g)), dim3(256), 0, stream, a);
    return irm_launch_status();
}

// ---------------------------------------------------------------------------
struct BlendF32Args {
    TileBlend g;
    float* out;            // [H][W][Co]
    const float* range;    // {lo, hi, mul}: out = clip(v * mul, lo, hi)
};

__global__ __launch_bounds__(256) void blend_f32_kernel(BlendF32Args a) {
    const long total = (long)a.g.H * a.g.W * a.g.Co;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const float v = irm_blend_element<true>(a.g, idx, [](float p) { return p; });
    const float lo = a.range[0], hi = a.range[1], mul = a.range[2];
    a.out[idx] = fminf(fmaxf(__fmul_rn(v, mul), lo), hi);    // np.clip(acc * hi, lo, hi): utils.py:453-454
}

extern "C" int irm_window_blend_f32(const float* pred, const int* origins, const float* window, float* out,
                                    const float* range, int H, int W, int Co, int Cp, int th, int tw, int ph, int pw,
                                    int ps, int T, int scale, hipStream_t stream) {
    BlendF32Args a{{pred, origins, window, H, W, Co, Cp, th, tw, ph, pw, ps, T, scale}, out, range};
    if (!range || !irm_tile_blend_plan(a.g, out, true)) return IRM_EINVAL;
    const long total = (long)a.g.H * a.g.W * Co;
    hipLaunchKernelGGL(blend_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a);
    return irm_launch_status();
}
