// Float32 frames on the device side of the tiled-patch loop (src/utils.py:353-454): the per-frame min / max that
// utils.normalize (159-171) and the final clip (450-454) need, tile extraction from a float32 HWC frame and the window
// blend into a float32 HWC frame.  Indexing, padding, noise and accumulation restate tiler.hip's integer kernels with
// the same float32 operation order; the value range comes from a 3-float device buffer {lo, hi, mul}, so nothing
// here waits for the host.
#include "irm_common.h"

// ---------------------------------------------------------------------------
// min / max of n floats: no atomics, per-workgroup partials in ws ([nwg][2]), one finishing workgroup.  Both are
// order independent, so the result is bitwise the sequential one for finite input.
#define MINMAX_MAX_WG 1024
#define MINMAX_PER_WG 8192          // elements a workgroup should at least have before another one is started

__device__ __forceinline__ void minmax_wg(float mn, float mx, float* lo, float* hi) {
    __shared__ float part[2][4];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = mn; part[1][threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        *lo = fminf(fminf(part[0][0], part[0][1]), fminf(part[0][2], part[0][3]));
        *hi = fmaxf(fmaxf(part[1][0], part[1][1]), fmaxf(part[1][2], part[1][3]));
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
    const int* origins;    // [T][2] (y0, x0)
    const double* noise;   // [th][tw][C] float64 field (same for every tile) or null
    float* tiles;          // [T][C][ph][pw]
    int H, W, C, th, tw, ph, pw, T;
    int pad_zero;          // 0: reflect pad (utils.pad), 1: zero pad
};

__global__ __launch_bounds__(256) void tile_extract_f32_kernel(ExtractF32Args a) {
    const long total = (long)a.T * a.C * a.ph * a.pw;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int px = (int)(idx % a.pw);
    long t = idx / a.pw;
    const int py = (int)(t % a.ph); t /= a.ph;
    const int c = (int)(t % a.C);
    const int tile = (int)(t / a.C);
    if (a.pad_zero && (py >= a.th || px >= a.tw)) {
        a.tiles[idx] = 0.0f;
        return;
    }
    // reflect (no edge repeat) for the padded rows/cols: utils.py:174-181
    const int sy = py < a.th ? py : 2 * a.th - 2 - py;
    const int sx = px < a.tw ? px : 2 * a.tw - 2 - px;
    const int gy = a.origins[tile * 2] + sy, gx = a.origins[tile * 2 + 1] + sx;
    const float raw = a.img[((long)gy * a.W + gx) * a.C + c];
    const float hi = a.range[1];
    float v = hi > 1.0f ? __fdiv_rn(raw, hi) : raw;         // utils.py:159-171
    if (a.noise) {                                          // utils.py:29-36
        const double d = (double)v + a.noise[((long)sy * a.tw + sx) * a.C + c];
        v = (float)fmin(fmax(d, 0.0), 1.0);
    }
    a.tiles[idx] = v;
}

extern "C" int irm_tile_extract_f32(const float* img, const float* range, const int* origins, const double* noise,
                                    float* tiles, int H, int W, int C, int th, int tw, int ph, int pw, int T,
                                    int pad_zero, hipStream_t stream) {
    if (!img || !range || !origins || !tiles || H <= 0 || W <= 0 || C <= 0 || T <= 0) return IRM_EINVAL;
    if (th <= 0 || tw <= 0 || ph < th || pw < tw || th > H || tw > W) return IRM_EINVAL;
    if (!pad_zero && (ph - th >= th || pw - tw >= tw)) return IRM_EINVAL;    // reflect needs pad < extent
    ExtractF32Args a{img, range, origins, noise, tiles, H, W, C, th, tw, ph, pw, T, pad_zero};
    const long total = (long)T * C * ph * pw;
    hipLaunchKernelGGL(tile_extract_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a);
    return irm_launch_status();
}

// ---------------------------------------------------------------------------
struct BlendF32Args {
    const float* pred;     // [T][Cp][ph][pw], only [:Co][:th][:tw] is used
    const int* origins;    // [T][2], in the reference's loop order, in input pixels
    const float* window;   // [ps][ps]
    float* out;            // [H][W][Co]
    const float* range;    // {lo, hi, mul}: out = clip(v * mul, lo, hi)
    int H, W, Co, Cp, th, tw, ph, pw, ps, T;     // at output scale
    int scale;             // the origins are multiplied by it
};

__global__ __launch_bounds__(256) void blend_f32_kernel(BlendF32Args a) {
    const long total = (long)a.H * a.W * a.Co;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % a.Co);
    const long t = idx / a.Co;
    const int x = (int)(t % a.W), y = (int)(t / a.W);
    float acc = 0.0f, wsum = 0.0f;
    for (int i = 0; i < a.T; ++i) {                // same order as the h_idx / w_idx loops
        const int ly = y - a.origins[2 * i] * a.scale, lx = x - a.origins[2 * i + 1] * a.scale;
        if (ly < 0 || ly >= a.th || lx < 0 || lx >= a.tw) continue;
        const float p = a.pred[(((long)i * a.Cp + c) * a.ph + ly) * a.pw + lx];
        const float w = a.window[ly * a.ps + lx];
        acc = __fadd_rn(acc, __fmul_rn(p, w));          // utils.py:433
        wsum = __fadd_rn(wsum, w);                       // utils.py:434
    }
    const float v = __fdiv_rn(acc, fmaxf(wsum, 1e-8f));  // utils.py:440
    const float lo = a.range[0], hi = a.range[1], mul = a.range[2];
    a.out[idx] = fminf(fmaxf(__fmul_rn(v, mul), lo), hi);    // np.clip(acc * hi, lo, hi): utils.py:453-454
}

extern "C" int irm_window_blend_f32(const float* pred, const int* origins, const float* window, float* out,
                                    const float* range, int H, int W, int Co, int Cp, int th, int tw, int ph, int pw,
                                    int ps, int T, int scale, hipStream_t stream) {
    if (!pred || !origins || !window || !out || !range || H <= 0 || W <= 0 || Co <= 0 || Cp < Co || T <= 0)
        return IRM_EINVAL;
    if (th <= 0 || tw <= 0 || ph < th || pw < tw || th > ps || tw > ps || scale < 1 || scale > 8) return IRM_EINVAL;
    // int indices inside the kernel: output rows / columns and the window index (s ps)^2 stay below 2^31
    if ((long)H * scale > (1L << 20) || (long)W * scale > (1L << 20) || (long)ps * scale * ps * scale >= (1L << 31))
        return IRM_EINVAL;
    const int s = scale;
    BlendF32Args a{pred, origins, window, out, range, s * H, s * W, Co, Cp, s * th, s * tw, s * ph, s * pw, s * ps, T, s};
    const long total = (long)a.H * a.W * Co;
    hipLaunchKernelGGL(blend_f32_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, a);
    return irm_launch_status();
}
