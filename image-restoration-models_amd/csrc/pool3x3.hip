// The two 3x3 poolings of the Inception-ResNet-v2 encoder (DeblurGANv2 FPN-Inception), planar NCHW with batch-strided
// tensors, so that a pooled branch lands in its channel slice of a concat buffer:
//   mode 0  MaxPool2d(3, stride 2), no padding: OH = (H - 3) / 2 + 1; the maximum starts at -inf, not at 0 (the
//           inputs may be all negative); a last row / column that no window reaches is ignored
//   mode 1  AvgPool2d(3, stride 1, padding 1, count_include_pad=False): the sum of the taps inside the image divided
//           by their number - 4 at the corners, 6 at the edges, 9 inside (fewer on images below 3 pixels)
// One thread per output pixel; a memory stream, no LDS.
#include "irm_common.h"
#include <math.h>

__global__ __launch_bounds__(256) void pool3x3_kernel(const float* __restrict__ X, long x_bs, float* __restrict__ Y,
                                                      long y_bs, int H, int W, int OH, int OW, int mode) {
    const long n = (long)blockIdx.x * 256 + threadIdx.x;
    if (n >= (long)OH * OW) return;
    const int oy = (int)(n / OW), ox = (int)(n % OW);
    const float* x = X + (long)blockIdx.z * x_bs + (long)blockIdx.y * H * W;
    float* y = Y + (long)blockIdx.z * y_bs + (long)blockIdx.y * OH * OW;
    const int y0 = mode ? oy - 1 : 2 * oy, x0 = mode ? ox - 1 : 2 * ox;
    float m = -INFINITY, s = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int gy = y0 + dy, gx = x0 + dx;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const float v = x[(long)gy * W + gx];
                m = fmaxf(m, v);
                s += v;
                ++cnt;
            }
        }
    }
    y[n] = mode ? s / (float)cnt : m;
}

extern "C" int irm_pool3x3_f32(const float* x, long x_bs, float* y, long y_bs, int B, int C, int H, int W, int mode,
                               hipStream_t stream) {
    if (!x || !y || B <= 0 || C <= 0 || H <= 0 || W <= 0 || mode < 0 || mode > 1) return IRM_EINVAL;
    if (B > 65535 || C > 65535) return IRM_EINVAL;
    if (mode == 0 && (H < 3 || W < 3)) return IRM_EINVAL;                     // no window fits
    const int OH = mode ? H : (H - 3) / 2 + 1, OW = mode ? W : (W - 3) / 2 + 1;
    const long blocks = ((long)OH * OW + 255) / 256;
    if (blocks > 0x7fffffffL) return IRM_EINVAL;
    dim3 grid((unsigned)blocks, C, B);
    hipLaunchKernelGGL(pool3x3_kernel, grid, dim3(256), 0, stream, x, x_bs, y, y_bs, H, W, OH, OW, mode);
    return irm_launch_status();
}
