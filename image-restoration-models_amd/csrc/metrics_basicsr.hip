// Per-frame squared-error sum and SSIM of the super-resolution protocol, on the device: what basicsr's calculate_psnr /
// calculate_ssim compute (crop_border, test_y_channel; the host restatement is utils.calculate_metrics_basicsr).  For
// each of K frame pairs [H][W][C] (u8 or u16, C = 1 or 3), after cropping `crop` pixels from every side:
//   values  test_y off: the raw integers, all C channels;
//           test_y on : one channel.  C = 3: the BT.601 luma with the reference's rounding steps - v / R in fp32, the
//                       three-term dot (ascending channel order, no contraction) plus 16 in fp64, / 255 in fp64, rounded
//                       to fp32, x R in fp32.  C = 1: the fp32 round trip v / R x R.  (R = 255 or 65535.)
//   SSE     test_y off: exact integer sum over all values; test_y on: fp64 sum of the fp64 squares of the differences;
//   SSIM    per channel over the valid region (Hc - 10) x (Wc - 10): separable 11-tap Gaussian exp(-(i-5)^2 / 4.5),
//           normalised, moments in fp64; c1 = (0.01 R)^2, c2 = (0.03 R)^2 (6.5025 / 58.5225 for u8); channel mean.
//
// Reproducibility as in metrics.hip: each workgroup writes its partials to its own workspace slot (a fixed order inside
// the workgroup), a second launch sums a frame's slots in a fixed order.  No atomics; a frame's result does not depend
// on K or on the run.  The final SSIM ratio uses explicitly rounded operations, so identical frames give exactly 1.
#include "irm_frame.h"

#define BT_ROWS 16                     // output rows per tile
#define BT_OUT 192                     // output values (pixel x kept channel) per tile row
#define BT_HALO 10                     // 11-tap window

struct BasicsrArgs {
    const void* pred;                  // [K][H][W][C]
    const void* target;
    unsigned long long* sse_part;      // [K][ntiles]: u64, or the bit pattern of an fp64 with test_y on
    double* ssim_part;                 // [K][ntiles]
    int H, W, crop, tiles_x, tiles_y, bgr;
    float range;
    double c1, c2;
    double g[11];                      // the normalised window
};

// s + g v with the product and the sum each rounded (no FMA): the window sums are then the numbers the host restatement's
// numpy expressions give, tap by tap in ascending order
__device__ __forceinline__ double bt_acc(double s, double g, double v) { return __dadd_rn(s, __dmul_rn(g, v)); }

// the value the metric sees, as an fp32 (raw integers up to 65535 are exact in it)
template <typename T, int C, bool Y>
__device__ __forceinline__ float bt_value(const T* p, int j, float range, int bgr) {
    if (!Y) return (float)p[j];
    if (C == 1) return (float)p[j] / range * range;
    const double c0 = (double)((float)p[3 * j] / range), c1 = (double)((float)p[3 * j + 1] / range),
                 c2 = (double)((float)p[3 * j + 2] / range);
    const double k0 = bgr ? 24.966 : 65.481, k2 = bgr ? 65.481 : 24.966;
    const double dot = __dadd_rn(__dadd_rn(__dmul_rn(c0, k0), __dmul_rn(c1, 128.553)), __dmul_rn(c2, k2));
    return (float)(__dadd_rn(dot, 16.0) / 255.0) * range;
}

// One workgroup: BT_ROWS output rows x (BT_OUT / CE) output pixels of one cropped frame, CE = kept channels.  The
// tile's values plus the 10-pixel halo are staged in LDS as fp32; per output row each thread forms the 11-row vertical
// moments of one staged column, then each thread sums 11 of those horizontally for one output value.
template <typename T, int C, bool Y>
__global__ __launch_bounds__(256) void basicsr_tile_kernel(BasicsrArgs a) {
    constexpr int CE = Y ? 1 : C;
    using Tile = SsimTile<BT_ROWS, BT_OUT, BT_HALO, CE>;
    constexpr int rw = Tile::rw;
    __shared__ float sx[BT_ROWS + BT_HALO][rw], sy[BT_ROWS + BT_HALO][rw];
    __shared__ double vm[5][rw];
    __shared__ double dpart[4], epart[4];
    __shared__ unsigned long long upart[4];
    const Tile tg(a.H - 2 * a.crop, a.W - 2 * a.crop, a.tiles_x, a.tiles_y, blockIdx.x);
    const int ox0 = tg.ox0, oy0 = tg.oy0, nrow = tg.nrow, ncol = tg.ncol, k = blockIdx.y;
    const long frame = (long)k * a.H * a.W * C + ((long)a.crop * a.W + a.crop) * C;
    const T* P = reinterpret_cast<const T*>(a.pred) + frame;
    const T* Q = reinterpret_cast<const T*>(a.target) + frame;

    unsigned long long err = 0;
    double errd = 0.0;
    for (int i = threadIdx.x; i < nrow * ncol; i += 256) {
        const int ly = i / ncol, lj = i - ly * ncol;
        const long rowoff = (long)(oy0 + ly) * a.W * C + (long)ox0 * C;      // (CE values of a pixel <-> its C inputs)
        const float xv = bt_value<T, C, Y>(P + rowoff, lj, a.range, a.bgr);
        const float yv = bt_value<T, C, Y>(Q + rowoff, lj, a.range, a.bgr);
        sx[ly][lj] = xv;
        sy[ly][lj] = yv;
        const int gy = oy0 + ly, gj = ox0 * CE + lj;
        if (tg.owns(gy, gj)) {
            if (Y) {
                const double d = (double)xv - (double)yv;
                errd = __dadd_rn(errd, __dmul_rn(d, d));
            } else {
                const long d = (long)(xv - yv);                               // exact: both are integers below 2^16
                err += (unsigned long long)(d * d);
            }
        }
    }
    __syncthreads();

    const int nout_rows = tg.nout_rows, nout = tg.nout;
    const int t = threadIdx.x;
    double acc = 0.0;
#pragma unroll 1
    for (int r = 0; r < nout_rows; ++r) {
        if (t < ncol) {
            double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
            for (int d = 0; d < 11; ++d) {
                const double xv = sx[r + d][t], yv = sy[r + d][t], g = a.g[d];
                s0 = bt_acc(s0, g, xv);
                s1 = bt_acc(s1, g, yv);
                s2 = bt_acc(s2, g, __dmul_rn(xv, xv));
                s3 = bt_acc(s3, g, __dmul_rn(yv, yv));
                s4 = bt_acc(s4, g, __dmul_rn(xv, yv));
            }
            vm[0][t] = s0;
            vm[1][t] = s1;
            vm[2][t] = s2;
            vm[3][t] = s3;
            vm[4][t] = s4;
        }
        __syncthreads();
        if (t < nout) {                          // t = pixel * CE + channel; window values t, t + CE, ..., t + 10 CE
            double m1 = 0, m2 = 0, e11 = 0, e22 = 0, e12 = 0;
#pragma unroll
            for (int d = 0; d < 11; ++d) {
                const int j = t + d * CE;
                const double g = a.g[d];
                m1 = bt_acc(m1, g, vm[0][j]);
                m2 = bt_acc(m2, g, vm[1][j]);
                e11 = bt_acc(e11, g, vm[2][j]);
                e22 = bt_acc(e22, g, vm[3][j]);
                e12 = bt_acc(e12, g, vm[4][j]);
            }
            // every step rounded on its own (no contraction): with identical frames m1 == m2 and the three second
            // moments coincide bitwise, numerator and denominator are the same number and the ratio is exactly 1
            const double m11 = __dmul_rn(m1, m1), m22 = __dmul_rn(m2, m2), m12 = __dmul_rn(m1, m2);
            const double v1 = __dsub_rn(e11, m11), v2 = __dsub_rn(e22, m22), v12 = __dsub_rn(e12, m12);
            const double num = __dmul_rn(__dadd_rn(__dmul_rn(2.0, m12), a.c1), __dadd_rn(__dmul_rn(2.0, v12), a.c2));
            const double den = __dmul_rn(__dadd_rn(__dadd_rn(m11, m22), a.c1), __dadd_rn(__dadd_rn(v1, v2), a.c2));
            acc += num / den;
        }
        __syncthreads();
    }

    const double s = irm_block_reduce256<FrSum>(acc, dpart);
    const long slot = (long)k * a.tiles_x * a.tiles_y + blockIdx.x;
    if (Y) {
        const double e = irm_block_reduce256<FrSum>(errd, epart);
        if (threadIdx.x == 0) a.sse_part[slot] = (unsigned long long)__double_as_longlong(e);
    } else {
        const unsigned long long e = irm_block_reduce256<FrSum>(err, upart);
        if (threadIdx.x == 0) a.sse_part[slot] = e;
    }
    if (threadIdx.x == 0) a.ssim_part[slot] = s;
}

template <typename T, int C>
static void launch_basicsr(const BasicsrArgs& a, int test_y, dim3 grid, hipStream_t stream) {
    if (test_y) hipLaunchKernelGGL((basicsr_tile_kernel<T, C, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((basicsr_tile_kernel<T, C, false>), grid, dim3(256), 0, stream, a);
}

extern "C" int irm_frame_metrics_basicsr(const void* pred, const void* target, int is_u16, int K, int H, int W, int C,
                                         int crop_border, int test_y_channel, int bgr, void* sse, double* ssim, void* ws,
                                         long ws_words, hipStream_t stream) {
    if (!pred || !target || !sse || !ssim || !ws) return IRM_EINVAL;
    if (!irm_frames_ok(is_u16, K, H, W, C) || !irm_is_flag(test_y_channel) || !irm_is_flag(bgr)) return IRM_EINVAL;
    if (crop_border < 0 || crop_border > 16384) return IRM_EINVAL;
    const int Hc = H - 2 * crop_border, Wc = W - 2 * crop_border;
    if (Hc < 11 || Wc < 11) return IRM_EINVAL;
    const int CE = test_y_channel ? 1 : C;
    SsimPlan p;
    if (!irm_ssim_plan(p, Hc - BT_HALO, Wc - BT_HALO, BT_ROWS, BT_OUT / CE, K, ws, ws_words)) return IRM_EINVAL;
    const double R = is_u16 ? 65535.0 : 255.0;
    BasicsrArgs a{pred, target, p.sse_part, p.ssim_part, H, W, crop_border, p.tiles_x, p.tiles_y, bgr, (float)R,
                  (0.01 * R) * (0.01 * R), (0.03 * R) * (0.03 * R), {}};
    double gs = 0.0;
    for (int i = 0; i < 11; ++i) {
        a.g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        gs += a.g[i];
    }
    for (int i = 0; i < 11; ++i) a.g[i] /= gs;
    const dim3 grid((unsigned)p.ntiles, K);
    irm_dispatch_frames(is_u16, C, [&](auto kind) {
        launch_basicsr<typename decltype(kind)::type, decltype(kind)::C>(a, test_y_channel, grid, stream);
    });
    if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
    const double count = (double)CE * (Hc - BT_HALO) * (Wc - BT_HALO);
    unsigned long long* sse_out = reinterpret_cast<unsigned long long*>(sse);
    if (test_y_channel)
        hipLaunchKernelGGL(ssim_reduce_kernel<true>, dim3(K), dim3(256), 0, stream, p.sse_part, p.ssim_part, (int)p.ntiles,
                           count, sse_out, ssim);
    else
        hipLaunchKernelGGL(ssim_reduce_kernel<false>, dim3(K), dim3(256), 0, stream, p.sse_part, p.ssim_part, (int)p.ntiles,
                           count, sse_out, ssim);
    return irm_launch_status();
}
