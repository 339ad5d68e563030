// Per-frame PSNR / SSIM of restored frames against their targets, on the device (src/utils.py:134-156; the host
// restatement is utils.calculate_metrics).  For each of K frames [H][W][C] (u8 or u16, C = 1 or 3):
//   SSE  = exact integer sum of squared differences over all H*W*C values;
//   SSIM = skimage structural_similarity with its defaults (7x7 uniform window, K1 = .01, K2 = .03, sample
//          covariance 49/48), averaged over the interior S[3:-3, 3:-3] and, for C = 3, over the channels.
// The crop means no kept window reaches the border: only the (H-6) x (W-6) interior is evaluated, no padding mode.
//
// Numerics: the window moments (sum x, y, x^2, y^2, xy) are exact integers (int32 for u8; int64 for u16, where
// 49 * 65535^2 > 2^31), each variance is (49 * sum x^2 - (sum x)^2) / (49 * 48) with an exact integer numerator, and
// only the per-pixel ratio is evaluated in fp64 (one division per pixel: the 49 and 49 * 48 scales cancel in it).
//
// Reproducibility: each workgroup writes its fp64 SSIM sum and u64 SSE to its own workspace slot (a fixed order inside
// the workgroup), and a second launch sums a frame's slots in a fixed order.  No atomics: a frame's result does not
// depend on the run or on how many frames share the launch.
//
// Shared with metrics_basicsr.hip through irm_frame.h: the tile geometry (SsimTile), the workspace plan, the block
// sum and the slot reduction.  The staging and the two window passes stay written out in each file and no shared
// skeleton was built for them: this one issues all loads of a thread before the first wait and keeps exact integer
// moments, the other converts while it stages and rounds every fp64 tap on its own, so a policy would carry the
// accumulator type, the taps, the load schedule and the squared-error arithmetic - the whole loop body.
#include "irm_frame.h"

#define MT_ROWS 16                     // output rows per tile
#define MT_OUT 192                     // output values (pixel x channel) per tile row: 64 RGB or 192 grey pixels

struct MetricsArgs {
    const void* pred;                  // [K][H][W][C]
    const void* target;                // [K][H][W][C]
    unsigned long long* sse_part;      // [K][ntiles]
    double* ssim_part;                 // [K][ntiles]
    int H, W, tiles_x, tiles_y;
    double k1, k2;                     // 49^2 c1, 49*48 c2 (c1 = (0.01 R)^2, c2 = (0.03 R)^2)
};

// One workgroup: MT_ROWS output rows x (MT_OUT / C) output pixels of one frame.  The tile plus its 3-pixel halo is
// staged in LDS (a thread issues all its loads before it waits for the first); per output row, each thread forms the
// 7-row vertical moments of one loaded column, then each thread sums 7 of those horizontally for one output value and
// evaluates its SSIM.
template <typename T, typename A, int C>
__global__ __launch_bounds__(256) void ssim_tile_kernel(MetricsArgs a) {
    using Tile = SsimTile<MT_ROWS, MT_OUT, 6, C>;
    constexpr int rw = Tile::rw;                            // loaded values per tile row
    constexpr int NLD = ((MT_ROWS + 6) * rw + 255) / 256;   // loads per thread
    __shared__ T sx[MT_ROWS + 6][rw], sy[MT_ROWS + 6][rw];
    __shared__ A vm[5][rw];
    __shared__ double dpart[4];
    __shared__ unsigned long long upart[4];
    const Tile tg(a.H, a.W, a.tiles_x, a.tiles_y, blockIdx.x);
    const int ox0 = tg.ox0, oy0 = tg.oy0, nrow = tg.nrow, ncol = tg.ncol, k = blockIdx.y;
    const long frame = (long)k * a.H * a.W * C;
    const T* P = reinterpret_cast<const T*>(a.pred) + frame;
    const T* Q = reinterpret_cast<const T*>(a.target) + frame;

    // unconditional loads (outside the region: the frame's first value, replaced by 0), so none waits for another
    T xr[NLD], yr[NLD];
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
        const int i = threadIdx.x + u * 256, ly = i / rw, lj = i - ly * rw;
        const bool in = ly < nrow && lj < ncol;
        const long g = in ? (long)(oy0 + ly) * a.W * C + ox0 * C + lj : 0;
        xr[u] = P[g];
        yr[u] = Q[g];
        if (!in) xr[u] = yr[u] = 0;
    }
    unsigned long long err = 0;
#pragma unroll
    for (int u = 0; u < NLD; ++u) {
        const int i = threadIdx.x + u * 256, ly = i / rw, lj = i - ly * rw;
        if (ly < MT_ROWS + 6) {
            const int gy = oy0 + ly, gj = ox0 * C + lj;
            if (tg.owns(gy, gj)) {                        // (owned values lie inside the loaded region)
                const long d = (long)xr[u] - (long)yr[u];
                err += (unsigned long long)(d * d);
            }
            sx[ly][lj] = xr[u];
            sy[ly][lj] = yr[u];
        }
    }
    __syncthreads();

    const int nout_rows = tg.nout_rows, nout = tg.nout;
    const int t = threadIdx.x;
    double acc = 0.0;
#pragma unroll 1
    for (int r = 0; r < nout_rows; ++r) {
        if (t < ncol) {
            A s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
            for (int d = 0; d < 7; ++d) {
                const A xv = sx[r + d][t], yv = sy[r + d][t];
                s0 += xv;
                s1 += yv;
                s2 += xv * xv;
                s3 += yv * yv;
                s4 += xv * yv;
            }
            vm[0][t] = s0;
            vm[1][t] = s1;
            vm[2][t] = s2;
            vm[3][t] = s3;
            vm[4][t] = s4;
        }
        __syncthreads();
        if (t < nout) {                          // t = pixel * C + channel; window values t, t + C, ..., t + 6C
            A sxs = 0, sys = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
            for (int d = 0; d < 7; ++d) {
                const int j = t + d * C;
                sxs += vm[0][j];
                sys += vm[1][j];
                sxx += vm[2][j];
                syy += vm[3][j];
                sxy += vm[4][j];
            }
            // S = ((2 ux uy + c1)(2 vxy + c2)) / ((ux^2 + uy^2 + c1)(vx + vy + c2)), ux = sx / 49,
            // vx = (49 sxx - sx^2) / (49 * 48): scaling the first factors by 49^2 and the second by 49 * 48 leaves exact
            // integers plus k1 = 49^2 c1, k2 = 49 * 48 c2 (u8: every term below 2^31).  One rounded add per factor, no
            // contraction: identical frames give exactly 1.
            const A nx = 49 * sxx - sxs * sxs, ny = 49 * syy - sys * sys, nxy = 49 * sxy - sxs * sys;
            const double num = __dmul_rn(__dadd_rn((double)(2 * sxs * sys), a.k1), __dadd_rn((double)(2 * nxy), a.k2));
            const double den = __dmul_rn(__dadd_rn((double)(sxs * sxs + sys * sys), a.k1), __dadd_rn((double)(nx + ny), a.k2));
            acc += num / den;
        }
        __syncthreads();
    }

    const unsigned long long e = irm_block_reduce256<FrSum>(err, upart);
    const double s = irm_block_reduce256<FrSum>(acc, dpart);
    if (threadIdx.x == 0) {
        const long slot = (long)k * a.tiles_x * a.tiles_y + blockIdx.x;
        a.sse_part[slot] = e;
        a.ssim_part[slot] = s;
    }
}

extern "C" int irm_frame_metrics(const void* pred, const void* target, int is_u16, int K, int H, int W, int C,
                                 double data_range, unsigned long long* sse, double* ssim, void* ws, long ws_words,
                                 hipStream_t stream) {
    if (!pred || !target || !sse || !ssim || !ws) return IRM_EINVAL;
    if (!irm_frames_ok(is_u16, K, H, W, C) || H < 7 || W < 7 || !(data_range > 0.0)) return IRM_EINVAL;
    SsimPlan p;
    if (!irm_ssim_plan(p, H - 6, W - 6, MT_ROWS, MT_OUT / C, K, ws, ws_words)) return IRM_EINVAL;
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    MetricsArgs a{pred, target, p.sse_part, p.ssim_part, H, W, p.tiles_x, p.tiles_y, 2401.0 * c1, 2352.0 * c2};
    const dim3 grid((unsigned)p.ntiles, K);
    irm_dispatch_frames(is_u16, C, [&](auto kind) {
        using T = typename decltype(kind)::type;
        using A = std::conditional_t<sizeof(T) == 1, int, long long>;       // the exact window moments: see the head
        hipLaunchKernelGGL((ssim_tile_kernel<T, A, decltype(kind)::C>), grid, dim3(256), 0, stream, a);
    });
    if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
    const double count = (double)C * (H - 6) * (W - 6);   // interior values of one frame
    hipLaunchKernelGGL(ssim_reduce_kernel<false>, dim3(K), dim3(256), 0, stream, p.sse_part, p.ssim_part, (int)p.ntiles,
                       count, sse, ssim);
    return irm_launch_status();
}
