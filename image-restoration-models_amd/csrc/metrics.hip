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
#include "irm_common.h"

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

// Sum over a workgroup of 256 threads in a fixed order: butterfly in each wave, then the four waves in order.
template <typename V>
__device__ __forceinline__ V block_sum256(V v, V* part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// One workgroup: MT_ROWS output rows x (MT_OUT / C) output pixels of one frame.  The tile plus its 3-pixel halo is
// staged in LDS (a thread issues all its loads before it waits for the first); per output row, each thread forms the
// 7-row vertical moments of one loaded column, then each thread sums 7 of those horizontally for one output value and
// evaluates its SSIM.
template <typename T, typename A, int C>
__global__ __launch_bounds__(256) void ssim_tile_kernel(MetricsArgs a) {
    constexpr int twp = MT_OUT / C, rw = (twp + 6) * C;     // output pixels, loaded values per tile row
    constexpr int NLD = ((MT_ROWS + 6) * rw + 255) / 256;   // loads per thread
    __shared__ T sx[MT_ROWS + 6][rw], sy[MT_ROWS + 6][rw];
    __shared__ A vm[5][rw];
    __shared__ double dpart[4];
    __shared__ unsigned long long upart[4];
    const int Ho = a.H - 6, Wo = a.W - 6;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x, k = blockIdx.y;
    const int ox0 = tx * twp, oy0 = ty * MT_ROWS;
    const long frame = (long)k * a.H * a.W * C;
    const T* P = reinterpret_cast<const T*>(a.pred) + frame;
    const T* Q = reinterpret_cast<const T*>(a.target) + frame;

    // loaded region: image rows [oy0, oy0 + nrow), row values [ox0*C, ox0*C + ncol)
    const int nrow = min(MT_ROWS + 6, a.H - oy0);
    const int ncol = min(rw, (a.W - ox0) * C);
    // SSE ownership: the tile's output centres, widened to the image border for the first / last tile of a row or
    // column, so that the tiles of a frame partition it exactly
    const int cy0 = ty == 0 ? 0 : oy0 + 3;
    const int cy1 = ty == a.tiles_y - 1 ? a.H : oy0 + MT_ROWS + 3;
    const int cx0 = (tx == 0 ? 0 : ox0 + 3) * C;
    const int cx1 = (tx == a.tiles_x - 1 ? a.W : ox0 + twp + 3) * C;
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
            if (gy >= cy0 && gy < cy1 && gj >= cx0 && gj < cx1) {   // (owned values lie inside the loaded region)
                const long d = (long)xr[u] - (long)yr[u];
                err += (unsigned long long)(d * d);
            }
            sx[ly][lj] = xr[u];
            sy[ly][lj] = yr[u];
        }
    }
    __syncthreads();

    const int nout_rows = min(MT_ROWS, Ho - oy0);
    const int nout = min(twp, Wo - ox0) * C;     // valid output values per row; their windows lie inside ncol
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

    const unsigned long long e = block_sum256(err, upart);
    const double s = block_sum256(acc, dpart);
    if (threadIdx.x == 0) {
        const long slot = (long)k * a.tiles_x * a.tiles_y + blockIdx.x;
        a.sse_part[slot] = e;
        a.ssim_part[slot] = s;
    }
}

// One workgroup per frame: its tile slots summed in a fixed order.
__global__ __launch_bounds__(256) void metrics_reduce_kernel(const unsigned long long* sse_part, const double* ssim_part,
                                                             int ntiles, double count, unsigned long long* sse,
                                                             double* ssim) {
    __shared__ double dpart[4];
    __shared__ unsigned long long upart[4];
    const long base = (long)blockIdx.x * ntiles;
    unsigned long long e = 0;
    double s = 0.0;
    for (int j = threadIdx.x; j < ntiles; j += 256) {
        e += sse_part[base + j];
        s += ssim_part[base + j];
    }
    e = block_sum256(e, upart);
    s = block_sum256(s, dpart);
    if (threadIdx.x == 0) {
        sse[blockIdx.x] = e;
        ssim[blockIdx.x] = s / count;
    }
}

extern "C" int irm_frame_metrics(const void* pred, const void* target, int is_u16, int K, int H, int W, int C,
                                 double data_range, unsigned long long* sse, double* ssim, void* ws, long ws_words,
                                 hipStream_t stream) {
    if (!pred || !target || !sse || !ssim || !ws) return IRM_EINVAL;
    if ((is_u16 != 0 && is_u16 != 1) || K <= 0 || K > 65535 || H < 7 || W < 7 || (C != 1 && C != 3)) return IRM_EINVAL;
    if (!(data_range > 0.0) || (long)H * W * C > 0x7fffffffL) return IRM_EINVAL;
    const int tiles_x = (W - 6 + MT_OUT / C - 1) / (MT_OUT / C), tiles_y = (H - 6 + MT_ROWS - 1) / MT_ROWS;
    const long ntiles = (long)tiles_x * tiles_y;
    if (ws_words < 2 * K * ntiles) return IRM_EINVAL;
    unsigned long long* sse_part = reinterpret_cast<unsigned long long*>(ws);
    double* ssim_part = reinterpret_cast<double*>(sse_part + K * ntiles);
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    MetricsArgs a{pred, target, sse_part, ssim_part, H, W, tiles_x, tiles_y, 2401.0 * c1, 2352.0 * c2};
    const dim3 grid((unsigned)ntiles, K);
    if (is_u16 && C == 3) hipLaunchKernelGGL((ssim_tile_kernel<unsigned short, long long, 3>), grid, dim3(256), 0, stream, a);
    else if (is_u16) hipLaunchKernelGGL((ssim_tile_kernel<unsigned short, long long, 1>), grid, dim3(256), 0, stream, a);
    else if (C == 3) hipLaunchKernelGGL((ssim_tile_kernel<unsigned char, int, 3>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((ssim_tile_kernel<unsigned char, int, 1>), grid, dim3(256), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
    const double count = (double)C * (H - 6) * (W - 6);   // interior values of one frame
    hipLaunchKernelGGL(metrics_reduce_kernel, dim3(K), dim3(256), 0, stream, sse_part, ssim_part, (int)ntiles, count,
                       sse, ssim);
    return irm_launch_status();
}
