// The aligned scoring protocol of beam-splitter pairs (include/irm_hip_align.h; the float64 statement is
// irm_amd/align.py, the contract DESIGN.md section 24):
//   irm_align_prepare    one gain from exact integer sums, then the template / image planes (grey, 5-tap Gaussian) and
//                        the image gradients, float32;
//   irm_ecc_iterate      `iterations` x (accumulate, solve) of the forward additive ECC iteration for a homography: a
//                        workgroup per 16 x 64 target pixels leaves 66 fp64 sums in its workspace slot, one workgroup
//                        sums the slots, factorises the 8 x 8 Hessian and updates the map in device memory;
//   irm_aligned_metrics  the bicubic warp of the prediction at 1/32-pixel positions and squared error, mask count and
//                        masked Gaussian-window SSIM on the SsimTile skeleton of irm_frame.h.
// Everything per pixel is fp64 and the file is built with -ffp-contract=off: a product and the sum that takes it are
// rounded separately, in the order the statement writes them, so positions, masks and phases are the statement's bit for
// bit.  One-pass statistics: the zero-mean quantities follow from the 66 raw sums (the planes lie in [0, 1.1], the
// cancellation costs about one decimal digit of fp64).  No atomics, no barrier across workgroups, no waiting on memory:
// stream order is the only synchronisation, every sum has a fixed order.
#include "irm_frame.h"

#define AL_CHUNK 4096                  // samples per workgroup of the gain sums
#define AL_TW 64                       // target pixels per tile row of the accumulate kernel
#define AL_TH 16                       // tile rows: four per thread
#define AL_SUMS 66
#define AM_ROWS 16                     // output rows per tile of the metrics kernel
#define AM_OUT 96                      // output values per tile row: 32 pixels x 3 channels
#define AM_HALO 10                     // 11-tap window

// dcb|abcd|cba (the pre-filter and the gradients) and cba|abcd|dcb (the final warp); one reflection: |offset| <= n
__device__ __forceinline__ int al_reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
__device__ __forceinline__ int al_reflect(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - 1 - i : i); }

// the map as the kernels use it
struct AlMap { double m0, m1, m2, m3, m4, m5, m6, m7; };
__device__ __forceinline__ AlMap al_load_map(const double* m) { return {m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7]}; }

// source position of target pixel (x, y): multiply, add and divide as separate operations in this order
__device__ __forceinline__ void al_position(const AlMap& m, double x, double y, double& den, double& px, double& py) {
    den = (m.m6 * x + m.m7 * y) + 1.0;
    px = ((m.m0 * x + m.m1 * y) + m.m2) / den;
    py = ((m.m3 * x + m.m4 * y) + m.m5) / den;
}
// the position rounded to nearest (half to even) lies inside the frame; false for NaN
__device__ __forceinline__ bool al_inside(double px, double py, int H, int W) {
    const double rx = rint(px), ry = rint(py);
    return rx >= 0.0 && rx <= (double)(W - 1) && ry >= 0.0 && ry <= (double)(H - 1);
}

// ---------------------------------------------------------------------------
// irm_align_prepare
template <typename T>
__global__ __launch_bounds__(256) void align_gain_kernel(const T* z, const T* x, long n, double* part) {
    __shared__ double pa[4], pb[4];
    double sxz = 0.0, szz = 0.0;                   // sums of integers: exact below 2^53, whatever the order
    const long base = (long)blockIdx.x * AL_CHUNK;
    for (int k = 0; k < AL_CHUNK / 256; ++k) {
        const long i = base + k * 256 + threadIdx.x;
        if (i < n) {
            const double a = (double)z[i], b = (double)x[i];
            sxz += a * b;
            szz += a * a;
        }
    }
    sxz = irm_block_reduce256<FrSum>(sxz, pa);
    szz = irm_block_reduce256<FrSum>(szz, pb);
    if (threadIdx.x == 0) {
        part[2 * (long)blockIdx.x] = sxz;
        part[2 * (long)blockIdx.x + 1] = szz;
    }
}

__global__ __launch_bounds__(256) void align_gain_finish_kernel(const double* part, int nparts, double* gain, int* status) {
    __shared__ double pa[4], pb[4];
    double a = 0.0, b = 0.0;
    for (int j = threadIdx.x; j < nparts; j += 256) {
        a += part[2 * (long)j];
        b += part[2 * (long)j + 1];
    }
    a = irm_block_reduce256<FrSum>(a, pa);
    b = irm_block_reduce256<FrSum>(b, pb);
    if (threadIdx.x == 0) {
        const bool ok = b > 0.0;
        *gain = ok ? a / b : 0.0;
        *status = ok ? 0 : 1;
    }
}

struct AlPrep {
    const void* pred;
    const void* target;
    const double* gain;
    float* tmpl;
    float* img;
    int H, W;
    double peak;
    double g[5];
};

// one pixel per thread: five rows of five grey values, rows along x first
template <typename T>
__global__ __launch_bounds__(256) void align_blur_kernel(AlPrep a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)a.H * a.W) return;
    const int y = (int)(idx / a.W), x = (int)(idx - (long)y * a.W);
    const T* Z = reinterpret_cast<const T*>(a.pred);
    const T* X = reinterpret_cast<const T*>(a.target);
    const double gain = *a.gain;
    double vt = 0.0, vi = 0.0;
#pragma unroll
    for (int dy = 0; dy < 5; ++dy) {
        const int yy = al_reflect101(y + dy - 2, a.H);
        double ht = 0.0, hi = 0.0;
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) {
            const int xx = al_reflect101(x + dx - 2, a.W);
            const long p = ((long)yy * a.W + xx) * 3;
            const double t = (0.299 * ((double)X[p] / a.peak) + 0.587 * ((double)X[p + 1] / a.peak)) +
                             0.114 * ((double)X[p + 2] / a.peak);
            const double i = (0.299 * (gain * ((double)Z[p] / a.peak)) + 0.587 * (gain * ((double)Z[p + 1] / a.peak))) +
                             0.114 * (gain * ((double)Z[p + 2] / a.peak));
            ht = ht + a.g[dx] * t;
            hi = hi + a.g[dx] * i;
        }
        vt = vt + a.g[dy] * ht;
        vi = vi + a.g[dy] * hi;
    }
    a.tmpl[idx] = (float)vt;
    a.img[idx] = (float)vi;
}

__global__ __launch_bounds__(256) void align_grad_kernel(const float* img, float* gx, float* gy, int H, int W) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)H * W) return;
    const int y = (int)(idx / W), x = (int)(idx - (long)y * W);
    const float* row = img + (long)y * W;
    gx[idx] = (float)(0.5 * ((double)row[al_reflect101(x + 1, W)] - (double)row[al_reflect101(x - 1, W)]));
    gy[idx] = (float)(0.5 * ((double)img[(long)al_reflect101(y + 1, H) * W + x] -
                             (double)img[(long)al_reflect101(y - 1, H) * W + x]));
}

static bool al_frame_ok(const void* pred, const void* target, int is_u16, int H, int W) {
    if (!pred || !target || !irm_is_flag(is_u16) || H < 11 || W < 11 || (long)H * W * 3 > 0x7fffffffL) return false;
    const uintptr_t mis = is_u16 ? 1 : 0;
    return !((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target)) & mis);
}
static bool al_aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

extern "C" int irm_align_prepare(const void* pred, const void* target, int is_u16, int H, int W, double* gain, int* status,
                                 float* tmpl, float* img, float* gx, float* gy, void* ws, long ws_words,
                                 hipStream_t stream) {
    if (!al_frame_ok(pred, target, is_u16, H, W) || !gain || !status || !tmpl || !img || !gx || !gy || !ws) return IRM_EINVAL;
    if (!al_aligned(gain, 8) || !al_aligned(ws, 8) || !al_aligned(status, 4) || !al_aligned(tmpl, 4) || !al_aligned(img, 4) ||
        !al_aligned(gx, 4) || !al_aligned(gy, 4))
        return IRM_EINVAL;
    const long n = (long)H * W * 3;
    const long nparts = (n + AL_CHUNK - 1) / AL_CHUNK;
    if (ws_words < 2 * nparts) return IRM_EINVAL;
    double* part = reinterpret_cast<double*>(ws);
    AlPrep a{pred, target, gain, tmpl, img, H, W, is_u16 ? 65535.0 : 255.0, {}};
    double gs = 0.0;
    for (int i = 0; i < 5; ++i) {
        a.g[i] = exp(-(double)((i - 2) * (i - 2)) / (2.0 * 1.1 * 1.1));
        gs += a.g[i];
    }
    for (int i = 0; i < 5; ++i) a.g[i] /= gs;
    const unsigned pix_blocks = (unsigned)(((long)H * W + 255) / 256);
    if (is_u16) {
        hipLaunchKernelGGL(align_gain_kernel<unsigned short>, dim3((unsigned)nparts), dim3(256), 0, stream,
                           reinterpret_cast<const unsigned short*>(pred), reinterpret_cast<const unsigned short*>(target), n, part);
    } else {
        hipLaunchKernelGGL(align_gain_kernel<unsigned char>, dim3((unsigned)nparts), dim3(256), 0, stream,
                           reinterpret_cast<const unsigned char*>(pred), reinterpret_cast<const unsigned char*>(target), n, part);
    }
    if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
    hipLaunchKernelGGL(align_gain_finish_kernel, dim3(1), dim3(256), 0, stream, part, (int)nparts, gain, status);
    if (is_u16) hipLaunchKernelGGL(align_blur_kernel<unsigned short>, dim3(pix_blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(align_blur_kernel<unsigned char>, dim3(pix_blocks), dim3(256), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
    hipLaunchKernelGGL(align_grad_kernel, dim3(pix_blocks), dim3(256), 0, stream, img, gx, gy, H, W);
    return irm_launch_status();
}

// ---------------------------------------------------------------------------
// irm_ecc_iterate
struct EccArgs {
    const float* tmpl;
    const float* img;
    const float* gx;
    const float* gy;
    const double* map;
    const int* status;
    double* slots;                     // [blocks][AL_SUMS]
    int H, W, tiles_x;
};

// the bilinear sample of one plane: taps outside the frame (the flags) read 0
__device__ __forceinline__ double al_bilinear(const float* p, long o, int W, bool l, bool r, bool t, bool b, double fx,
                                              double wx0, double fy, double wy0) {
    const double v00 = (t && l) ? (double)p[o] : 0.0, v01 = (t && r) ? (double)p[o + 1] : 0.0;
    const double v10 = (b && l) ? (double)p[o + W] : 0.0, v11 = (b && r) ? (double)p[o + W + 1] : 0.0;
    return (v00 * wx0 + v01 * fx) * wy0 + (v10 * wx0 + v11 * fx) * fy;
}

__global__ __launch_bounds__(256) void ecc_accumulate_kernel(EccArgs a) {
    if (*a.status != 0) return;                    // the same answer for every thread: nobody reaches a barrier
    __shared__ double part[4];
    const AlMap m = al_load_map(a.map);
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const int x = tx * AL_TW + (threadIdx.x & 63);
    double acc[AL_SUMS];
#pragma unroll
    for (int k = 0; k < AL_SUMS; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int r = 0; r < AL_TH / 4; ++r) {
        const int y = ty * AL_TH + (threadIdx.x >> 6) + 4 * r;
        if (x >= a.W || y >= a.H) continue;
        const double xd = (double)x, yd = (double)y;
        double den, px, py;
        al_position(m, xd, yd, den, px, py);
        if (!al_inside(px, py, a.H, a.W)) continue;
        // inside: floor(p) lies in [-1, extent - 1], so the int conversion is safe
        const double fx0 = floor(px), fy0 = floor(py);
        const int x0 = (int)fx0, y0 = (int)fy0;
        const double fx = px - fx0, fy = py - fy0, wx0 = 1.0 - fx, wy0 = 1.0 - fy;
        const bool l = x0 >= 0, rr = x0 + 1 < a.W, t = y0 >= 0, b = y0 + 1 < a.H;
        const long o = (long)y0 * a.W + x0;
        const double vi = al_bilinear(a.img, o, a.W, l, rr, t, b, fx, wx0, fy, wy0);
        const double gx = al_bilinear(a.gx, o, a.W, l, rr, t, b, fx, wx0, fy, wy0);
        const double gy = al_bilinear(a.gy, o, a.W, l, rr, t, b, fx, wx0, fy, wy0);
        const double tv = (double)a.tmpl[(long)y * a.W + x];
        const double ja = gx / den, jb = gy / den, jt = -(px * ja + py * jb);
        const double J[8] = {ja * xd, jb * xd, jt * xd, ja * yd, jb * yd, jt * yd, ja, jb};
        acc[0] += 1.0;
        acc[1] += vi;
        acc[2] += tv;
        acc[3] += vi * vi;
        acc[4] += tv * tv;
        acc[5] += vi * tv;
        int k = 6;
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = i; j < 8; ++j) acc[k++] += J[i] * J[j];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            acc[42 + i] += J[i] * vi;
            acc[50 + i] += J[i] * tv;
            acc[58 + i] += J[i];
        }
    }
    double* slot = a.slots + (long)blockIdx.x * AL_SUMS;
#pragma unroll
    for (int k = 0; k < AL_SUMS; ++k) {
        const double s = irm_block_reduce256<FrSum, true>(acc[k], part);
        if (threadIdx.x == 0) slot[k] = s;
    }
}

// One workgroup: threads 0..65 sum one of the 66 values over the slots in ascending order, thread 0 does the algebra.
__global__ __launch_bounds__(256) void ecc_solve_kernel(const double* slots, int nblocks, double* map, double* rho,
                                                        int* status) {
    if (*status != 0) return;
    __shared__ double S[AL_SUMS];
    if (threadIdx.x < AL_SUMS) {
        double s = 0.0;
        for (int b = 0; b < nblocks; ++b) s += slots[(long)b * AL_SUMS + threadIdx.x];
        S[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double n = S[0];
    if (!(n > 0.0)) { *status = 1; return; }
    const double mi = S[1] / n, mt = S[2] / n;
    const double ni2 = S[3] - mi * S[1], nt2 = S[4] - mt * S[2], corr = S[5] - mi * S[2];
    double bi[8], bt[8], L[8][8];
    for (int i = 0; i < 8; ++i) {
        bi[i] = S[42 + i] - mi * S[58 + i];
        bt[i] = S[50 + i] - mt * S[58 + i];
    }
    const double r = corr / (sqrt(ni2) * sqrt(nt2));
    if (r == r) *rho = r;
    // Cholesky H = L L^T, row by row; the upper triangle of H lies at S[6 + ..] row by row
    int k = 6;
    for (int i = 0; i < 8; ++i)
        for (int j = i; j < 8; ++j) L[j][i] = S[k++];          // L[j][i], j >= i, holds H[i][j] until it is factorised
    for (int j = 0; j < 8; ++j) {
        double d = L[j][j];
        for (int q = 0; q < j; ++q) d = d - L[j][q] * L[j][q];
        if (!(d > 0.0) || !(d < 1.7e308)) { *status = 1; return; }
        const double dj = sqrt(d);
        L[j][j] = dj;
        for (int i = j + 1; i < 8; ++i) {
            double s = L[i][j];
            for (int q = 0; q < j; ++q) s = s - L[i][q] * L[j][q];
            L[i][j] = s / dj;
        }
    }
    auto solve = [&](const double (&rhs)[8], double (&out)[8]) {
        double yv[8];
        for (int i = 0; i < 8; ++i) {
            double s = rhs[i];
            for (int q = 0; q < i; ++q) s = s - L[i][q] * yv[q];
            yv[i] = s / L[i][i];
        }
        for (int i = 7; i >= 0; --i) {
            double s = yv[i];
            for (int q = i + 1; q < 8; ++q) s = s - L[q][i] * out[q];
            out[i] = s / L[i][i];
        }
    };
    double hi[8], res[8], dp[8];
    solve(bi, hi);
    double ln = ni2, ld = corr;
    for (int i = 0; i < 8; ++i) {
        ln = ln - bi[i] * hi[i];
        ld = ld - bt[i] * hi[i];
    }
    if (!(ld > 0.0)) { *status = 1; return; }
    const double lambda = ln / ld;
    for (int i = 0; i < 8; ++i) res[i] = lambda * bt[i] - bi[i];
    solve(res, dp);
    for (int i = 0; i < 8; ++i)
        if (!(fabs(dp[i]) < 1.7e308)) { *status = 1; return; }
    map[0] += dp[0]; map[3] += dp[1]; map[6] += dp[2];
    map[1] += dp[3]; map[4] += dp[4]; map[7] += dp[5];
    map[2] += dp[6]; map[5] += dp[7];
}

extern "C" int irm_ecc_iterate(const float* tmpl, const float* img, const float* gx, const float* gy, int H, int W,
                               int iterations, double* map, double* rho, int* status, void* ws, long ws_words,
                               hipStream_t stream) {
    if (!tmpl || !img || !gx || !gy || !map || !rho || !status || !ws) return IRM_EINVAL;
    if (H < 11 || W < 11 || (long)H * W * 3 > 0x7fffffffL || iterations < 1 || iterations > 10000) return IRM_EINVAL;
    if (!al_aligned(map, 8) || !al_aligned(rho, 8) || !al_aligned(ws, 8) || !al_aligned(status, 4) || !al_aligned(tmpl, 4) ||
        !al_aligned(img, 4) || !al_aligned(gx, 4) || !al_aligned(gy, 4))
        return IRM_EINVAL;
    const int tiles_x = (W + AL_TW - 1) / AL_TW, tiles_y = (H + AL_TH - 1) / AL_TH;
    const long blocks = (long)tiles_x * tiles_y;
    if (ws_words < AL_SUMS * blocks) return IRM_EINVAL;
    EccArgs a{tmpl, img, gx, gy, map, status, reinterpret_cast<double*>(ws), H, W, tiles_x};
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(ecc_accumulate_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(ecc_solve_kernel, dim3(1), dim3(256), 0, stream, a.slots, (int)blocks, map, rho, status);
        if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
    }
    return IRM_OK;
}

// ---------------------------------------------------------------------------
// irm_aligned_metrics
struct AmArgs {
    const void* pred;
    const void* target;
    const double* gain;
    const double* map;
    float* zr;                         // optional
    unsigned char* cr;                 // optional
    double* part;                      // [3][ntiles]: squared error, mask count of the owned pixels, of the valid region
    double* ssim_part;                 // [3][ntiles]: per channel
    int H, W, tiles_x, tiles_y;
    double peak, c1, c2;
    double g[11];
    double cub[32][4];
};

// s + w v, product and sum rounded separately
__device__ __forceinline__ double am_acc(double s, double w, double v) { return __dadd_rn(s, __dmul_rn(w, v)); }

template <typename T>
__global__ __launch_bounds__(256) void aligned_tile_kernel(AmArgs a) {
    using Tile = SsimTile<AM_ROWS, AM_OUT, AM_HALO, 3>;
    constexpr int rw = Tile::rw, pw = rw / 3;
    __shared__ double sx[AM_ROWS + AM_HALO][rw], sy[AM_ROWS + AM_HALO][rw];
    __shared__ double vm[5][rw];
    __shared__ unsigned char sm[AM_ROWS + AM_HALO][pw];
    __shared__ double part[4];
    const Tile tg(a.H, a.W, a.tiles_x, a.tiles_y, blockIdx.x);
    const int ox0 = tg.ox0, oy0 = tg.oy0, nrow = tg.nrow, npix = tg.ncol / 3;
    const T* Z = reinterpret_cast<const T*>(a.pred);
    const T* X = reinterpret_cast<const T*>(a.target);
    const AlMap m = al_load_map(a.map);
    const double gain = *a.gain;

    double err = 0.0, cnt = 0.0;
    for (int i = threadIdx.x; i < nrow * npix; i += 256) {
        const int ly = i / npix, lp = i - ly * npix;
        const int gy = oy0 + ly, gx = ox0 + lp;
        double den, px, py;
        al_position(m, (double)gx, (double)gy, den, px, py);
        const bool in = al_inside(px, py, a.H, a.W);
        double zv[3] = {0.0, 0.0, 0.0}, xv[3] = {0.0, 0.0, 0.0};
        if (in) {
            // inside: |32 p| is below 2^27, the conversion is exact
            const long qx = (long)rint(32.0 * px), qy = (long)rint(32.0 * py);
            const int ix = (int)(qx >> 5) - 1, iy = (int)(qy >> 5) - 1;
            const double* wx = a.cub[qx & 31];
            const double* wy = a.cub[qy & 31];
            int xs[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) xs[j] = al_reflect(ix + j, a.W) * 3;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const T* row = Z + (long)al_reflect(iy + r, a.H) * a.W * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    double h = 0.0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) h = h + wx[j] * (gain * ((double)row[xs[j] + c] / a.peak));
                    zv[c] = zv[c] + wy[r] * h;
                }
            }
            const long p = ((long)gy * a.W + gx) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) xv[c] = (double)X[p + c] / a.peak;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            sx[ly][lp * 3 + c] = xv[c];
            sy[ly][lp * 3 + c] = zv[c];
        }
        sm[ly][lp] = in ? 1 : 0;
        if (tg.owns(gy, gx * 3)) {                 // the owners partition the frame: every pixel is written once
            const long p = (long)gy * a.W + gx;
            cnt += in ? 1.0 : 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double d = xv[c] - zv[c];
                err = err + d * d;
                if (a.zr) a.zr[p * 3 + c] = (float)zv[c];
            }
            if (a.cr) a.cr[p] = in ? 1 : 0;
        }
    }
    __syncthreads();

    const int nout_rows = tg.nout_rows, nout = tg.nout, ncol = tg.ncol;
    const int t = threadIdx.x;
    double acc = 0.0, cntv = 0.0;
#pragma unroll 1
    for (int r = 0; r < nout_rows; ++r) {
        if (t < ncol) {
            double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
            for (int d = 0; d < 11; ++d) {
                const double xv = sx[r + d][t], yv = sy[r + d][t], g = a.g[d];
                s0 = am_acc(s0, g, xv);
                s1 = am_acc(s1, g, yv);
                s2 = am_acc(s2, g, __dmul_rn(xv, xv));
                s3 = am_acc(s3, g, __dmul_rn(yv, yv));
                s4 = am_acc(s4, g, __dmul_rn(xv, yv));
            }
            vm[0][t] = s0;
            vm[1][t] = s1;
            vm[2][t] = s2;
            vm[3][t] = s3;
            vm[4][t] = s4;
        }
        __syncthreads();
        if (t < nout) {                            // t = pixel * 3 + channel; window values t, t + 3, ..., t + 30
            double m1 = 0, m2 = 0, e11 = 0, e22 = 0, e12 = 0;
#pragma unroll
            for (int d = 0; d < 11; ++d) {
                const int j = t + d * 3;
                const double g = a.g[d];
                m1 = am_acc(m1, g, vm[0][j]);
                m2 = am_acc(m2, g, vm[1][j]);
                e11 = am_acc(e11, g, vm[2][j]);
                e22 = am_acc(e22, g, vm[3][j]);
                e12 = am_acc(e12, g, vm[4][j]);
            }
            // as in metrics_basicsr.hip: identical frames give numerator == denominator bitwise, the ratio is exactly 1
            const double m11 = __dmul_rn(m1, m1), m22 = __dmul_rn(m2, m2), m12 = __dmul_rn(m1, m2);
            const double v1 = __dsub_rn(e11, m11), v2 = __dsub_rn(e22, m22), v12 = __dsub_rn(e12, m12);
            const double num = __dmul_rn(__dadd_rn(__dmul_rn(2.0, m12), a.c1), __dadd_rn(__dmul_rn(2.0, v12), a.c2));
            const double den = __dmul_rn(__dadd_rn(__dadd_rn(m11, m22), a.c1), __dadd_rn(__dadd_rn(v1, v2), a.c2));
            if (sm[r + AM_HALO / 2][t / 3 + AM_HALO / 2]) {       // the mask at the window's centre
                acc += num / den;
                if (t % 3 == 0) cntv += 1.0;
            }
        }
        __syncthreads();
    }

    const long ntiles = (long)a.tiles_x * a.tiles_y;
    const double e = irm_block_reduce256<FrSum, true>(err, part);
    const double n = irm_block_reduce256<FrSum, true>(cnt, part);
    const double nv = irm_block_reduce256<FrSum, true>(cntv, part);
    double sc[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) sc[c] = irm_block_reduce256<FrSum, true>(t % 3 == c ? acc : 0.0, part);
    if (t == 0) {
        a.part[blockIdx.x] = e;
        a.part[ntiles + blockIdx.x] = n;
        a.part[2 * ntiles + blockIdx.x] = nv;
#pragma unroll
        for (int c = 0; c < 3; ++c) a.ssim_part[c * ntiles + blockIdx.x] = sc[c];
    }
}

// One workgroup: the six slot families summed in a fixed order
__global__ __launch_bounds__(256) void aligned_reduce_kernel(const double* part, const double* ssim_part, int ntiles,
                                                             double pixels, double* out, int* status) {
    __shared__ double red[4];
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = threadIdx.x; j < ntiles; j += 256) {
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            s[f] += part[(long)f * ntiles + j];
            s[3 + f] += ssim_part[(long)f * ntiles + j];
        }
    }
#pragma unroll
    for (int f = 0; f < 6; ++f) s[f] = irm_block_reduce256<FrSum, true>(s[f], red);
    if (threadIdx.x == 0) {
        out[0] = s[0];
        out[1] = s[1];
        out[2] = s[3];
        out[3] = s[4];
        out[4] = s[5];
        out[5] = out[6] = out[7] = s[2];
        out[8] = s[1] / pixels;
        if (status && !(s[1] > 0.0)) *status = 1;
    }
}

extern "C" int irm_aligned_metrics(const void* pred, const void* target, int is_u16, int H, int W, const double* gain,
                                   const double* map, double* out, int* status, float* zr, unsigned char* cr, void* ws,
                                   long ws_words, hipStream_t stream) {
    if (!al_frame_ok(pred, target, is_u16, H, W) || !gain || !map || !out || !ws) return IRM_EINVAL;
    if (!al_aligned(gain, 8) || !al_aligned(map, 8) || !al_aligned(out, 8) || !al_aligned(ws, 8) || !al_aligned(status, 4) ||
        !al_aligned(zr, 4))
        return IRM_EINVAL;
    SsimPlan p;
    if (!irm_ssim_plan(p, H - AM_HALO, W - AM_HALO, AM_ROWS, AM_OUT / 3, 3, ws, ws_words)) return IRM_EINVAL;
    AmArgs a{pred, target, gain, map, zr, cr, reinterpret_cast<double*>(p.sse_part), p.ssim_part, H, W, p.tiles_x,
             p.tiles_y, is_u16 ? 65535.0 : 255.0, 0.01 * 0.01, 0.03 * 0.03, {}, {}};
    double gs = 0.0;
    for (int i = 0; i < 11; ++i) {
        a.g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        gs += a.g[i];
    }
    for (int i = 0; i < 11; ++i) a.g[i] /= gs;
    const double A = -0.75;
    for (int i = 0; i < 32; ++i) {                 // interpolateCubic; the fourth tap closes the sum to 1
        const double x = (double)i / 32.0, x1 = x + 1.0, x2 = 1.0 - x;
        a.cub[i][0] = ((A * x1 - 5.0 * A) * x1 + 8.0 * A) * x1 - 4.0 * A;
        a.cub[i][1] = (((A + 2.0) * x - (A + 3.0)) * x) * x + 1.0;
        a.cub[i][2] = (((A + 2.0) * x2 - (A + 3.0)) * x2) * x2 + 1.0;
        a.cub[i][3] = ((1.0 - a.cub[i][0]) - a.cub[i][1]) - a.cub[i][2];
    }
    if (is_u16) hipLaunchKernelGGL(aligned_tile_kernel<unsigned short>, dim3((unsigned)p.ntiles), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(aligned_tile_kernel<unsigned char>, dim3((unsigned)p.ntiles), dim3(256), 0, stream, a);
    if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
    hipLaunchKernelGGL(aligned_reduce_kernel, dim3(1), dim3(256), 0, stream, a.part, a.ssim_part, (int)p.ntiles,
                       (double)H * (double)W, out, status);
    return irm_launch_status();
}
