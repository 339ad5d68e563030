// PSNR / SSIM of the two kinds of frame that never pass through 255 RGB levels (include/irm_hip_metrics.h):
//   irm_frame_metrics_f32   K float32 frames [H][W][C] against their targets: fp64 squared error and SSIM;
//   irm_yuv_metrics         the planes of one YUV frame (4:2:0, 4:2:2 or 4:4:4 at 8, 10 or 12 bit; include/irm_hip_video.h)
//                           against the target's, per component: exact integer squared error and SSIM of Y, U and V;
//   irm_yuv420_metrics      the 4:2:0 entry for I420, NV12 and P010: a depth check and a call of irm_yuv_metrics.
// The SSIM is that of metrics.hip (skimage's defaults: 7x7 uniform window, K1 = .01, K2 = .03, sample covariance 49/48,
// mean over the interior), and so are the tile geometry (SsimTile), the workspace slots and the fixed-order sums of
// irm_frame.h.  One kernel template serves all entries; what differs is a policy (Src) that names the plane pair a
// workgroup scores, the stored type and the type of the window moments:
//   float32   moments in fp64.  A float32 product is exact in fp64, the seven-row and then seven-column sums are rounded
//             in that fixed order;
//   8 bit     moments in int32: (49 * 255)^2 < 2^31;
//   10 bit    moments in int64: (49 * 1023)^2 = 2.5e9 does not fit 32 bits;
//   12 bit    moments in int64: (49 * 4095)^2 = 4.0e10.
// The last step forms numerator and denominator from the SAME rounded products (pxx, pyy, pxy below), one rounded
// operation each: identical frames give num == den bit for bit, SSIM exactly 1 and a squared error of exactly 0.  The
// file is built with -ffp-contract=off (csrc/Makefile), so no product is fused into the sum that takes it.
//
// Staging: the tile plus its 3-pixel halo goes to LDS in 16-byte pieces.  A piece is one 16-byte load where the plane
// allows it (base and row pitch 16-byte aligned, neighbours one sample apart) and the whole piece lies inside the row of
// the plane; elsewhere its elements are loaded one by one, and only those inside the staged region.  Nothing outside
// [H][W] of a pitched plane is read.  A thread issues every load of its pieces before it waits for the first.
// No atomics: each workgroup writes its own slot, a second launch sums the slots in a fixed order.
#include "irm_frame.h"
#include <math.h>

#define MV_ROWS 16                     // output rows per tile
#define MV_OUT 192                     // output values (pixel x channel) per tile row
#define MV_NR (MV_ROWS + 6)            // staged rows

typedef unsigned long long mv_u64;

// The plane pair one workgroup scores a tile of
template <typename T>
struct MvPlane {
    const T* P;                        // prediction, first sample
    const T* Q;                        // target
    long pitch_p, pitch_q;             // row pitch in samples
    int step;                          // samples between two neighbours of a row
    int vec_p, vec_q;                  // 16-byte pieces may be loaded whole
    int Hc, Wc;                        // rows and pixels per row
    int tiles_x, tiles_y, tile;
    long slot;                         // workspace slot of this tile
};

template <typename T>
union MvPiece {
    irm_u4 q;
    T e[16 / sizeof(T)];
};

// One piece of a staged row: samples [j0, j0 + VE) of the plane row at `row`, lj0 its place in the tile row.  `whole`:
// one 16-byte load (step is 1 then).  Else element by element, those at or beyond ncol - and a row outside the region -
// replaced by 0 (the load goes to the plane's first sample, so no load waits for a branch).
template <typename T>
__device__ __forceinline__ void mv_load(MvPiece<T>& r, const T* base, long row, int j0, int lj0, int step, bool whole,
                                        bool row_in, int ncol) {
    constexpr int VE = 16 / sizeof(T);
    if (whole) {
        r.q = *reinterpret_cast<const irm_u4*>(base + row + j0);
        return;
    }
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        const bool in = row_in && lj0 + e < ncol;
        const T v = base[in ? row + (long)(j0 + e) * step : 0];
        r.e[e] = in ? v : T(0);
    }
}

// One workgroup: MV_ROWS output rows x (MV_OUT / C) output pixels of one plane pair.  Per output row each thread forms
// the 7-row moments of one staged column, then each thread sums 7 of those along the row for one output value.
template <class Src>
__global__ __launch_bounds__(256) void ssim7_tile_kernel(Src a) {
    using T = typename Src::T;
    using V = typename Src::V;
    using E = typename Src::E;
    constexpr int C = Src::C;
    using Tile = SsimTile<MV_ROWS, MV_OUT, 6, C>;
    constexpr int rw = Tile::rw;                            // staged values per tile row
    constexpr int VE = 16 / sizeof(T);                      // values per piece
    constexpr int PPR = (rw + VE - 1) / VE;                 // pieces per row
    constexpr int RWP = PPR * VE;
    constexpr int NP = (MV_NR * PPR + 255) / 256;           // pieces per thread
    __shared__ __attribute__((aligned(16))) T sx[MV_NR][RWP];
    __shared__ __attribute__((aligned(16))) T sy[MV_NR][RWP];
    __shared__ V vm[5][rw];
    __shared__ double dpart[4];
    __shared__ E epart[4];
    const MvPlane<T> g = a.plane();
    const Tile tg(g.Hc, g.Wc, g.tiles_x, g.tiles_y, g.tile);
    const int ox0 = tg.ox0, oy0 = tg.oy0, nrow = tg.nrow, ncol = tg.ncol;
    const int rowlen = (g.Wc - ox0) * C;                    // what is left of the plane's row: ncol without the cap

    MvPiece<T> xr[NP], yr[NP];
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const int p = threadIdx.x + u * 256, ly = p / PPR, lj0 = (p - ly * PPR) * VE;
        const bool row_in = ly < nrow, fits = row_in && lj0 + VE <= rowlen;
        const int j0 = ox0 * C + lj0;
        mv_load(xr[u], g.P, (long)(oy0 + ly) * g.pitch_p, j0, lj0, g.step, g.vec_p && fits, row_in, ncol);
        mv_load(yr[u], g.Q, (long)(oy0 + ly) * g.pitch_q, j0, lj0, g.step, g.vec_q && fits, row_in, ncol);
    }
    E err = 0;
#pragma unroll
    for (int u = 0; u < NP; ++u) {
        const int p = threadIdx.x + u * 256, ly = p / PPR, lj0 = (p - ly * PPR) * VE;
        if (ly < MV_NR) {
            const int gy = oy0 + ly;
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                const int lj = lj0 + e;
                if (lj < ncol && tg.owns(gy, ox0 * C + lj)) {        // (owned values lie inside the staged region)
                    const V d = a.value(xr[u].e[e]) - a.value(yr[u].e[e]);
                    err += (E)(d * d);
                }
            }
            *reinterpret_cast<irm_u4*>(&sx[ly][lj0]) = xr[u].q;
            *reinterpret_cast<irm_u4*>(&sy[ly][lj0]) = yr[u].q;
        }
    }
    __syncthreads();

    const int nout_rows = tg.nout_rows, nout = tg.nout;
    const int t = threadIdx.x;
    double acc = 0.0;
#pragma unroll 1
    for (int r = 0; r < nout_rows; ++r) {
        if (t < ncol) {
            V s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0;
#pragma unroll
            for (int d = 0; d < 7; ++d) {
                const V xv = a.value(sx[r + d][t]), yv = a.value(sy[r + d][t]);
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
            V sxs = 0, sys = 0, sxx = 0, syy = 0, sxy = 0;
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
            // vx = (49 sxx - sx^2) / (49 * 48): the first factors scaled by 49^2, the second by 49 * 48, with
            // k1 = 49^2 c1, k2 = 49 * 48 c2.  Integer V: every term is exact.  fp64 V: pxx, pyy, pxy are rounded once and
            // used on both sides; 2 p and p + p are the same exact value for identical frames.
            const V pxx = sxs * sxs, pyy = sys * sys, pxy = sxs * sys;
            const V nx = V(49) * sxx - pxx, ny = V(49) * syy - pyy, nxy = V(49) * sxy - pxy;
            const double num = __dmul_rn(__dadd_rn((double)(V(2) * pxy), a.k1), __dadd_rn((double)(V(2) * nxy), a.k2));
            const double den = __dmul_rn(__dadd_rn((double)(pxx + pyy), a.k1), __dadd_rn((double)(nx + ny), a.k2));
            acc += num / den;
        }
        __syncthreads();
    }

    const E e = irm_block_reduce256<FrSum>(err, epart);
    const double s = irm_block_reduce256<FrSum>(acc, dpart);
    if (threadIdx.x == 0) {
        a.sse_part[g.slot] = Src::bits(e);
        a.ssim_part[g.slot] = s;
    }
}

// ---------------------------------------------------------------------------
// float32 frames [K][H][W][C]: blockIdx.y is the frame
template <int C_>
struct F32Src {
    using T = float;
    using V = double;
    using E = double;
    static constexpr int C = C_;
    const float* pred;
    const float* target;
    mv_u64* sse_part;                  // [K][ntiles], fp64 bit patterns
    double* ssim_part;                 // [K][ntiles]
    int H, W, tiles_x, tiles_y, vec;
    double k1, k2;
    __device__ __forceinline__ MvPlane<float> plane() const {
        const long frame = (long)blockIdx.y * H * W * C, pitch = (long)W * C;
        return {pred + frame, target + frame, pitch, pitch, 1, vec, vec, H, W, tiles_x, tiles_y, (int)blockIdx.x,
                (long)blockIdx.y * tiles_x * tiles_y + blockIdx.x};
    }
    __device__ __forceinline__ double value(float v) const { return (double)v; }
    static __device__ __forceinline__ mv_u64 bits(double e) { return (mv_u64)__double_as_longlong(e); }
};

extern "C" int irm_frame_metrics_f32(const float* pred, const float* target, int K, int H, int W, int C,
                                     double data_range, double* sse, double* ssim, void* ws, long ws_words,
                                     hipStream_t stream) {
    if (!pred || !target || !sse || !ssim || !ws) return IRM_EINVAL;
    if (!irm_frames_ok(0, K, H, W, C) || H < 7 || W < 7 || !(data_range > 0.0 && data_range < INFINITY)) return IRM_EINVAL;
    if ((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target)) & 3) return IRM_EINVAL;
    if ((reinterpret_cast<uintptr_t>(sse) | reinterpret_cast<uintptr_t>(ssim) | reinterpret_cast<uintptr_t>(ws)) & 7)
        return IRM_EINVAL;
    SsimPlan p;
    if (!irm_ssim_plan(p, H - 6, W - 6, MV_ROWS, MV_OUT / C, K, ws, ws_words)) return IRM_EINVAL;
    const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
    // whole pieces: every row of every frame starts on a 16-byte boundary (a tile starts 192 values into its row)
    const int vec = ((long)W * C) % 4 == 0 && irm_aligned16(pred) && irm_aligned16(target);
    const dim3 grid((unsigned)p.ntiles, K);
    if (C == 3) {
        const F32Src<3> a{pred, target, p.sse_part, p.ssim_part, H, W, p.tiles_x, p.tiles_y, vec, 2401.0 * c1, 2352.0 * c2};
        hipLaunchKernelGGL(ssim7_tile_kernel<F32Src<3>>, grid, dim3(256), 0, stream, a);
    } else {
        const F32Src<1> a{pred, target, p.sse_part, p.ssim_part, H, W, p.tiles_x, p.tiles_y, vec, 2401.0 * c1, 2352.0 * c2};
        hipLaunchKernelGGL(ssim7_tile_kernel<F32Src<1>>, grid, dim3(256), 0, stream, a);
    }
    if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
    const double count = (double)C * (H - 6) * (W - 6);   // interior values of one frame
    hipLaunchKernelGGL(ssim_reduce_kernel<true>, dim3(K), dim3(256), 0, stream, p.sse_part, p.ssim_part, (int)p.ntiles,
                       count, reinterpret_cast<mv_u64*>(sse), ssim);
    return irm_launch_status();
}

// ---------------------------------------------------------------------------
// YUV planes: the tiles of Y, then those of U, then those of V, in one grid; a tile's slot is its block
struct YuvSide {
    const void* y;
    const void* u;
    const void* v;
    long pitch_y, pitch_c;
    int step, vec_y, vec_c;
};

template <typename T_, typename V_>
struct YuvSrc {
    using T = T_;
    using V = V_;                      // the exact window moments: see the head
    using E = mv_u64;
    static constexpr int C = 1;
    YuvSide p, q;
    mv_u64* sse_part;                  // [ny + 2 nc]
    double* ssim_part;
    int H, W, CH, CW, shift;           // luma and chroma extents
    int ny, ytx, yty, nc, ctx, cty;    // tiles of the luma plane and of one chroma plane
    double k1, k2;
    __device__ __forceinline__ MvPlane<T> plane() const {
        const int b = blockIdx.x;
        if (b < ny)
            return {(const T*)p.y, (const T*)q.y, p.pitch_y, q.pitch_y, 1, p.vec_y, q.vec_y, H, W, ytx, yty, b, b};
        const bool is_v = b - ny >= nc;
        return {(const T*)(is_v ? p.v : p.u), (const T*)(is_v ? q.v : q.u), p.pitch_c, q.pitch_c, p.step, p.vec_c,
                q.vec_c, CH, CW, ctx, cty, b - ny - (is_v ? nc : 0), b};
    }
    __device__ __forceinline__ V value(T s) const { return (V)(s >> shift); }
    static __device__ __forceinline__ mv_u64 bits(mv_u64 e) { return e; }
};

// One workgroup per component: its slots summed in a fixed order
__global__ __launch_bounds__(256) void yuv_reduce_kernel(const mv_u64* sse_part, const double* ssim_part, int ny, int nc,
                                                         double count_y, double count_c, mv_u64* sse, double* ssim) {
    __shared__ double dpart[4];
    __shared__ mv_u64 upart[4];
    const int comp = blockIdx.x;
    const int base = comp == 0 ? 0 : ny + (comp - 1) * nc, n = comp == 0 ? ny : nc;
    mv_u64 e = 0;
    double s = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) {
        e += sse_part[base + j];
        s += ssim_part[base + j];
    }
    s = irm_block_reduce256<FrSum>(s, dpart);
    e = irm_block_reduce256<FrSum>(e, upart);
    if (threadIdx.x == 0) {
        sse[comp] = e;
        ssim[comp] = s / (comp == 0 ? count_y : count_c);
    }
}

// The checks of one side and its piece flags; es = bytes per sample
static bool yuv_side(YuvSide& s, const void* y, const void* u, const void* v, int step, long pitch_y, long pitch_c,
                     int luma_only, int W, int CW, uintptr_t es) {
    if (!y || pitch_y < W || (reinterpret_cast<uintptr_t>(y) & (es - 1))) return false;
    s = YuvSide{y, u, v, pitch_y, pitch_c, step, 0, 0};
    s.vec_y = irm_aligned16(y) && (pitch_y * (long)es) % 16 == 0;
    if (luma_only) return true;
    if (!u || !v || (step != 1 && step != 2) || pitch_c < (long)step * CW) return false;
    if ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(v)) & (es - 1)) return false;
    s.vec_c = step == 1 && irm_aligned16(u) && irm_aligned16(v) && (pitch_c * (long)es) % 16 == 0;
    return true;
}

// The checks of the extents, the sides and the workspace, and the two launches.  The code of an upper-bits word is
// the word shifted right by 16 - depth.
extern "C" int irm_yuv_metrics(const void* pred_y, const void* pred_u, const void* pred_v, int pred_step,
                               long pred_pitch_y, long pred_pitch_c, const void* target_y, const void* target_u,
                               const void* target_v, int target_step, long target_pitch_y, long target_pitch_c, int sub_w,
                               int sub_h, int depth, int upper_bits, int luma_only, int H, int W, unsigned long long* sse,
                               double* ssim, void* ws, long ws_words, hipStream_t stream) {
    if (!sse || !ssim || !ws) return IRM_EINVAL;
    if ((reinterpret_cast<uintptr_t>(sse) | reinterpret_cast<uintptr_t>(ssim) | reinterpret_cast<uintptr_t>(ws)) & 7)
        return IRM_EINVAL;
    if (!((sub_w == 2 && sub_h == 2) || (sub_w == 2 && sub_h == 1) || (sub_w == 1 && sub_h == 1))) return IRM_EINVAL;
    if ((depth != 8 && depth != 10 && depth != 12) || !irm_is_flag(upper_bits) || (depth == 8 && upper_bits)
        || !irm_is_flag(luma_only)) return IRM_EINVAL;
    if (H <= 0 || W <= 0 || H % sub_h || W % sub_w || H > (1 << 20) || W > (1 << 20)) return IRM_EINVAL;
    // a chroma plane holds one 7 x 7 window; the luma plane alone with luma_only
    if (luma_only ? (H < 7 || W < 7) : (H / sub_h < 7 || W / sub_w < 7)) return IRM_EINVAL;
    const int CH = H / sub_h, CW = W / sub_w, shift = upper_bits ? 16 - depth : 0;
    const uintptr_t es = depth == 8 ? 1 : 2;
    YuvSide p, q;
    if (!yuv_side(p, pred_y, pred_u, pred_v, pred_step, pred_pitch_y, pred_pitch_c, luma_only, W, CW, es)) return IRM_EINVAL;
    if (!yuv_side(q, target_y, target_u, target_v, target_step, target_pitch_y, target_pitch_c, luma_only, W, CW, es))
        return IRM_EINVAL;
    if (!luma_only && pred_step != target_step) return IRM_EINVAL;
    const int ytx = (W - 6 + MV_OUT - 1) / MV_OUT, yty = (H - 6 + MV_ROWS - 1) / MV_ROWS;
    const int ctx = luma_only ? 0 : (CW - 6 + MV_OUT - 1) / MV_OUT, cty = luma_only ? 0 : (CH - 6 + MV_ROWS - 1) / MV_ROWS;
    const long ny = (long)ytx * yty, nc = (long)ctx * cty, total = ny + 2 * nc;
    if (ws_words < 2 * total || total > 0x7fffffffL) return IRM_EINVAL;
    mv_u64* sse_part = reinterpret_cast<mv_u64*>(ws);
    double* ssim_part = reinterpret_cast<double*>(sse_part + total);
    const double range = (double)((1 << depth) - 1);
    const double c1 = (0.01 * range) * (0.01 * range), c2 = (0.03 * range) * (0.03 * range);
    if (depth == 8) {
        const YuvSrc<unsigned char, int> a{p, q, sse_part, ssim_part, H, W, CH, CW, shift, (int)ny, ytx, yty, (int)nc, ctx,
                                           cty, 2401.0 * c1, 2352.0 * c2};
        hipLaunchKernelGGL((ssim7_tile_kernel<YuvSrc<unsigned char, int>>), dim3((unsigned)total), dim3(256), 0, stream, a);
    } else {
        const YuvSrc<unsigned short, long long> a{p, q, sse_part, ssim_part, H, W, CH, CW, shift, (int)ny, ytx, yty, (int)nc,
                                                  ctx, cty, 2401.0 * c1, 2352.0 * c2};
        hipLaunchKernelGGL((ssim7_tile_kernel<YuvSrc<unsigned short, long long>>), dim3((unsigned)total), dim3(256), 0,
                           stream, a);
    }
    if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
    const double count_y = (double)(H - 6) * (W - 6), count_c = (double)(CH - 6) * (CW - 6);
    hipLaunchKernelGGL(yuv_reduce_kernel, dim3(luma_only ? 1 : 3), dim3(256), 0, stream, sse_part, ssim_part, (int)ny,
                       (int)nc, count_y, count_c, sse, ssim);
    return irm_launch_status();
}

// The 4:2:0 entry of include/irm_hip_metrics.h: depths 8 and 10 only, as it was (is_p010 is upper_bits at 10 bit)
extern "C" int irm_yuv420_metrics(const void* pred_y, const void* pred_u, const void* pred_v, int pred_step,
                                  long pred_pitch_y, long pred_pitch_c, const void* target_y, const void* target_u,
                                  const void* target_v, int target_step, long target_pitch_y, long target_pitch_c,
                                  int depth, int is_p010, int luma_only, int H, int W, unsigned long long* sse,
                                  double* ssim, void* ws, long ws_words, hipStream_t stream) {
    if ((depth != 8 && depth != 10) || !irm_is_flag(is_p010)) return IRM_EINVAL;
    return irm_yuv_metrics(pred_y, pred_u, pred_v, pred_step, pred_pitch_y, pred_pitch_c, target_y, target_u, target_v,
                           target_step, target_pitch_y, target_pitch_c, 2, 2, depth, is_p010, luma_only, H, W, sse, ssim,
                           ws, ws_words, stream);
}
