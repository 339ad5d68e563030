// MATLAB-compatible bicubic resize (imresize with antialiasing) of K frames [H][W][C], u8 or u16, C = 1 or 3, by an
// integer factor s or 1/s (s = 2, 3, 4) - the resize every super-resolution table makes its low-resolution frames with
// (the reference carries it as basicsr's matlab_functions.imresize; the host restatement is utils.imresize_host).
//
// The host builds, per axis, a table of P taps per output coordinate (utils.resize_table): fp32 weights that sum to 1
// and int32 source indices already reflected into [0, n).  P = 6 when enlarging, 4 s + 2 when shrinking (18 at 1/4).
//
// One workgroup makes RZ_ROWS x tow output pixels of one frame (tow = 32 shrinking, 128 enlarging):
//   1. the source columns its taps touch form one contiguous range [cmin, cmax] (reflection folds a contiguous span
//      onto a contiguous range): found with a fixed-order min / max over the tile's table rows;
//   2. H pass: for each of the tile's output rows and each value of those columns, the fp32 FMA chain over the P row
//      taps in ascending order, inputs normalised to [0, 1] (v / 255 or v / 65535, correctly rounded) first; the fp32
//      intermediate goes to LDS and never to memory;
//   3. W pass: the FMA chain over the P column taps from LDS, then the store: fp32 as it is, or clamped to [0, 1],
//      scaled by 255 / 65535 in fp32 and rounded half to even to the input's type.
// A value is a function of its own taps only: it does not depend on K, on the tile or on the run.  No atomics.
//
// LDS: RZ_ROWS rows x ncol columns x C floats, ncol <= floor((tow - 1) / scale) + 1 + P; at 1/4 with tow = 32 that
// is 8 x 143 x 3 floats = 13.4 KiB, which RZ_LDS_FLOATS is sized for (several workgroups per CU).
#include "irm_frame.h"

#define RZ_ROWS 8
#define RZ_LDS_FLOATS (RZ_ROWS * 143 * 3)

struct ResizeArgs {
    const void* in;                    // [K][H][W][C]
    void* out;                         // [K][OH][OW][C]: fp32 or the input's type
    const float* wh;                   // [OH][PH]
    const int* ih;                     // [OH][PH]
    const float* ww;                   // [OW][PW]
    const int* iw;                     // [OW][PW]
    int H, W, OH, OW, PH, PW, tow, tiles_x, ncol_max;
    float range;                       // 255 or 65535
};

template <typename T, int C, bool OUT_FLOAT>
__global__ __launch_bounds__(256) void imresize_kernel(ResizeArgs a) {
    __shared__ float mid[RZ_LDS_FLOATS];
    __shared__ int ipart[4];
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x, k = blockIdx.y;
    const int ox0 = tx * a.tow, oy0 = ty * RZ_ROWS;
    const int nox = min(a.tow, a.OW - ox0), noy = min(RZ_ROWS, a.OH - oy0);
    const int t = threadIdx.x;

    // 1. source column range of the tile (indices clamped: a wrong table cannot read outside the frame)
    int lo = a.W - 1, hi = 0;
    for (int e = t; e < nox * a.PW; e += 256) {
        const int c = min(max(a.iw[(long)ox0 * a.PW + e], 0), a.W - 1);
        lo = min(lo, c);
        hi = max(hi, c);
    }
    const int cmin = irm_block_reduce256<FrMin, true>(lo, ipart);      // (true: `ipart` serves both reductions)
    const int cmax = -irm_block_reduce256<FrMin, true>(-hi, ipart);
    const int ncol = min(cmax - cmin + 1, a.ncol_max);        // (<= ncol_max by construction of the table)
    const int rowv = ncol * C;                                // values per intermediate row

    // 2. H pass
    const T* src = reinterpret_cast<const T*>(a.in) + (long)k * a.H * a.W * C + (long)cmin * C;
    for (int e = t; e < noy * rowv; e += 256) {
        const int r = e / rowv, j = e - r * rowv;
        const float* w = a.wh + (long)(oy0 + r) * a.PH;
        const int* id = a.ih + (long)(oy0 + r) * a.PH;
        float acc = 0.0f;
        for (int p = 0; p < a.PH; ++p) {
            const int y = min(max(id[p], 0), a.H - 1);
            acc = fmaf(w[p], (float)src[(long)y * a.W * C + j] / a.range, acc);
        }
        mid[e] = acc;
    }
    __syncthreads();

    // 3. W pass and store
    for (int e = t; e < noy * nox * C; e += 256) {
        const int r = e / (nox * C), q = e - r * (nox * C), x = q / C, ch = q - x * C;
        const float* w = a.ww + (long)(ox0 + x) * a.PW;
        const int* id = a.iw + (long)(ox0 + x) * a.PW;
        float acc = 0.0f;
        for (int p = 0; p < a.PW; ++p) {
            const int c = min(max(id[p] - cmin, 0), ncol - 1);
            acc = fmaf(w[p], mid[r * rowv + c * C + ch], acc);
        }
        const long o = (((long)k * a.OH + oy0 + r) * a.OW + ox0 + x) * C + ch;
        if (OUT_FLOAT) {
            reinterpret_cast<float*>(a.out)[o] = acc;
        } else {
            const float v = fminf(fmaxf(acc, 0.0f), 1.0f) * a.range;
            reinterpret_cast<T*>(a.out)[o] = (T)rintf(v);       // round half to even
        }
    }
}

template <typename T, int C>
static void launch_resize(const ResizeArgs& a, int out_float, dim3 grid, hipStream_t stream) {
    if (out_float) hipLaunchKernelGGL((imresize_kernel<T, C, true>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((imresize_kernel<T, C, false>), grid, dim3(256), 0, stream, a);
}

extern "C" int irm_imresize_bicubic(const void* in, int is_u16, void* out, int out_float, const float* wh, const int* ih,
                                    const float* ww, const int* iw, int K, int H, int W, int C, int s, int shrink,
                                    hipStream_t stream) {
    if (!in || !out || !wh || !ih || !ww || !iw) return IRM_EINVAL;
    if (!irm_frames_ok(is_u16, K, H, W, C) || !irm_is_flag(out_float) || !irm_is_flag(shrink)) return IRM_EINVAL;
    if (s < 2 || s > 4) return IRM_EINVAL;
    const int P = shrink ? 4 * s + 2 : 6;
    if (H < P || W < P || H > 32768 || W > 32768) return IRM_EINVAL;           // one reflection must reach every tap
    const int OH = shrink ? (H + s - 1) / s : H * s, OW = shrink ? (W + s - 1) / s : W * s;
    if ((long)OH * OW * C > 0x7fffffffL) return IRM_EINVAL;
    const int tow = shrink ? 32 : 128;
    const int ncol_max = (shrink ? (tow - 1) * s : (tow - 1) / s) + 1 + P;
    if (RZ_ROWS * ncol_max * C > RZ_LDS_FLOATS) return IRM_EINVAL;
    const int tiles_x = (OW + tow - 1) / tow, tiles_y = (OH + RZ_ROWS - 1) / RZ_ROWS;
    ResizeArgs a{in, out, wh, ih, ww, iw, H, W, OH, OW, P, P, tow, tiles_x, ncol_max, is_u16 ? 65535.0f : 255.0f};
    const dim3 grid((unsigned)(tiles_x * tiles_y), K);
    irm_dispatch_frames(is_u16, C, [&](auto kind) {
        launch_resize<typename decltype(kind)::type, decltype(kind)::C>(a, out_float, grid, stream);
    });
    return irm_launch_status();
}
