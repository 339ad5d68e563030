// Table-driven resize of K frames [H][W][C], u8 / u16 / f32, C = 1 or 3, to any size (include/irm_hip_resize.h; the
// float64 statement is resize.resize_host).  The filter (bicubic, Lanczos, bilinear), the scale of each axis and the
// antialiasing all live in the two tap tables the host builds (resize.resize_taps): per output coordinate P taps, fp32
// weights that sum to 1 and int32 source indices already reflected into [0, n), PH and PW independent.  At the six
// factors of resize.hip and the bicubic kernel the tables are resize_table's and every output bit is
// irm_imresize_bicubic's: the two kernels spell the same FMA chains.
//
// One workgroup makes RZ_ROWS x tow output pixels of one frame, as imresize_kernel does:
//   1. the source columns its taps touch form one contiguous range [cmin, cmax]: fixed-order min / max over the tile's
//      table rows;
//   2. H pass: for each of the tile's output rows and each value of those columns, the fp32 FMA chain over the PH row
//      taps in ascending order (integer inputs normalised to [0, 1] first: v / 255 or v / 65535, correctly rounded; a
//      float32 input is taken as it is); consecutive threads read consecutive row values; the fp32 intermediate goes to
//      LDS and never to memory;
//   3. W pass: the FMA chain over the PW column taps from LDS (stride C floats per tap), then the store: fp32 as it is,
//      fp32 clamped to [0, 1], or clamped, scaled by 255 / 65535 in fp32 and rounded half to even to the input's type.
// A value is a function of its own taps only: it does not depend on K, on the tile, on tow or on the run.  No atomics.
//
// LDS is dynamic, sized per launch: 16 bytes for the reduction, then RZ_ROWS x ncol_max x C floats, ncol_max the
// largest number of source columns any tile of tow output columns touches.  The host reads it off the W table and
// picks the widest tow whose window stays under 16 KiB (at 1/4 bicubic the 32 columns and 13.4 KiB of imresize_kernel:
// ten workgroups per CU of the 160 KiB, and twice the workgroups of a 64-column tile), or, where no tile does, the
// widest under RZA_WINDOW_BYTES (1/16 with lanczos3, P = 98: 16 columns, 31.7 KiB, five workgroups per CU).
// The kernel clamps every index to the frame and to the window: a wrong table gives wrong pixels, never a wild access.
//
// irm_unit_quantise is the store rule alone, for the float32 frame that travels between the stages of a chain.
#include "irm_frame.h"

#define RZ_ROWS 8
#define RZA_WINDOW_BYTES 32768
#define RZA_MAX_TAPS 128
#define RZA_MAX_SIDE 32768

enum { RZA_U8 = 0, RZA_U16 = 1, RZA_F32 = 2 };            // in_kind
enum { RZA_QUANT = 0, RZA_FLOAT = 1, RZA_UNIT = 2 };      // out_kind

struct ResizeAnyArgs {
    const void* in;                    // [K][H][W][C]
    void* out;                         // [K][OH][OW][C]: fp32 or the input's type
    const float* wh;                   // [OH][PH]
    const int* ih;                     // [OH][PH]
    const float* ww;                   // [OW][PW]
    const int* iw;                     // [OW][PW]
    int H, W, OH, OW, PH, PW, tow, tiles_x, ncol_max;
    float range;                       // 255 or 65535 (1 for f32 frames: never used)
};

template <typename T>
__device__ __forceinline__ float rza_sample(T v, float range) { return (float)v / range; }
template <>
__device__ __forceinline__ float rza_sample<float>(float v, float) { return v; }

template <typename T, int C, int OUT>
__global__ __launch_bounds__(256) void resize_taps_kernel(ResizeAnyArgs a) {
    extern __shared__ __attribute__((aligned(16))) char rza_smem[];
    int* ipart = reinterpret_cast<int*>(rza_smem);                    // 4 ints
    float* mid = reinterpret_cast<float*>(rza_smem + 16);             // [RZ_ROWS][ncol_max][C]
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
            acc = fmaf(w[p], rza_sample<T>(src[(long)y * a.W * C + j], a.range), acc);
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
        if constexpr (OUT == RZA_FLOAT) {
            reinterpret_cast<float*>(a.out)[o] = acc;
        } else if constexpr (OUT == RZA_UNIT) {
            reinterpret_cast<float*>(a.out)[o] = fminf(fmaxf(acc, 0.0f), 1.0f);
        } else {
            const float v = fminf(fmaxf(acc, 0.0f), 1.0f) * a.range;
            reinterpret_cast<T*>(a.out)[o] = (T)rintf(v);       // round half to even
        }
    }
}

template <typename T, int C>
static void launch_resize_any(const ResizeAnyArgs& a, int out_kind, dim3 grid, size_t lds, hipStream_t stream) {
    if (out_kind == RZA_FLOAT) hipLaunchKernelGGL((resize_taps_kernel<T, C, RZA_FLOAT>), grid, dim3(256), lds, stream, a);
    else if (out_kind == RZA_UNIT) hipLaunchKernelGGL((resize_taps_kernel<T, C, RZA_UNIT>), grid, dim3(256), lds, stream, a);
    else if constexpr (!std::is_same<T, float>::value)        // (the entry refuses a quantised output of f32 frames)
        hipLaunchKernelGGL((resize_taps_kernel<T, C, RZA_QUANT>), grid, dim3(256), lds, stream, a);
}

static inline bool rza_tow_ok(int tow) { return tow == 8 || tow == 16 || tow == 32 || tow == 64 || tow == 128; }

extern "C" int irm_resize_taps(const void* in, int in_kind, void* out, int out_kind, const float* wh, const int* ih,
                               const float* ww, const int* iw, int K, int H, int W, int C, int OH, int OW, int PH, int PW,
                               int tow, int ncol_max, hipStream_t stream) {
    if (!in || !out || !wh || !ih || !ww || !iw) return IRM_EINVAL;
    if (in_kind < RZA_U8 || in_kind > RZA_F32 || out_kind < RZA_QUANT || out_kind > RZA_UNIT) return IRM_EINVAL;
    if (in_kind == RZA_F32 && out_kind == RZA_QUANT) return IRM_EINVAL;        // no integer type to quantise to
    if (!irm_frames_ok(in_kind == RZA_U16, K, H, W, C)) return IRM_EINVAL;
    if (H > RZA_MAX_SIDE || W > RZA_MAX_SIDE || OH < 1 || OW < 1) return IRM_EINVAL;
    if (PH < 1 || PW < 1 || PH > RZA_MAX_TAPS || PW > RZA_MAX_TAPS) return IRM_EINVAL;
    if (PH > H || PW > W) return IRM_EINVAL;                                   // one reflection must reach every tap
    if ((long)OH * OW * C > 0x7fffffffL || (long)OH * PH > 0x7fffffffL || (long)OW * PW > 0x7fffffffL) return IRM_EINVAL;
    if (!rza_tow_ok(tow) || ncol_max < 1 || ncol_max > W) return IRM_EINVAL;
    const long window = (long)RZ_ROWS * ncol_max * C * (long)sizeof(float);
    if (window > RZA_WINDOW_BYTES) return IRM_EINVAL;
    const long tiles_x = (OW + tow - 1) / tow, tiles_y = (OH + RZ_ROWS - 1) / RZ_ROWS;
    if (tiles_x * tiles_y > 0x7fffffffL) return IRM_EINVAL;
    ResizeAnyArgs a{in, out, wh, ih, ww, iw, H, W, OH, OW, PH, PW, tow, (int)tiles_x, ncol_max,
                    in_kind == RZA_U16 ? 65535.0f : in_kind == RZA_U8 ? 255.0f : 1.0f};
    const dim3 grid((unsigned)(tiles_x * tiles_y), K);
    const size_t lds = 16 + (size_t)window;
    if (in_kind == RZA_F32) {
        if (C == 3) launch_resize_any<float, 3>(a, out_kind, grid, lds, stream);
        else launch_resize_any<float, 1>(a, out_kind, grid, lds, stream);
    } else {
        irm_dispatch_frames(in_kind == RZA_U16, C, [&](auto kind) {
            launch_resize_any<typename decltype(kind)::type, decltype(kind)::C>(a, out_kind, grid, lds, stream);
        });
    }
    return irm_launch_status();
}

// ---------------------------------------------------------------------------
// The store rule on its own: n float32 values -> u8 / u16, clamp to [0, 1], x 255 (65535) in fp32, round half to even.
template <typename T>
__global__ __launch_bounds__(256) void unit_quantise_kernel(const float* in, T* out, long n, float range) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (T)rintf(fminf(fmaxf(in[i], 0.0f), 1.0f) * range);
}

extern "C" int irm_unit_quantise(const float* in, void* out, int is_u16, long n, hipStream_t stream) {
    if (!in || !out || !irm_is_flag(is_u16) || n < 1 || n > 0x7fffffffL * 256) return IRM_EINVAL;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (is_u16) hipLaunchKernelGGL(unit_quantise_kernel<unsigned short>, grid, dim3(256), 0, stream, in,
                                   reinterpret_cast<unsigned short*>(out), n, 65535.0f);
    else hipLaunchKernelGGL(unit_quantise_kernel<unsigned char>, grid, dim3(256), 0, stream, in,
                            reinterpret_cast<unsigned char*>(out), n, 255.0f);
    return irm_launch_status();
}
