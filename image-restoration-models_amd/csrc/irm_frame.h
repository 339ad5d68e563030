// Shared pieces of the frame-side kernels (tiler.hip, tiler_f32.hip, metrics.hip, metrics_basicsr.hip, resize.hip,
// niqe.hip and the statistics of fpn.hip): the fixed-order workgroup reduction, the u8 / u16 x C dispatch and the
// head of the frame-batch argument check, the tile walk of the tiled-patch loop (extract and window blend) and the
// output-tile geometry, workspace plan and slot reduction of the two SSIM kernels.  These kernels are bit-exact
// against the reference's loops, so each of these ideas has exactly one spelling.  No atomics in this file: the
// tiler's squared-error sum stays in tiler.hip.
#pragma once
#include "irm_common.h"
#include <type_traits>

// ---------------------------------------------------------------------------
// Reduction over a workgroup of 256 threads in a fixed order: butterfly 32..1 in each wave, then the four waves left
// to right; every thread gets the result.  REUSE: `part` held an earlier result that some thread may not have read
// yet, so a barrier comes before it is written again.
struct FrSum { template <typename V> __device__ __forceinline__ V operator()(V a, V b) const { return a + b; } };
struct FrMin {
    __device__ __forceinline__ int operator()(int a, int b) const { return min(a, b); }
    __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
};
struct FrMax { __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); } };

template <class Op, bool REUSE = false, typename V>
__device__ __forceinline__ V irm_block_reduce256(V v, V* part) {
    const Op op;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    if (REUSE) __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(op(part[0], part[1]), part[2]), part[3]);
}

// ---------------------------------------------------------------------------
// Frame batches [K][H][W][C], u8 or u16, C = 1 or 3.  The head of their argument check: the type flag, K as a grid
// dimension, the channel count and a frame that an int can index.  The entries add the conditions that are their own.
static inline bool irm_is_flag(int v) { return v == 0 || v == 1; }
static inline bool irm_frames_ok(int is_u16, int K, int H, int W, int C) {
    return irm_is_flag(is_u16) && K > 0 && K <= 65535 && (C == 1 || C == 3) && H > 0 && W > 0 &&
           (long)H * W * C <= 0x7fffffffL;
}

// f(FrameKind<sample type, C>{}) for the frame's type and channel count, both compile-time constants in f
template <typename T, int C_>
struct FrameKind {
    using type = T;
    static constexpr int C = C_;
};
template <class F>
static inline auto irm_dispatch_frames(int is_u16, int C, F&& f) {
    if (is_u16 && C == 3) return f(FrameKind<unsigned short, 3>{});
    if (is_u16) return f(FrameKind<unsigned short, 1>{});
    if (C == 3) return f(FrameKind<unsigned char, 3>{});
    return f(FrameKind<unsigned char, 1>{});
}

// ---------------------------------------------------------------------------
// Tile walk, extract side (src/utils.py:353-454): an HWC frame is cut into T equal-shape tiles [T][C][ph][pw].
struct TileCut {
    const int* origins;    // [T][2] (y0, x0)
    const double* noise;   // [th][tw][C] float64 field (same for every tile) or null
    float* tiles;          // [T][C][ph][pw]
    int H, W, C, th, tw, ph, pw, T;
    int pad_zero;          // 0: reflect pad (utils.pad), 1: zero pad (deblurganv2.pad)
};

static inline bool irm_tile_cut_ok(const void* img, const TileCut& g) {
    if (!img || !g.origins || !g.tiles || g.H <= 0 || g.W <= 0 || g.C <= 0 || g.T <= 0) return false;
    if (g.th <= 0 || g.tw <= 0 || g.ph < g.th || g.pw < g.tw || g.th > g.H || g.tw > g.W) return false;
    return g.pad_zero || (g.ph - g.th < g.th && g.pw - g.tw < g.tw);          // reflect needs pad < extent
}
static inline unsigned irm_tile_cut_blocks(const TileCut& g) {
    return (unsigned)(((long)g.T * g.C * g.ph * g.pw + 255) / 256);
}

// One tile element per thread; value(src) is the normalised sample at frame index src = (y W + x) C + c.
template <class Value>
__device__ __forceinline__ void irm_extract_element(const TileCut& g, Value value) {
    const long total = (long)g.T * g.C * g.ph * g.pw;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int px = (int)(idx % g.pw);
    long t = idx / g.pw;
    const int py = (int)(t % g.ph); t /= g.ph;
    const int c = (int)(t % g.C);
    const int tile = (int)(t / g.C);
    if (g.pad_zero && (py >= g.th || px >= g.tw)) {          // deblurganv2/__init__.py:16-24
        g.tiles[idx] = 0.0f;
        return;
    }
    // reflect (no edge repeat) for the padded rows/cols: utils.py:174-181
    const int sy = py < g.th ? py : 2 * g.th - 2 - py;
    const int sx = px < g.tw ? px : 2 * g.tw - 2 - px;
    const int gy = g.origins[tile * 2] + sy, gx = g.origins[tile * 2 + 1] + sx;
    float v = value(((long)gy * g.W + gx) * g.C + c);
    if (g.noise) {                                          // utils.py:29-36
        const double d = (double)v + g.noise[((long)sy * g.tw + sx) * g.C + c];
        v = (float)fmin(fmax(d, 0.0), 1.0);
    }
    g.tiles[idx] = v;
}

// Tile walk, blend side: the per-tile predictions go back into an HWC frame under the window.
struct TileBlend {
    const float* pred;     // [T][Cp][ph][pw], only [:Co][:th][:tw] is used
    const int* origins;    // [T][2], in the reference's loop order, in input pixels
    const float* window;   // [ps][ps]
    int H, W, Co, Cp, th, tw, ph, pw, ps, T;     // at output scale once irm_tile_blend_plan has run
    int scale;             // super-resolution factor s: the origins are multiplied by it
};

// The checks, then every extent brought to output scale.  `scaled`: the entry takes a factor and indexes with ints.
static inline bool irm_tile_blend_plan(TileBlend& g, const void* out, bool scaled) {
    if (!g.pred || !g.origins || !g.window || !out || g.H <= 0 || g.W <= 0 || g.Co <= 0 || g.Cp < g.Co || g.T <= 0)
        return false;
    if (g.th <= 0 || g.tw <= 0 || g.ph < g.th || g.pw < g.tw || g.th > g.ps || g.tw > g.ps) return false;
    const int s = g.scale;
    if (scaled) {
        if (s < 1 || s > 8) return false;
        // int indices inside the kernel: output rows / columns and the window index (s ps)^2 stay below 2^31
        if ((long)g.H * s > (1L << 20) || (long)g.W * s > (1L << 20) || (long)g.ps * s * g.ps * s >= (1L << 31))
            return false;
    }
    g.H *= s; g.W *= s; g.th *= s; g.tw *= s; g.ph *= s; g.pw *= s; g.ps *= s;
    return true;
}

// The blended value of output element idx = (y W + x) Co + c: the window-weighted sum over the tiles that cover it,
// divided by the weight sum.  SCALED: the origins are multiplied by g.scale; pred_of(p) is the entry's transform of a
// prediction before it is weighted.
template <bool SCALED, class PredOf>
__device__ __forceinline__ float irm_blend_element(const TileBlend& g, long idx, PredOf pred_of) {
    const int c = (int)(idx % g.Co);
    const long t = idx / g.Co;
    const int x = (int)(t % g.W), y = (int)(t / g.W);
    float acc = 0.0f, wsum = 0.0f;
    for (int i = 0; i < g.T; ++i) {                // same order as the h_idx / w_idx loops
        const int oy = SCALED ? g.origins[2 * i] * g.scale : g.origins[2 * i];
        const int ox = SCALED ? g.origins[2 * i + 1] * g.scale : g.origins[2 * i + 1];
        const int ly = y - oy, lx = x - ox;
        if (ly < 0 || ly >= g.th || lx < 0 || lx >= g.tw) continue;
        const float p = pred_of(g.pred[(((long)i * g.Cp + c) * g.ph + ly) * g.pw + lx]);
        const float w = g.window[ly * g.ps + lx];
        acc = __fadd_rn(acc, __fmul_rn(p, w));          // utils.py:433
        wsum = __fadd_rn(wsum, w);                       // utils.py:434
    }
    return __fdiv_rn(acc, fmaxf(wsum, 1e-8f));           // utils.py:440
}

// ---------------------------------------------------------------------------
// The two SSIM kernels (metrics.hip: 7-box, metrics_basicsr.hip: 11-tap Gaussian).  One workgroup makes ROWS output
// rows x (OUT / CE) output pixels of one (cropped) frame Hc x Wc with CE kept channels; a window spans HALO + 1
// values, so the tile stages ROWS + HALO rows of rw values.
template <int ROWS, int OUT, int HALO, int CE>
struct SsimTile {
    static constexpr int twp = OUT / CE, rw = (twp + HALO) * CE;     // output pixels, staged values per tile row
    int ox0, oy0;              // first output pixel and row
    int nrow, ncol;            // staged region: frame rows [oy0, oy0 + nrow), row values [ox0 CE, ox0 CE + ncol)
    int cy0, cy1, cx0, cx1;    // SSE ownership, rows and row values
    int nout_rows, nout;       // valid output rows, and values per row: their windows lie inside ncol

    __device__ __forceinline__ SsimTile(int Hc, int Wc, int tiles_x, int tiles_y, unsigned block) {
        const int tx = block % tiles_x, ty = block / tiles_x;
        ox0 = tx * twp;
        oy0 = ty * ROWS;
        nrow = min(ROWS + HALO, Hc - oy0);
        ncol = min(rw, (Wc - ox0) * CE);
        // SSE ownership: the tile's output centres, widened to the border for the first / last tile of a row or
        // column, so that the tiles of a frame partition the (cropped) frame exactly
        cy0 = ty == 0 ? 0 : oy0 + HALO / 2;
        cy1 = ty == tiles_y - 1 ? Hc : oy0 + ROWS + HALO / 2;
        cx0 = (tx == 0 ? 0 : ox0 + HALO / 2) * CE;
        cx1 = (tx == tiles_x - 1 ? Wc : ox0 + twp + HALO / 2) * CE;
        nout_rows = min(ROWS, Hc - HALO - oy0);
        nout = min(twp, Wc - HALO - ox0) * CE;
    }
    __device__ __forceinline__ bool owns(int gy, int gj) const { return gy >= cy0 && gy < cy1 && gj >= cx0 && gj < cx1; }
};

// Host side: the tile counts for Ho x Wo output pixels in tiles of rows x twp, and the workspace [2][K][ntiles] split
// into the u64 SSE slots and the fp64 SSIM slots.  False where the workspace is too short.
struct SsimPlan {
    int tiles_x, tiles_y;
    long ntiles;
    unsigned long long* sse_part;
    double* ssim_part;
};
static inline bool irm_ssim_plan(SsimPlan& p, int Ho, int Wo, int rows, int twp, int K, void* ws, long ws_words) {
    p.tiles_x = (Wo + twp - 1) / twp;
    p.tiles_y = (Ho + rows - 1) / rows;
    p.ntiles = (long)p.tiles_x * p.tiles_y;
    if (ws_words < 2 * K * p.ntiles) return false;
    p.sse_part = reinterpret_cast<unsigned long long*>(ws);
    p.ssim_part = reinterpret_cast<double*>(p.sse_part + K * p.ntiles);
    return true;
}

// One workgroup per frame: its tile slots summed in a fixed order.  F64: the SSE slots hold fp64 bit patterns.
template <bool F64>
__global__ __launch_bounds__(256) void ssim_reduce_kernel(const unsigned long long* sse_part, const double* ssim_part,
                                                          int ntiles, double count, unsigned long long* sse,
                                                          double* ssim) {
    __shared__ double dpart[4], epart[4];
    __shared__ unsigned long long upart[4];
    const long base = (long)blockIdx.x * ntiles;
    unsigned long long e = 0;
    double ed = 0.0, s = 0.0;
    for (int j = threadIdx.x; j < ntiles; j += 256) {
        if (F64) ed += __longlong_as_double((long long)sse_part[base + j]);
        else e += sse_part[base + j];
        s += ssim_part[base + j];
    }
    s = irm_block_reduce256<FrSum>(s, dpart);
    if (F64) e = (unsigned long long)__double_as_longlong(irm_block_reduce256<FrSum>(ed, epart));
    else e = irm_block_reduce256<FrSum>(e, upart);
    if (threadIdx.x == 0) {
        sse[blockIdx.x] = e;
        ssim[blockIdx.x] = s / count;
    }
}
