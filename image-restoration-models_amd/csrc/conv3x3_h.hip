// Dense 3x3 convolution (stride 1, zero pad 1) on NATIVE fp16 operands: the reduced-precision mode of the conv stacks
// (DnCNN network_dncnn.py:40-71, REDNet rednet.py:64-136).  Activations between layers are fp16 channel-last
// [B][H][W][C], C in {64, 128}: a pixel's channels are one or two 128-byte lines and the 8 channels of an MFMA operand
// fragment are one 16-byte read.  Three kernels:
//   in   fp32 planar [B][Ci <= 3][H][W] -> fp16 channel-last, fp32 FMAs on the vector pipe (<= 27 per output);
//   mid  fp16 channel-last -> fp16 channel-last, ONE v_mfma_f32_16x16x32_f16 per k-step, fp32 accumulation;
//   out  fp16 channel-last -> fp32 planar [B][Co <= 3][H][W], fp32 FMAs on the vector pipe, output not rounded to fp16.
// Every fp16 store is one round-to-nearest-even conversion of the fp32 epilogue value: beyond +-65504 it gives +-inf,
// NaN stays NaN (the ReLUs here let NaN through), nothing is clamped - a broken chain stays visible.
//
// mid: one workgroup (8 waves) = an 8 x 32 pixel tile and CT output tiles of 16 channels; wave w owns row w (2 MFMA
// tiles of 16 pixels).  The halo tile (10 x 34 pixels) of every 64-channel stage arrives by LDS-DMA straight into the
// operand image - 16-byte chunk c of halo pixel p at slot 8 p + (c ^ 2 ((p >> 1) & 3)): with the 128-byte pixel stride
// two pixels share a bank row, the XOR puts the 16 lanes of every ds_read_b128 lane group (8 pixels of one parity pair
// x 2 chunks) on 16 different slots for any tap offset.  Chunks outside the image read a zero page.  The weights are the
// MFMA A operand (rows = output channels), so a lane ends up with 4 consecutive channels of one pixel: an 8-byte
// channel-last store.  They stream per (stage, tap) through a double-buffered LDS area (host packed, L2 resident).
#include "irm_common.h"

#define CH_TH 8
#define CH_TW 32
#define CH_HC 34
#define CH_NP 340
#define CH_IMGB (43 * 1024)      // 2720 slots of 16 bytes, rounded up to whole 1 KiB DMA pieces
#define CH_NIMG 6                // image DMA instructions per lane and stage (43 pieces / 8 waves)

// ReLU that keeps NaN (fmaxf would return 0)
__device__ __forceinline__ float ch_relu(float v) { return v < 0.0f ? 0.0f : v; }

struct ConvHArgs {
    const _Float16* Wp;            // [S][9 taps][Co / 16][2 k-steps][64 lanes][8 halves], see irm_hip.h
    const _Float16* X; long x_bs;  // [B][H][W][Ci]
    _Float16* Y; long y_bs;        // [B][H][W][Co]
    const _Float16* R; long r_bs;  // [B][H][W][Co] or null
    const float* bias;
    int Ci, Co, H, W, S, mtiles;
    int relu1, res_mode, relu2, tiles_x;
    float inv_s;                   // 1 / weight scale
};

template <int CT>
__global__ __launch_bounds__(512, 2) void conv3x3_h_kernel(ConvHArgs a) {
    constexpr int WGB = CT * 2048;                 // bytes of the weights of one (stage, tap): CT tiles x 2 k-steps x 1 KiB
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* lds = reinterpret_cast<char*>(smem);
    const int S = a.S;
    char* img = lds;                               // [S][CH_IMGB]
    char* wbuf = lds + S * CH_IMGB;                // [2][WGB]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, r = lane & 15;
    const int b = blockIdx.z;
    const int ty0 = (blockIdx.x / a.tiles_x) * CH_TH, tx0 = (blockIdx.x % a.tiles_x) * CH_TW;
    const int mt0 = blockIdx.y * CT;
    const _Float16* X = a.X + (long)b * a.x_bs;
    const _Float16* const zero_page = reinterpret_cast<const _Float16*>(irm_zero_page);

    // ---- the halo tile of every stage: slot q = j * 512 + tid -> (halo pixel, swizzled chunk)
#pragma unroll
    for (int j = 0; j < CH_NIMG; ++j) {
        if (j * 8 + wave >= CH_IMGB / 1024) break;                         // (wave-uniform: 43 pieces)
        const int q = j * 512 + tid;
        const int pi = q >> 3, c = (q & 7) ^ (((pi >> 1) & 3) << 1);
        const int row = pi / CH_HC, col = pi - row * CH_HC;
        const int gy = ty0 - 1 + row, gx = tx0 - 1 + col;
        const bool ok = pi < CH_NP && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        const long off = ((long)gy * a.W + gx) * a.Ci + 8 * c;
        for (int s = 0; s < S; ++s) {
            const _Float16* src = ok ? X + off + 64 * s : zero_page;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                             (__attribute__((address_space(3))) void*)(img + s * CH_IMGB + (j * 512 + wave * 64) * 16),
                                             16, 0, 0);
        }
    }
    // weight group n = 9 s + tap -> buffer n & 1 (piece pc of 1 KiB by wave pc % 8)
    auto issue_w = [&](int n) {
#pragma unroll
        for (int i = 0; i < (2 * CT + 7) / 8; ++i) {
            const int pc = wave + 8 * i;
            if (pc < 2 * CT) {
                const _Float16* src = a.Wp + ((long)n * a.mtiles + mt0) * 1024 + pc * 512 + lane * 8;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                                 (__attribute__((address_space(3))) void*)(wbuf + (n & 1) * WGB + pc * 1024), 16, 0, 0);
            }
        }
    };
    issue_w(0);

    f32x4 acc[2][CT];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[p][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int s = 0; s < S; ++s) {
        const char* im = img + s * CH_IMGB;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int n = 9 * s + tap, dy = tap / 3, dx = tap - 3 * dy;
            irm_wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();          // group n (and the image) landed; everybody is done with group n - 1
            if (n + 1 < 9 * S) issue_w(n + 1);
            const char* wb = wbuf + (n & 1) * WGB;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                irm_h8 px[2];
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const int pi = (wave + dy) * CH_HC + 16 * p + r + dx;
                    const int c = (4 * ks + g) ^ (((pi >> 1) & 3) << 1);
                    px[p] = *reinterpret_cast<const irm_h8*>(im + (pi * 8 + c) * 16);
                }
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const irm_h8 w = *reinterpret_cast<const irm_h8*>(wb + (c * 2 + ks) * 1024 + lane * 16);
#pragma unroll
                    for (int p = 0; p < 2; ++p) acc[p][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, px[p], acc[p][c], 0, 0, 0);
                }
            }
        }
    }

    // ---- epilogue: lane (g, r) holds channels 16 (mt0 + c) + 4 g + e of pixel (ty0 + wave, tx0 + 16 p + r)
    const int y = ty0 + wave;
    if (y >= a.H) return;
    _Float16* Y = a.Y + (long)b * a.y_bs;
    const _Float16* R = a.res_mode ? a.R + (long)b * a.r_bs : nullptr;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int x = tx0 + 16 * p + r;
        if (x >= a.W) continue;
        const long pix = ((long)y * a.W + x) * a.Co;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int co = (mt0 + c) * 16 + 4 * g;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = fmaf(acc[p][c][e], a.inv_s, a.bias ? a.bias[co + e] : 0.0f);
                if (a.relu1) v[e] = ch_relu(v[e]);
            }
            if (R) {
                const irm_h4 rr = *reinterpret_cast<const irm_h4*>(R + pix + co);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += (float)rr[e];
            }
            irm_h4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (_Float16)(a.relu2 ? ch_relu(v[e]) : v[e]);
            *reinterpret_cast<irm_h4*>(Y + pix + co) = o;
        }
    }
}

template <int CT>
static int launch_conv_h(const ConvHArgs& a, int B, hipStream_t stream) {
    const size_t lds = (size_t)a.S * CH_IMGB + 2 * (CT * 2048);
    static_assert((size_t)2 * CH_IMGB + 2 * (CT * 2048) <= 160 * 1024, "LDS");
    IRM_ALLOW_BIG_LDS((&conv3x3_h_kernel<CT>));
    const int tiles_y = (a.H + CH_TH - 1) / CH_TH;
    dim3 grid(a.tiles_x * tiles_y, a.mtiles / CT, B);
    hipLaunchKernelGGL((conv3x3_h_kernel<CT>), grid, dim3(512), lds, stream, a);
    return irm_launch_status();
}

extern "C" int irm_conv3x3_h_f16(const void* wp, float inv_scale, const void* x, long x_bs, void* y, long y_bs,
                                 const void* res, long r_bs, const float* bias, int B, int Ci, int Co, int H, int W,
                                 int relu1, int res_mode, int relu2, hipStream_t stream) {
    if (!wp || !x || !y || B <= 0 || H <= 0 || W <= 0 || B > 65535) return IRM_EINVAL;
    if ((Ci != 64 && Ci != 128) || (Co != 64 && Co != 128)) return IRM_EINVAL;
    if (res_mode < 0 || res_mode > 1 || (res_mode && !res)) return IRM_EINVAL;
    if ((x_bs & 7) || (y_bs & 7) || (r_bs & 7)) return IRM_EINVAL;
    if (!irm_aligned16(wp) || !irm_aligned16(x) || !irm_aligned16(y) || !irm_aligned16(res)) return IRM_EINVAL;
    const long tiles = (long)((W + CH_TW - 1) / CH_TW) * ((H + CH_TH - 1) / CH_TH);
    if (tiles > 0x7fffffffL) return IRM_EINVAL;
    ConvHArgs a;
    a.Wp = static_cast<const _Float16*>(wp); a.X = static_cast<const _Float16*>(x); a.x_bs = x_bs;
    a.Y = static_cast<_Float16*>(y); a.y_bs = y_bs; a.R = static_cast<const _Float16*>(res); a.r_bs = r_bs; a.bias = bias;
    a.Ci = Ci; a.Co = Co; a.H = H; a.W = W; a.S = Ci / 64; a.mtiles = Co / 16;
    a.relu1 = relu1; a.res_mode = res_mode; a.relu2 = relu2; a.tiles_x = (W + CH_TW - 1) / CH_TW; a.inv_s = inv_scale;
    // all output tiles of a pixel tile in one workgroup (the input tile is fetched once) unless the launch is small:
    // then 64 channels per workgroup, twice as many workgroups
    if (Co == 128 && tiles * B >= 256) return launch_conv_h<8>(a, B, stream);
    return launch_conv_h<4>(a, B, stream);
}

// ---- in: work item = one pixel x 8 consecutive output channels (one 16-byte store); the weights lie transposed in LDS
// ([Ci 9 taps][Co]: the 8 channels of an item are two 16-byte reads per tap).
struct ConvHInArgs {
    const float* w;                // [Co][Ci][3][3]
    const float* x; long x_bs;     // [B][Ci][H][W]
    _Float16* y; long y_bs;        // [B][H][W][Co]
    const float* bias;
    int Ci, Co, H, W, relu1;
};

__global__ __launch_bounds__(256) void conv3x3_h_in_kernel(ConvHInArgs a) {
    __shared__ __attribute__((aligned(16))) float wl[27 * 128];
    const int nt = a.Ci * 9;
    for (int i = threadIdx.x; i < a.Co * nt; i += 256) {
        const int co = i / nt, t = i - co * nt;
        wl[t * a.Co + co] = a.w[i];
    }
    __syncthreads();
    const int nch = a.Co >> 3;
    const long item = (long)blockIdx.x * 256 + threadIdx.x;
    const long plane = (long)a.H * a.W;
    if (item >= plane * nch) return;
    const long pix = item / nch;
    const int ch = (int)(item - pix * nch) * 8;
    const int y = (int)(pix / a.W), x = (int)(pix - (long)y * a.W);
    const float* xb = a.x + (long)blockIdx.y * a.x_bs;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = a.bias ? a.bias[ch + e] : 0.0f;
    for (int ci = 0; ci < a.Ci; ++ci) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int gy = y + tap / 3 - 1, gx = x + tap % 3 - 1;
            const bool ok = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            const float xv = ok ? xb[(long)ci * plane + (long)gy * a.W + gx] : 0.0f;
            const float* wr = wl + (ci * 9 + tap) * a.Co + ch;
            const float4 w0 = *reinterpret_cast<const float4*>(wr), w1 = *reinterpret_cast<const float4*>(wr + 4);
            v[0] = fmaf(w0.x, xv, v[0]); v[1] = fmaf(w0.y, xv, v[1]); v[2] = fmaf(w0.z, xv, v[2]); v[3] = fmaf(w0.w, xv, v[3]);
            v[4] = fmaf(w1.x, xv, v[4]); v[5] = fmaf(w1.y, xv, v[5]); v[6] = fmaf(w1.z, xv, v[6]); v[7] = fmaf(w1.w, xv, v[7]);
        }
    }
    irm_h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (_Float16)(a.relu1 ? ch_relu(v[e]) : v[e]);
    *reinterpret_cast<irm_h8*>(a.y + (long)blockIdx.y * a.y_bs + pix * a.Co + ch) = o;
}

extern "C" int irm_conv3x3_h_in_f32(const float* w, const float* x, long x_bs, void* y, long y_bs, const float* bias, int B,
                                    int Ci, int Co, int H, int W, int relu1, hipStream_t stream) {
    if (!w || !x || !y || B <= 0 || Ci <= 0 || Ci > 3 || H <= 0 || W <= 0 || B > 65535) return IRM_EINVAL;
    if ((Co != 64 && Co != 128) || (y_bs & 7) || !irm_aligned16(y)) return IRM_EINVAL;
    const long blocks = ((long)H * W * (Co / 8) + 255) / 256;
    if (blocks > 0x7fffffffL) return IRM_EINVAL;
    ConvHInArgs a{w, x, x_bs, static_cast<_Float16*>(y), y_bs, bias, Ci, Co, H, W, relu1};
    hipLaunchKernelGGL(conv3x3_h_in_kernel, dim3((unsigned)blocks, B), dim3(256), 0, stream, a);
    return irm_launch_status();
}

// ---- out: 8 lanes share a pixel, lane q of them sums the 16-byte channel chunks q, q + 8 of the 9 taps (the 8 lanes
// read one 128-byte line); the partial sums meet by three xor-shuffles (a fixed order: bitwise reproducible) and the
// first lane applies the epilogue.  Weights in LDS as [Co][9 taps][Ci]: a lane's 8 channels are two 16-byte reads, the
// pixels of a wave read the same addresses (broadcast).
struct ConvHOutArgs {
    const float* w;                // [Co][Ci][3][3]
    const _Float16* x; long x_bs;  // [B][H][W][Ci]
    float* y; long y_bs;           // [B][Co][H][W]
    const float* res; long r_bs;   // [B][Co][H][W] or null
    const float* bias;
    int Ci, Co, H, W, res_mode;
};

template <int CO>
__global__ __launch_bounds__(256) void conv3x3_h_out_kernel(ConvHOutArgs a) {
    __shared__ __attribute__((aligned(16))) float wl[CO * 9 * 128];
    for (int i = threadIdx.x; i < CO * 9 * a.Ci; i += 256) {
        const int co = i / (9 * a.Ci), rem = i - co * 9 * a.Ci, tap = rem / a.Ci, ci = rem - tap * a.Ci;
        wl[i] = a.w[((long)co * a.Ci + ci) * 9 + tap];
    }
    __syncthreads();
    const int q = threadIdx.x & 7;
    const long plane = (long)a.H * a.W;
    const long pix = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool live = pix < plane;
    const int y = live ? (int)(pix / a.W) : 0, x = live ? (int)(pix - (long)y * a.W) : 0;
    const _Float16* xb = a.x + (long)blockIdx.y * a.x_bs;
    float acc[CO];
#pragma unroll
    for (int c = 0; c < CO; ++c) acc[c] = 0.0f;
    for (int ch = 8 * q; ch < a.Ci; ch += 64) {
#pragma unroll 1
        for (int tap = 0; tap < 9; ++tap) {
            const int gy = y + tap / 3 - 1, gx = x + tap % 3 - 1;
            const bool ok = live && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            irm_h8 xv = {0, 0, 0, 0, 0, 0, 0, 0};
            if (ok) xv = *reinterpret_cast<const irm_h8*>(xb + ((long)gy * a.W + gx) * a.Ci + ch);
#pragma unroll
            for (int c = 0; c < CO; ++c) {
                const float* wr = wl + (c * 9 + tap) * a.Ci + ch;
                const float4 w0 = *reinterpret_cast<const float4*>(wr), w1 = *reinterpret_cast<const float4*>(wr + 4);
                float s = acc[c];
                s = fmaf(w0.x, (float)xv[0], s); s = fmaf(w0.y, (float)xv[1], s); s = fmaf(w0.z, (float)xv[2], s);
                s = fmaf(w0.w, (float)xv[3], s); s = fmaf(w1.x, (float)xv[4], s); s = fmaf(w1.y, (float)xv[5], s);
                s = fmaf(w1.z, (float)xv[6], s); s = fmaf(w1.w, (float)xv[7], s);
                acc[c] = s;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < CO; ++c) {
        acc[c] += __shfl_xor(acc[c], 1);
        acc[c] += __shfl_xor(acc[c], 2);
        acc[c] += __shfl_xor(acc[c], 4);
    }
    if (!live || q != 0) return;
    float* yb = a.y + (long)blockIdx.y * a.y_bs;
    const float* rb = a.res_mode ? a.res + (long)blockIdx.y * a.r_bs : nullptr;
#pragma unroll
    for (int c = 0; c < CO; ++c) {
        float v = acc[c] + (a.bias ? a.bias[c] : 0.0f);
        if (a.res_mode == 1) v += rb[c * plane + pix];
        else if (a.res_mode == 2) v = rb[c * plane + pix] - v;
        yb[c * plane + pix] = v;
    }
}

extern "C" int irm_conv3x3_h_out_f32(const float* w, const void* x, long x_bs, float* y, long y_bs, const float* res,
                                     long r_bs, const float* bias, int B, int Ci, int Co, int H, int W, int res_mode,
                                     hipStream_t stream) {
    if (!w || !x || !y || B <= 0 || Co <= 0 || Co > 3 || H <= 0 || W <= 0 || B > 65535) return IRM_EINVAL;
    if ((Ci != 64 && Ci != 128) || (x_bs & 7) || !irm_aligned16(x)) return IRM_EINVAL;
    if (res_mode < 0 || res_mode > 2 || (res_mode && !res)) return IRM_EINVAL;
    const long blocks = ((long)H * W + 31) / 32;
    if (blocks > 0x7fffffffL) return IRM_EINVAL;
    ConvHOutArgs a{w, static_cast<const _Float16*>(x), x_bs, y, y_bs, res, r_bs, bias, Ci, Co, H, W, res_mode};
    const dim3 grid((unsigned)blocks, B);
    if (Co == 1) hipLaunchKernelGGL(conv3x3_h_out_kernel<1>, grid, dim3(256), 0, stream, a);
    else if (Co == 2) hipLaunchKernelGGL(conv3x3_h_out_kernel<2>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(conv3x3_h_out_kernel<3>, grid, dim3(256), 0, stream, a);
    return irm_launch_status();
}
