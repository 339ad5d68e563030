// Dense K_h x K_w convolution with stride and zero padding as an implicit GEMM on the exact-f32 MFMA, planar NCHW:
// the geometries of the Inception-ResNet-v2 encoder of DeblurGANv2's FPN-Inception generator that the 3x3 pad-1 family
// (conv3x3.hip) does not cover - 3x3 stride 2 pad 0 (conv2d_1a, mixed_6a, mixed_7a), 3x3 stride 1 pad 0 (conv2d_2a,
// conv2d_4a), 5x5 pad 2 (mixed_5b), 1x7 pad (0,3) and 7x1 pad (3,0) (Block17) - and the 1x1 "block closer"
// relu(x + s (W cat + b)) of Block35 / Block17, which needs the residual BEFORE the ReLU (s is folded into W and b when
// they are packed).
//
// Mapping (conv3x3.hip's guarded kernel, generalised): one 256-thread workgroup = an 8 x 32 tile of OUTPUT pixels.  Its
// input halo tile, ((8 - 1) S + KH) x ((32 - 1) S + KW) pixels of 4 KS input channels, is staged through
// double-buffered LDS from guarded loads (out-of-image taps and channels beyond Ci read 0: that is the zero padding).
// Each wave owns 4 pixel groups of 16 consecutive output columns (2 rows x 2 halves) and CT output-channel tiles; for
// every tap (dy, dx) and k-step the A operand is the LDS tile at (S y + dy, S x + dx), the B operand the packed weight
//   Wp[tap][mtile][kstep][lane] = W[16 mtile + (lane & 15)][4 kstep + (lane >> 4)][tap / KW][tap % KW],
// staged through LDS as well.  One MFMA per tap, k-step, pixel group and output tile.
//
// LDS (floats): 2 x (4 KS PLANE) input + 2 x (KH KW CT KS 64) weights; a half-wave of an A read covers 16 columns of
// 2 channel planes, so PLANE = 16 mod 32 at stride 1 and odd at stride 2 (columns 2 apart fill the even banks) keeps
// ds_read_b32 conflict free.  Per geometry, at the largest CT:
//   1x1  KS 4  PLANE  272   34.0 + 8.0  KiB      3x3 s1  KS 2  PLANE  368   23.0 + 36.0 KiB
//   1x7  KS 2  PLANE  304   19.0 + 28.0 KiB      7x1     KS 2  PLANE  464   29.0 + 28.0 KiB
//   5x5  KS 1  PLANE  432   13.5 + 25.0 KiB (CT <= 2)          3x3 s2  KS 1  PLANE 1105   34.5 + 18.0 KiB
// all below 64 KiB, so at least two workgroups share a CU's 160 KiB.
#include "conv_epilogue.h"

#define CK_TH 8
#define CK_TW IRM_CONV_TW

struct ConvKArgs {
    const float* Wp;              // packed [KH*KW][mtiles][ksteps][64]
    const float* X; long x_bs;    // [B][Ci][IH][IW]
    float* Y; long y_bs;          // [B][Co][H][W]
    const float* R; long r_bs;    // residual [B][Co][H][W] or null
    const float* bias;            // [Co] or null
    int Ci, Co, H, W;             // H, W: the OUTPUT size (irm_conv_store addresses the output with them)
    int IH, IW;                   // the input size
    int pad_h, pad_w;
    int mtiles, ksteps;           // ceil(Co/16), ceil(Ci/4)
    int relu1;                    // after the bias: 0 none, 1 ReLU
    float slope;                  // (the family's LeakyReLU slope: unused, relu1 < 2)
    int ps_r;                     // (the family's PixelShuffle factor: unused, store_mode 0)
    int res_mode;                 // 0 none, 1: v += R
    int relu2;                    // relu after the residual
    int store_mode;               // 0 NCHW
    int tiles_x;
    int vec;                      // 16-byte stores are legal
};

template <int KH, int KW, int S>
struct ConvKGeom {
    static constexpr int T = KH * KW;
    static constexpr int ROWS = (CK_TH - 1) * S + KH, COLS = (CK_TW - 1) * S + KW;
    static constexpr int plane() {
        int p = ROWS * COLS;
        if (S == 1) { while (p % 32 != 16) ++p; }
        else if (p % 2 == 0) ++p;
        return p;
    }
    static constexpr int PLANE = plane();
    // k-steps (4 input channels each) per stage and the largest CT, from the LDS budget above
    static constexpr int KS = T == 1 ? 4 : (S == 1 && T <= 9) ? 2 : 1;
    static constexpr int MAXCT = T > 9 ? 2 : 4;
};

template <int KH, int KW, int S, int CT>
__global__ __launch_bounds__(256) void convkxk_kernel(ConvKArgs a) {
    using G = ConvKGeom<KH, KW, S>;
    constexpr int T = G::T, ROWS = G::ROWS, COLS = G::COLS, PLANE = G::PLANE, KS = G::KS;
    constexpr int CK = 4 * KS;                         // input channels per stage
    constexpr int XST = CK * ROWS * COLS;              // halo elements per stage
    constexpr int WST = T * CT * KS * 64;              // packed weights per stage
    static_assert((2 * CK * PLANE + 2 * WST) * 4 <= 64 * 1024, "LDS budget");
    __shared__ float xs[2][CK * PLANE];
    __shared__ float wsm[2][WST];
    constexpr int NLOAD = (XST + 255) / 256;
    constexpr int WLOAD = (WST + 255) / 256;
    float xr[NLOAD], wr[WLOAD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z;
    const int ty0 = (blockIdx.x / a.tiles_x) * CK_TH;
    const int tx0 = (blockIdx.x % a.tiles_x) * CK_TW;
    const float* X = a.X + (long)b * a.x_bs;
    const long iplane = (long)a.IH * a.IW;
    const long plane = (long)a.H * a.W;
    const int iy0 = ty0 * S - a.pad_h, ix0 = tx0 * S - a.pad_w;

    auto load_stage = [&](int s) {
#pragma unroll
        for (int j = 0; j < NLOAD; ++j) {
            const int e = tid + j * 256;
            float v = 0.0f;
            if (e < XST) {
                const int ch = e / (ROWS * COLS);
                const int rem = e % (ROWS * COLS);
                const int yy = rem / COLS, xx = rem % COLS;
                const int ci = s * CK + ch, gy = iy0 + yy, gx = ix0 + xx;
                if (ci < a.Ci && gy >= 0 && gy < a.IH && gx >= 0 && gx < a.IW)
                    v = X[(long)ci * iplane + (long)gy * a.IW + gx];
            }
            xr[j] = v;
        }
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int j = 0; j < NLOAD; ++j) {
            const int e = tid + j * 256;
            if (e < XST) {
                const int ch = e / (ROWS * COLS);
                const int rem = e % (ROWS * COLS);
                xs[buf][ch * PLANE + rem] = xr[j];
            }
        }
    };

    const int g = lane >> 4, r = lane & 15;
    const int nstages = (a.ksteps + KS - 1) / KS;
    const int nchunks = (a.mtiles + CT - 1) / CT;

    for (int chunk = blockIdx.y; chunk < nchunks; chunk += gridDim.y) {
        const int mt0 = chunk * CT;
        const int nct = min(CT, a.mtiles - mt0);
        auto load_w = [&](int s) {
#pragma unroll
            for (int j = 0; j < WLOAD; ++j) {
                const int e = tid + j * 256;                   // ((tap * CT + c) * KS + kk) * 64 + lane
                float v = 0.0f;
                if (e < WST) {
                    const int ln = e & 63, q = e >> 6, kk = q % KS, tc = q / KS, c = tc % CT, tap = tc / CT;
                    const int ks = s * KS + kk;
                    if (c < nct && ks < a.ksteps) v = a.Wp[(((long)tap * a.mtiles + mt0 + c) * a.ksteps + ks) * 64 + ln];
                }
                wr[j] = v;
            }
        };
        auto store_w = [&](int buf) {
#pragma unroll
            for (int j = 0; j < WLOAD; ++j) {
                const int e = tid + j * 256;
                if (e < WST) wsm[buf][e] = wr[j];
            }
        };
        f32x4 acc[4][CT];
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int c = 0; c < CT; ++c) acc[p][c] = (f32x4){0.f, 0.f, 0.f, 0.f};

        __syncthreads();                      // the previous chunk is done with both buffers
        load_stage(0);
        load_w(0);
        store_stage(0);
        store_w(0);
        __syncthreads();
        for (int s = 0; s < nstages; ++s) {
            const int buf = s & 1;
            if (s + 1 < nstages) { load_stage(s + 1); load_w(s + 1); }
#pragma unroll
            for (int tap = 0; tap < T; ++tap) {
                const int dy = tap / KW, dx = tap % KW;
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) {
                    float bf[CT], af[4];
#pragma unroll
                    for (int c = 0; c < CT; ++c) bf[c] = wsm[buf][((tap * CT + c) * KS + kk) * 64 + lane];
#pragma unroll
                    for (int p = 0; p < 4; ++p) {
                        const int yy = (wave * 2 + (p >> 1)) * S + dy;
                        const int xx = ((p & 1) * 16 + r) * S + dx;
                        af[p] = xs[buf][(kk * 4 + g) * PLANE + yy * COLS + xx];
                    }
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        if (c < nct) {
#pragma unroll
                            for (int p = 0; p < 4; ++p) acc[p][c] = irm_mfma16(af[p], bf[c], acc[p][c]);
                        }
                    }
                }
            }
            if (s + 1 < nstages) { store_stage(buf ^ 1); store_w(buf ^ 1); }
            __syncthreads();
        }

        // epilogue: lane holds output pixels (y, x..x+3) of channel co
        float* Y = a.Y + (long)b * a.y_bs;
        const float* R = a.R ? a.R + (long)b * a.r_bs : nullptr;
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int co = (mt0 + c) * 16 + r;
            if (c < nct && co < a.Co) {
                const float bv = a.bias ? a.bias[co] : 0.0f;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int y = ty0 + wave * 2 + (p >> 1);
                    const int x = tx0 + (p & 1) * 16 + g * 4;
                    if (y >= a.H || x >= a.W) continue;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = irm_conv_act1(acc[p][c][e] + bv, a);
                    irm_conv_store<true>(v, co, y, x, plane, Y, R, a, a.vec);
                }
            }
        }
    }
}

template <int KH, int KW, int S, int CT>
static int launch_convk(const ConvKArgs& a, int B, int ygroups, hipStream_t stream) {
    const int tiles_y = (a.H + CK_TH - 1) / CK_TH;
    dim3 grid(a.tiles_x * tiles_y, ygroups, B);
    hipLaunchKernelGGL((convkxk_kernel<KH, KW, S, CT>), grid, dim3(256), 0, stream, a);
    return irm_launch_status();
}

template <int KH, int KW, int S>
static int launch_convk_ct(const ConvKArgs& a, int B, int ct, int ygroups, hipStream_t stream) {
    if (ct > ConvKGeom<KH, KW, S>::MAXCT) return IRM_EINVAL;
    switch (ct) {
        case 1: return launch_convk<KH, KW, S, 1>(a, B, ygroups, stream);
        case 2: return launch_convk<KH, KW, S, 2>(a, B, ygroups, stream);
        case 4:
            if constexpr (ConvKGeom<KH, KW, S>::MAXCT >= 4) return launch_convk<KH, KW, S, 4>(a, B, ygroups, stream);
            return IRM_EINVAL;
        default: return IRM_EINVAL;
    }
}

extern "C" int irm_convkxk_f32(const float* wp, const float* x, long x_bs, float* y, long y_bs, const float* res,
                               long r_bs, const float* bias, int B, int Ci, int Co, int H, int W, int kh, int kw,
                               int stride, int pad_h, int pad_w, int act1, int res_mode, int relu2, int ct, int ygroups,
                               hipStream_t stream) {
    if (!wp || !x || !y || B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) return IRM_EINVAL;
    if (kh <= 0 || kw <= 0 || stride <= 0 || pad_h < 0 || pad_w < 0 || pad_h >= kh || pad_w >= kw) return IRM_EINVAL;
    if (act1 < 0 || act1 > 1 || res_mode < 0 || res_mode > 1 || (res_mode && !res)) return IRM_EINVAL;
    if (B > 65535 || ct <= 0) return IRM_EINVAL;
    if (H + 2 * pad_h < kh || W + 2 * pad_w < kw) return IRM_EINVAL;          // no output pixel
    ConvKArgs a;
    a.Wp = wp; a.X = x; a.x_bs = x_bs; a.Y = y; a.y_bs = y_bs; a.R = res; a.r_bs = r_bs; a.bias = bias;
    a.Ci = Ci; a.Co = Co; a.IH = H; a.IW = W;
    a.H = (H + 2 * pad_h - kh) / stride + 1;
    a.W = (W + 2 * pad_w - kw) / stride + 1;
    a.pad_h = pad_h; a.pad_w = pad_w;
    a.mtiles = (Co + 15) / 16; a.ksteps = (Ci + 3) / 4;
    a.relu1 = act1; a.slope = 0.0f; a.ps_r = 2; a.res_mode = res_mode; a.relu2 = relu2 ? 1 : 0; a.store_mode = 0;
    a.tiles_x = (a.W + CK_TW - 1) / CK_TW;
    a.vec = !(a.W & 3) && !(y_bs & 3) && !(r_bs & 3) && irm_aligned16(y) && irm_aligned16(res);
    const int nchunks = (a.mtiles + ct - 1) / ct;
    if (ygroups <= 0) ygroups = 1;
    if (ygroups > nchunks) ygroups = nchunks;
    if (kh == 1 && kw == 1 && stride == 1) return launch_convk_ct<1, 1, 1>(a, B, ct, ygroups, stream);
    if (kh == 3 && kw == 3 && stride == 1) return launch_convk_ct<3, 3, 1>(a, B, ct, ygroups, stream);
    if (kh == 3 && kw == 3 && stride == 2) return launch_convk_ct<3, 3, 2>(a, B, ct, ygroups, stream);
    if (kh == 5 && kw == 5 && stride == 1) return launch_convk_ct<5, 5, 1>(a, B, ct, ygroups, stream);
    if (kh == 1 && kw == 7 && stride == 1) return launch_convk_ct<1, 7, 1>(a, B, ct, ygroups, stream);
    if (kh == 7 && kw == 1 && stride == 1) return launch_convk_ct<7, 1, 1>(a, B, ct, ygroups, stream);
    return IRM_EINVAL;                                                         // a geometry that is not built
}
