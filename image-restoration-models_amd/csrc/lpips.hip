// LPIPS v0.1 (net = 'alex') around the conv trunk (include/irm_hip_lpips.h):
//   irm_lpips_pack   K HWC frames (uint8, uint16 or float32, read where they lie) -> z [K][48][OH + 2][OW + 2] float32: the
//                    scaled frame, zero padded by 2, space-to-depth by 4, so that AlexNet's 11 x 11 stride-4 pad-2 conv is a
//                    3 x 3 stride-1 pad-0 conv over 48 channels (irm_convkxk_f32);
//   irm_lpips_head   one tap's distance of K pairs of feature maps: unit-normalise over the channels, weighted squared
//                    difference, mean over the pixels.
// Both are memory streams; neither has matrix work.
//
// lp_pack_kernel: a thread owns one position (Y, X) of z and one of the four source rows i that fold into it.  It reads
// the 12 samples of the source pixels 4X - 2 .. 4X + 1 of row 4Y + i - 2 - consecutive lanes read consecutive 12-sample
// runs, a wave one contiguous run - and stores them to the 12 planes c * 16 + i * 4 + j, every store 64 consecutive
// floats of one plane row.  A sample outside the reached part of the frame is not read and its position gets a literal
// 0: the conv's twelfth tap (weight 0) multiplies it, and a row or column that the stride never reaches may hold anything.
//
// lp_head_kernel: a workgroup owns 64 consecutive pixels of one pair, lanes along the pixels (planar maps: every load is
// 64 consecutive floats of one channel plane), its four waves a quarter of the channels each.  Pass 1 sums the squares of
// the two maps over the wave's channels, the four partial sums meet in LDS and every thread adds them in the same
// order; pass 2 forms the direct difference f_c r_f - g_c r_g, r = 1 / (n + eps), in float32 - identical maps give
// exactly 0 - squares and weights it.  Every sum runs in float64.  One partial per workgroup goes to the workspace;
// lp_fold_kernel adds a pair's partials in a fixed order and divides by the pixel count.  No atomics.
#include "irm_frame.h"

#define LP_EPS 1e-10f
#define LP_MAX_C 4096

struct LpPack {
    const void* frames;
    long pitch, frame_stride;          // in samples
    int Hr, Wr;                        // rows and columns of the frame that the stride reaches
    int ZH, ZW;                        // OH + 2, OW + 2
    float a[3], b[3];                  // u = fma(raw, a[c], b[c])
    float* z;
    long z_bs;
};

template <typename T>
__global__ __launch_bounds__(256) void lp_pack_kernel(LpPack g) {
    const int X = blockIdx.x * 64 + (threadIdx.x & 63), i = threadIdx.x >> 6, Y = blockIdx.y, k = blockIdx.z;
    if (X >= g.ZW) return;
    const int row = 4 * Y + i - 2, col0 = 4 * X - 2;
    const bool row_in = row >= 0 && row < g.Hr;
    const T* src = reinterpret_cast<const T*>(g.frames) + (long)k * g.frame_stride + (row_in ? (long)row * g.pitch : 0L);
    const long plane = (long)g.ZH * g.ZW;
    float* dst = g.z + (long)k * g.z_bs + (long)(i * 4) * plane + (long)Y * g.ZW + X;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + j;
        const bool in = row_in && col >= 0 && col < g.Wr;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float raw = (float)src[in ? (long)col * 3 + c : 0L];
            dst[(long)(c * 16 + j) * plane] = in ? __fmaf_rn(raw, g.a[c], g.b[c]) : 0.0f;
        }
    }
}

struct LpHead {
    const float* f;
    long f_bs;
    const float* lin;
    int K, C, N;                       // pairs, channels, pixels of a map
    int nblk;                          // workgroups (partials) per pair
    double* part;
};

__global__ __launch_bounds__(256) void lp_head_kernel(LpHead g) {
    __shared__ double ss[2][4][64];
    __shared__ double part[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, k = blockIdx.y;
    const int n = blockIdx.x * 64 + lane;
    const bool valid = n < g.N;
    const long N = g.N;
    const float* f = g.f + (long)k * g.f_bs + (valid ? n : 0);
    const float* h = g.f + (long)(k + g.K) * g.f_bs + (valid ? n : 0);

    double sf = 0.0, sg = 0.0;
    for (int c = wave; c < g.C; c += 4) {
        const double a = (double)f[c * N], b = (double)h[c * N];
        sf = fma(a, a, sf);
        sg = fma(b, b, sg);
    }
    ss[0][wave][lane] = sf;
    ss[1][wave][lane] = sg;
    __syncthreads();
    const float nf = (float)sqrt(((ss[0][0][lane] + ss[0][1][lane]) + ss[0][2][lane]) + ss[0][3][lane]);
    const float ng = (float)sqrt(((ss[1][0][lane] + ss[1][1][lane]) + ss[1][2][lane]) + ss[1][3][lane]);
    const float rf = __fdiv_rn(1.0f, __fadd_rn(nf, LP_EPS)), rg = __fdiv_rn(1.0f, __fadd_rn(ng, LP_EPS));

    double acc = 0.0;
    for (int c = wave; c < g.C; c += 4) {
        const float d = __fsub_rn(__fmul_rn(f[c * N], rf), __fmul_rn(h[c * N], rg));
        acc += (double)__fmul_rn(g.lin[c], __fmul_rn(d, d));
    }
    acc = irm_block_reduce256<FrSum>(valid ? acc : 0.0, part);
    if (t == 0) g.part[(long)k * g.nblk + blockIdx.x] = acc;
}

// One workgroup per pair: its partials in a fixed order, then the mean over the pixels.
__global__ __launch_bounds__(256) void lp_fold_kernel(const double* part, int nblk, double count, double* out,
                                                      long out_stride) {
    __shared__ double dpart[4];
    const long base = (long)blockIdx.x * nblk;
    double s = 0.0;
    for (int j = threadIdx.x; j < nblk; j += 256) s += part[base + j];
    s = irm_block_reduce256<FrSum>(s, dpart);
    if (threadIdx.x == 0) out[(long)blockIdx.x * out_stride] = s / count;
}

extern "C" int irm_lpips_pack(const void* frames, int kind, int K, int H, int W, long pitch, long frame_stride, float a0,
                              float a1, float a2, float b0, float b1, float b2, float* z, long z_bs,
                              hipStream_t stream) {
    if (!frames || !z) return IRM_EINVAL;
    if (kind < 0 || kind > 2 || K <= 0 || K > 65535 || H < 7 || W < 7 || (long)H * W * 3 > 0x7fffffffL) return IRM_EINVAL;
    const long rowv = (long)W * 3;
    if (pitch < rowv || frame_stride < (long)(H - 1) * pitch + rowv) return IRM_EINVAL;
    const uintptr_t es = kind == 0 ? 1 : kind == 1 ? 2 : 4;
    if ((reinterpret_cast<uintptr_t>(frames) & (es - 1)) || (reinterpret_cast<uintptr_t>(z) & 3)) return IRM_EINVAL;
    const int OH = (H - 7) / 4 + 1, OW = (W - 7) / 4 + 1;
    if (OH + 2 > 65535 || z_bs < 48L * (OH + 2) * (OW + 2)) return IRM_EINVAL;
    LpPack g;
    g.frames = frames;
    g.pitch = pitch;
    g.frame_stride = frame_stride;
    g.Hr = min(H, 4 * OH + 5);          // the last window ends at row 4 (OH - 1) - 2 + 10
    g.Wr = min(W, 4 * OW + 5);
    g.ZH = OH + 2;
    g.ZW = OW + 2;
    g.a[0] = a0; g.a[1] = a1; g.a[2] = a2;
    g.b[0] = b0; g.b[1] = b1; g.b[2] = b2;
    g.z = z;
    g.z_bs = z_bs;
    const dim3 grid((unsigned)((g.ZW + 63) / 64), (unsigned)g.ZH, (unsigned)K);
    if (kind == 0) hipLaunchKernelGGL(lp_pack_kernel<unsigned char>, grid, dim3(256), 0, stream, g);
    else if (kind == 1) hipLaunchKernelGGL(lp_pack_kernel<unsigned short>, grid, dim3(256), 0, stream, g);
    else hipLaunchKernelGGL(lp_pack_kernel<float>, grid, dim3(256), 0, stream, g);
    return irm_launch_status();
}

extern "C" int irm_lpips_head(const float* f, long f_bs, const float* lin, int K, int C, int H, int W, double* out,
                              long out_stride, void* ws, long ws_words, hipStream_t stream) {
    if (!f || !lin || !out || !ws) return IRM_EINVAL;
    if (K <= 0 || K > 65535 || C <= 0 || C > LP_MAX_C || H <= 0 || W <= 0) return IRM_EINVAL;
    const long N = (long)H * W;
    if (N * C > 0x7fffffffL || f_bs < N * C || out_stride < 1) return IRM_EINVAL;
    if ((reinterpret_cast<uintptr_t>(f) | reinterpret_cast<uintptr_t>(lin)) & 3) return IRM_EINVAL;
    if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(ws)) & 7) return IRM_EINVAL;
    const long nblk = (N + 63) / 64;
    if (ws_words < (long)K * nblk) return IRM_EINVAL;
    LpHead g;
    g.f = f;
    g.f_bs = f_bs;
    g.lin = lin;
    g.K = K;
    g.C = C;
    g.N = (int)N;
    g.nblk = (int)nblk;
    g.part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(lp_head_kernel, dim3((unsigned)nblk, (unsigned)K), dim3(256), 0, stream, g);
    if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
    hipLaunchKernelGGL(lp_fold_kernel, dim3((unsigned)K), dim3(256), 0, stream, g.part, g.nblk, (double)N, out,
                       out_stride);
    return irm_launch_status();
}
