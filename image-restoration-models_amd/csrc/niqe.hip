// NIQE block features on the device (basicsr/metrics/niqe.py: niqe(), compute_feature(), estimate_aggd_param(); the
// host restatement is utils.niqe_features).  For each of K frames [H][W][C] (u8 or u16, C = 1 or 3): the plane is the
// BT.601 Y channel (C = 3) or the values themselves (C = 1), u16 brought to the 0..255 range by / 257, cropped by
// `crop` pixels on every side and then to whole 96 x 96 blocks; the scale-2 plane is its 2 x 2 mean.  Per scale and
// block: the 7 x 7 window mean and sqrt|E[x^2] - mu^2| with the border of the cropped plane repeated (`nearest`), the
// MSCN image (x - mu) / (sigma + 1), and the AGGD fits of the block and of its products with four circularly rolled
// copies of itself (the roll wraps inside the block).  Everything is fp64, from the integers to the features.
//
// One workgroup of 1024 threads per (frame, scale, block), one launch, no workspace:
//   1. the block's plane values plus the 3-pixel halo go to LDS, computed from the input with clamped coordinates
//      (102 x 102 doubles at scale 1; at scale 2 each staged value is the mean of four Y values);
//   2. every thread forms the MSCN value of its pixels (49 taps) in registers; after a barrier the MSCN block
//      replaces the staged tile in LDS;
//   3. for the five signals every thread accumulates, over its pixels in ascending order, the sum of squares and the
//      count of the negative values, the same of the positive values, and the sum of |x|; a butterfly over the wave
//      and an ascending sum over the 16 waves follow;
//   4. all threads scan the table r_gam for the entry nearest to each signal's rhatnorm (ascending, so a thread keeps
//      its lowest index; the wave and workgroup steps prefer the lower index on equal distance: numpy's argmin);
//   5. five lanes finish the 18 features (tgamma of 1 / alpha, 2 / alpha, 3 / alpha).
// No atomics and a fixed order everywhere: a block's features are bitwise the same on every run and for any K.  A
// block without negative (or positive) values divides 0 by 0 and carries the NaN through, as the mean of an empty
// slice does; every comparison with a NaN distance is false and the search then answers index 0, as argmin does.
#include "irm_frame.h"

#define NQ_BLOCK 96
#define NQ_HALO 3
#define NQ_THREADS 1024
#define NQ_WAVES (NQ_THREADS / 64)
#define NQ_TABLE 9801
#define NQ_TILE (NQ_BLOCK + 2 * NQ_HALO)
#define NQ_PER ((NQ_BLOCK * NQ_BLOCK + NQ_THREADS - 1) / NQ_THREADS)

// LDS carve, in doubles
#define NQ_OFF_PART (NQ_TILE * NQ_TILE)            // [NQ_WAVES][25] moment partials
#define NQ_OFF_TOT (NQ_OFF_PART + NQ_WAVES * 25)   // [25] (+ pad)
#define NQ_OFF_WIN (NQ_OFF_TOT + 32)               // [49] (+ pad)
#define NQ_OFF_SD (NQ_OFF_WIN + 56)                // [NQ_WAVES][5] best distances
#define NQ_OFF_SI (NQ_OFF_SD + NQ_WAVES * 5)       // [NQ_WAVES][5] best indices (int)
#define NQ_LDS_DOUBLES (NQ_OFF_SI + NQ_WAVES * 5 / 2)

struct NiqeArgs {
    const void* frames;                // [K][H][W][C]
    const double* window;              // [7][7] correlation weights
    const double* table;               // [2][NQ_TABLE]: r_gam, gam
    double* feat;                      // [K][nbw * nbh][36]
    int H, W, crop, nbh, nbw, bgr, u16;
};

// the plane value at (y, x) of the cropped frame: every product and sum rounded on its own, in the reference's BGR
// order whatever the input's, so an RGB frame and its channel-reversed copy give the same bits
template <typename U, int C>
__device__ __forceinline__ double nq_plane(const U* F, int W, int y, int x, int bgr, int u16) {
    const U* p = F + ((long)y * W + x) * C;
    if (C == 1) return u16 ? (double)p[0] / 257.0 : (double)p[0];
    double b = (double)p[bgr ? 0 : 2], g = (double)p[1], r = (double)p[bgr ? 2 : 0];
    if (u16) {
        b /= 257.0;
        g /= 257.0;
        r /= 257.0;
    }
    const double dot = __dadd_rn(__dadd_rn(__dmul_rn(b / 255.0, 24.966), __dmul_rn(g / 255.0, 128.553)),
                                 __dmul_rn(r / 255.0, 65.481));
    return __dadd_rn(dot, 16.0);
}

template <typename U, int C>
__global__ __launch_bounds__(NQ_THREADS) void niqe_block_kernel(NiqeArgs a) {
    extern __shared__ double sm[];
    double* tile = sm;                 // [T][T] plane values, then [B][B] MSCN values
    double* part = sm + NQ_OFF_PART;
    double* tot = sm + NQ_OFF_TOT;
    double* win = sm + NQ_OFF_WIN;
    double* sd = sm + NQ_OFF_SD;
    int* si = reinterpret_cast<int*>(sm + NQ_OFF_SI);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = a.nbh * a.nbw;
    const int sc = blockIdx.x / nb, n = blockIdx.x - sc * nb, k = blockIdx.y;
    const int bw = n / a.nbh, bh = n - bw * a.nbh;               // the reference's order: column of blocks outer
    const int B = NQ_BLOCK >> sc, T = B + 2 * NQ_HALO;
    const int Hs = (a.nbh * NQ_BLOCK) >> sc, Ws = (a.nbw * NQ_BLOCK) >> sc;      // the plane of this scale
    const U* F = reinterpret_cast<const U*>(a.frames) + (long)k * a.H * a.W * C + ((long)a.crop * a.W + a.crop) * C;

    // 1. the block and its halo; coordinates clamped into the plane (`nearest`), so every read lies inside the frame
    const int y0 = bh * B - NQ_HALO, x0 = bw * B - NQ_HALO;
    for (int i = tid; i < T * T; i += NQ_THREADS) {
        const int ly = i / T, lx = i - ly * T;
        const int gy = min(max(y0 + ly, 0), Hs - 1), gx = min(max(x0 + lx, 0), Ws - 1);
        double v;
        if (sc == 0) {
            v = nq_plane<U, C>(F, a.W, gy, gx, a.bgr, a.u16);
        } else {
            const double v00 = nq_plane<U, C>(F, a.W, 2 * gy, 2 * gx, a.bgr, a.u16);
            const double v01 = nq_plane<U, C>(F, a.W, 2 * gy, 2 * gx + 1, a.bgr, a.u16);
            const double v10 = nq_plane<U, C>(F, a.W, 2 * gy + 1, 2 * gx, a.bgr, a.u16);
            const double v11 = nq_plane<U, C>(F, a.W, 2 * gy + 1, 2 * gx + 1, a.bgr, a.u16);
            v = __dmul_rn(__dadd_rn(__dadd_rn(__dadd_rn(v00, v01), v10), v11), 0.25);
        }
        tile[i] = v;
    }
    if (tid < 49) win[tid] = a.window[tid];
    __syncthreads();

    // 2. MSCN of this thread's pixels, tap sums in row-major tap order
    double ms[NQ_PER];
#pragma unroll
    for (int q = 0; q < NQ_PER; ++q) {
        const int i = tid + q * NQ_THREADS;
        ms[q] = 0.0;
        if (i < B * B) {
            const int py = i / B, px = i - py * B;
            double mu = 0.0, e2 = 0.0;
#pragma unroll 1
            for (int dy = 0; dy < 7; ++dy) {
                const double* row = tile + (py + dy) * T + px;
#pragma unroll
                for (int dx = 0; dx < 7; ++dx) {
                    const double v = row[dx], w = win[dy * 7 + dx];
                    mu = __dadd_rn(mu, __dmul_rn(w, v));
                    e2 = __dadd_rn(e2, __dmul_rn(w, __dmul_rn(v, v)));
                }
            }
            const double sigma = sqrt(fabs(__dsub_rn(e2, __dmul_rn(mu, mu))));
            ms[q] = (tile[(py + NQ_HALO) * T + px + NQ_HALO] - mu) / (sigma + 1.0);
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ_PER; ++q) {
        const int i = tid + q * NQ_THREADS;
        if (i < B * B) tile[i] = ms[q];
    }
    __syncthreads();

    // 3. the moments of the five signals: the block, and its products with np.roll(block, (sy, sx)) for the shifts
    //    (0, 1), (1, 0), (1, 1), (1, -1): rolled[y][x] = block[(y - sy) mod B][(x - sx) mod B]
    double acc[25];
#pragma unroll
    for (int j = 0; j < 25; ++j) acc[j] = 0.0;
#pragma unroll 1
    for (int i = tid; i < B * B; i += NQ_THREADS) {
        const int py = i / B, px = i - py * B;
        const int yu = py == 0 ? B - 1 : py - 1, xl = px == 0 ? B - 1 : px - 1, xr = px == B - 1 ? 0 : px + 1;
        const double c = tile[i];
        const double v[5] = {c, __dmul_rn(c, tile[py * B + xl]), __dmul_rn(c, tile[yu * B + px]),
                             __dmul_rn(c, tile[yu * B + xl]), __dmul_rn(c, tile[yu * B + xr])};
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const double x = v[s], xx = __dmul_rn(x, x);
            acc[s * 5 + 0] += x < 0.0 ? xx : 0.0;
            acc[s * 5 + 1] += x < 0.0 ? 1.0 : 0.0;
            acc[s * 5 + 2] += x > 0.0 ? xx : 0.0;
            acc[s * 5 + 3] += x > 0.0 ? 1.0 : 0.0;
            acc[s * 5 + 4] += fabs(x);
        }
    }
#pragma unroll
    for (int j = 0; j < 25; ++j) {
        double x = acc[j];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
        if (lane == 0) part[wave * 25 + j] = x;
    }
    __syncthreads();
    if (tid < 25) {
        double x = 0.0;
        for (int w = 0; w < NQ_WAVES; ++w) x += part[w * 25 + tid];
        tot[tid] = x;
    }
    __syncthreads();

    // 4. rhatnorm of every signal (all threads compute the same numbers), then the table search
    const double count = (double)(B * B);
    double rh[5], lstd[5], rstd[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        const double* m = tot + s * 5;
        lstd[s] = sqrt(m[0] / m[1]);                              // 0 / 0 = NaN: no negative value in the block
        rstd[s] = sqrt(m[2] / m[3]);
        const double g = lstd[s] / rstd[s], ma = m[4] / count;
        const double rhat = (ma * ma) / ((m[0] + m[2]) / count);
        const double g2 = g * g + 1.0;
        rh[s] = (rhat * (g * g * g + 1.0) * (g + 1.0)) / (g2 * g2);
    }
    double bd[5];
    int bi[5];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
        bd[s] = __builtin_huge_val();
        bi[s] = 0x7fffffff;
    }
    for (int i = tid; i < NQ_TABLE; i += NQ_THREADS) {
        const double r = a.table[i];
#pragma unroll
        for (int s = 0; s < 5; ++s) {
            const double d0 = __dsub_rn(r, rh[s]), d = __dmul_rn(d0, d0);
            if (d < bd[s] || (d == bd[s] && i < bi[s])) {
                bd[s] = d;
                bi[s] = i;
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 5; ++s) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(bd[s], o);
            const int oi = __shfl_xor(bi[s], o);
            if (od < bd[s] || (od == bd[s] && oi < bi[s])) {
                bd[s] = od;
                bi[s] = oi;
            }
        }
        if (lane == 0) {
            sd[wave * 5 + s] = bd[s];
            si[wave * 5 + s] = bi[s];
        }
    }
    __syncthreads();

    // 5. one lane per signal: the workgroup's nearest entry, then the features
    if (tid < 5) {
        const int s = tid;
        double d = sd[s];
        int idx = si[s];
        for (int w = 1; w < NQ_WAVES; ++w) {
            const double od = sd[w * 5 + s];
            const int oi = si[w * 5 + s];
            if (od < d || (od == d && oi < idx)) {
                d = od;
                idx = oi;
            }
        }
        if (idx == 0x7fffffff) idx = 0;                           // every distance NaN: argmin answers 0
        const double alpha = a.table[NQ_TABLE + idx];
        const double g1 = tgamma(1.0 / alpha), g2 = tgamma(2.0 / alpha), g3 = tgamma(3.0 / alpha);
        const double root = sqrt(g1 / g3);
        const double bl = lstd[s] * root, br = rstd[s] * root;
        double* f = a.feat + ((long)k * nb + n) * 36 + sc * 18;
        if (s == 0) {
            f[0] = alpha;
            f[1] = (bl + br) / 2.0;
        } else {
            f += 2 + (s - 1) * 4;
            f[0] = alpha;
            f[1] = (br - bl) * (g2 / g1);
            f[2] = bl;
            f[3] = br;
        }
    }
}

template <typename U, int C>
static int launch_niqe(const NiqeArgs& a, dim3 grid, hipStream_t stream) {
    constexpr size_t lds = NQ_LDS_DOUBLES * sizeof(double);
    IRM_ALLOW_BIG_LDS((niqe_block_kernel<U, C>));
    hipLaunchKernelGGL((niqe_block_kernel<U, C>), grid, dim3(NQ_THREADS), lds, stream, a);
    return irm_launch_status();
}

extern "C" int irm_niqe_features(const void* frames, int is_u16, int K, int H, int W, int C, int crop_border, int bgr,
                                 const double* window, const double* table, double* feat, long feat_words,
                                 hipStream_t stream) {
    if (!frames || !window || !table || !feat) return IRM_EINVAL;
    if (!irm_frames_ok(is_u16, K, H, W, C) || !irm_is_flag(bgr)) return IRM_EINVAL;
    if (crop_border < 0 || crop_border > 16384) return IRM_EINVAL;
    const int nbh = (H - 2 * crop_border) / NQ_BLOCK, nbw = (W - 2 * crop_border) / NQ_BLOCK;
    if (H - 2 * crop_border < NQ_BLOCK || W - 2 * crop_border < NQ_BLOCK || nbh * nbw < 2) return IRM_EINVAL;
    if (feat_words < (long)K * nbh * nbw * 36) return IRM_EINVAL;
    const NiqeArgs a{frames, window, table, feat, H, W, crop_border, nbh, nbw, bgr, is_u16};
    const dim3 grid((unsigned)(2 * nbh * nbw), K);
    return irm_dispatch_frames(is_u16, C, [&](auto kind) {
        return launch_niqe<typename decltype(kind)::type, decltype(kind)::C>(a, grid, stream);
    });
}
