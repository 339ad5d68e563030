// Noise level of integer frames from the diagonal Haar detail band (include/irm_hip_noise.h):
//   irm_noise_hh_stats   per (frame, channel) the four integers (n, m, below, at) of the 2 x 2 block values
//                        d = |a - b - c + e|: their count, their lower median and the counts below and at it.
// The median is exact: it is read off a histogram.  8-bit codes have d <= 510, one 512-bin histogram; 16-bit words have
// d <= 131070 and take a two-level radix select, d >> 8 in 512 bins, then the low 8 bits of the d in the bin that holds
// the median rank.  Every count is an integer, so the result does not depend on the order of the adds.
//
// Launches, all on the caller's stream (nothing is read back in between):
//   nz_zero_kernel      the histograms of the workspace
//   nz_hist_kernel      pass 1: the frame -> hist[K][NZ_REPL][C][512]
//   nz_select_kernel    8 bit: hist -> stats.   16 bit: hist -> sel[K][C] = (coarse bin, count below it, n),
//   nz_hist_kernel      16 bit, pass 2: the frame -> fine[K][NZ_REPL][C][512], the d of the selected bin only,
//   nz_select_kernel    16 bit: fine, sel -> stats.
//
// nz_hist_kernel: a workgroup walks tiles of NZ_ROWS frame rows x NZ_VALS row values (pixels x channels; a multiple of
// 16 bytes and of 2 C values for both sample sizes and channel counts).  A tile goes to LDS in 16-byte pieces as in
// metrics_video.hip: one 16-byte load where base, pitch and frame stride are 16-byte aligned and the piece lies inside
// the row, element by element otherwise (a view that starts at an odd column, the end of a row).  A trailing odd row or
// column is never read.  Then each thread forms blocks from LDS and adds them to the workgroup's histograms.
//
// Contention: a flat or noise-free frame sends every lane to bin 0.  Each wave has NZ_GROUPS private copies of the
// histogram (lane % NZ_GROUPS picks one; the copies are an odd number of words apart, so equal bins of two copies lie in
// different banks), and before the per-lane adds a wave takes out the values that many of its lanes share: the first
// pending lane's key is broadcast, the lanes that hold it are counted with a ballot and one lane adds the count.  This
// repeats while a round retires at least NZ_PEEL lanes - half a wave: a round costs a lane broadcast and its wait, more
// than the few-deep conflicts of per-lane adds - so a flat frame costs one LDS add per wave and step, and random data
// pays for one round.  A tile's block values are walked channel by channel, so a wave's lanes share their channel and
// a flat RGB frame is one key per wave, not three.  At the end the copies are summed and the non-zero bins go to a global histogram
// with integer atomics.  Adds to one address are served one after another, so a frame has NZ_REPL global copies and
// workgroup b adds to copy b % NZ_REPL; nz_select_kernel sums the copies.
#include "irm_frame.h"

#define NZ_ROWS 8                      // frame rows per tile: four block rows
#define NZ_VALS 768                    // row values per tile: a multiple of 16 bytes, of 2 values and of 6 values
#define NZ_BINS 512
#define NZ_GROUPS 2                    // histogram copies per wave
#define NZ_REPL 8                      // copies of a frame's histogram in global memory
#define NZ_PEEL 32                     // a wave-wide round goes on while it retires at least this many lanes
#define NZ_MAX_WG 256                  // workgroups per frame; each walks the tiles blockIdx.x, + gridDim.x, ...

typedef unsigned long long nz_u64;

template <typename T>
union NzPiece {
    irm_u4 q;
    T e[16 / sizeof(T)];
};

struct NzFrames {
    const void* frames;
    long pitch, frame_stride;          // in samples
    int Hb, Wv;                        // rows and row values in whole blocks: 2 (H / 2), 2 C (W / 2)
    int tiles_x, ntiles;
    int vec;                           // 16-byte pieces may be loaded whole
    int shift, sat_lo, sat_hi;
};

// key of block value d in the histogram of its pass, or -1 where the block is not counted in it
//   PASS 0   8-bit codes: d itself.   PASS 1   d >> 8.   PASS 2   the low byte of the d whose high part is `coarse`
template <int PASS>
__device__ __forceinline__ int nz_bin(int d, int coarse) {
    if (PASS == 0) return d;
    if (PASS == 1) return d >> 8;
    return (d >> 8) == coarse ? (d & 255) : -1;
}

// One round of adds of a whole wave: lane `lane` adds 1 at `key` (channel * NZ_BINS + bin) if `valid`.  hw: the wave's
// NZ_GROUPS copies, `stride` words apart.
__device__ __forceinline__ void nz_wave_add(unsigned* hw, int stride, int key, bool valid, int lane) {
    nz_u64 rem = __ballot(valid);
    while (rem) {                                           // wave-uniform: rem is a ballot
        const int lead = __ffsll((long long)rem) - 1;
        const int k0 = __shfl(key, lead);
        const nz_u64 m = __ballot(valid && key == k0) & rem;
        const int cnt = __popcll(m);
        if (cnt < NZ_PEEL) break;
        if (lane == lead) atomicAdd(&hw[k0], (unsigned)cnt);
        rem &= ~m;
    }
    if ((rem >> lane) & 1) atomicAdd(&hw[(lane % NZ_GROUPS) * stride + key], 1u);
}

template <typename T, int C, int PASS>
__global__ __launch_bounds__(256) void nz_hist_kernel(NzFrames g, const unsigned* sel, unsigned* hist) {
    constexpr int VE = 16 / sizeof(T);                      // values per piece
    constexpr int PPR = NZ_VALS / VE;                       // pieces per tile row
    constexpr int NP = (NZ_ROWS * PPR + 255) / 256;         // pieces per thread
    constexpr int BPR = NZ_VALS / 2;                        // block values per block row of a tile
    constexpr int CPB = BPR / C;                            // blocks per block row of a tile
    constexpr int NB = (NZ_ROWS / 2) * BPR / 256;           // block values per thread
    constexpr int STRIDE = C * NZ_BINS + 1;                 // words between two copies
    static_assert(NZ_VALS % VE == 0 && NZ_VALS % (2 * C) == 0 && ((NZ_ROWS / 2) * BPR) % 256 == 0 && CPB % 64 == 0, "tile");
    __shared__ __attribute__((aligned(16))) T s[NZ_ROWS][NZ_VALS];
    __shared__ unsigned h[4 * NZ_GROUPS * STRIDE];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, frame = blockIdx.y;
    const T* base = reinterpret_cast<const T*>(g.frames) + (long)frame * g.frame_stride;

    for (int i = t; i < 4 * NZ_GROUPS * STRIDE; i += 256) h[i] = 0;
    int coarse[C];
#pragma unroll
    for (int c = 0; c < C; ++c) coarse[c] = PASS == 2 ? (int)sel[((long)frame * C + c) * 4] : 0;
    unsigned* hw = h + wave * NZ_GROUPS * STRIDE;

    for (int tile = blockIdx.x; tile < g.ntiles; tile += gridDim.x) {
        const int ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
        const int y0 = ty * NZ_ROWS, j00 = tx * NZ_VALS;
        const int nrow = min(NZ_ROWS, g.Hb - y0);           // even
        const int rowlen = g.Wv - j00;                      // what is left of the row, in whole blocks
        const int ncol = min(NZ_VALS, rowlen);              // a multiple of 2 C

        NzPiece<T> r[NP];
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int p = t + u * 256, ly = p / PPR, lj0 = (p - ly * PPR) * VE;
            const bool row_in = ly < nrow;
            const long row = (long)(y0 + ly) * g.pitch;
            if (!row_in) {
                r[u].q = irm_u4{0u, 0u, 0u, 0u};
            } else if (g.vec && lj0 + VE <= rowlen) {
                r[u].q = *reinterpret_cast<const irm_u4*>(base + row + j00 + lj0);
            } else {
#pragma unroll
                for (int e = 0; e < VE; ++e) {
                    const bool in = row_in && lj0 + e < ncol;
                    const T v = base[in ? row + j00 + lj0 + e : 0];
                    r[u].e[e] = in ? v : T(0);
                }
            }
        }
        __syncthreads();                                    // the histogram is zero; the last tile has been read
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int p = t + u * 256, ly = p / PPR, lj0 = (p - ly * PPR) * VE;
            if (ly < NZ_ROWS) *reinterpret_cast<irm_u4*>(&s[ly][lj0]) = r[u].q;
        }
        __syncthreads();

#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int item = t + u * 256, br = item / BPR, q = item - br * BPR;
            // a block row of the tile channel by channel: the 64 lanes of a wave share their channel, so the values a
            // flat frame sends to bin 0 are one key per wave, not C
            const int ch = q / CPB, acol = (q - ch * CPB) * 2 * C + ch, bcol = acol + C;
            const bool in = 2 * br + 1 < nrow && bcol < ncol;
            const int ca = in ? acol : 0, cb = in ? bcol : 0, ra = in ? 2 * br : 0, rb = in ? 2 * br + 1 : 0;
            const int a = (int)s[ra][ca] >> g.shift, b = (int)s[ra][cb] >> g.shift;
            const int c = (int)s[rb][ca] >> g.shift, e = (int)s[rb][cb] >> g.shift;
            const int lo = min(min(a, b), min(c, e)), hi = max(max(a, b), max(c, e));
            const int d = abs(a - b - c + e);
            int cs = coarse[0];
#pragma unroll
            for (int k = 1; k < C; ++k) cs = ch == k ? coarse[k] : cs;
            const int bin = nz_bin<PASS>(d, cs);
            const bool valid = in && lo > g.sat_lo && hi < g.sat_hi && bin >= 0;
            nz_wave_add(hw, STRIDE, ch * NZ_BINS + (valid ? bin : 0), valid, lane);
        }
    }
    __syncthreads();
    // the workgroup's copy of the frame's histogram: consecutive workgroups add to different copies, so an address
    // sees an eighth of the workgroups one after another
    unsigned* out = hist + ((long)frame * NZ_REPL + blockIdx.x % NZ_REPL) * C * NZ_BINS;
    for (int k = t; k < C * NZ_BINS; k += 256) {
        unsigned v = 0;
#pragma unroll
        for (int cp = 0; cp < 4 * NZ_GROUPS; ++cp) v += h[cp * STRIDE + k];
        if (v) atomicAdd(&out[k], v);
    }
}

__global__ __launch_bounds__(256) void nz_zero_kernel(unsigned* p, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0;
}

// One workgroup per (frame, channel): the NZ_REPL copies of its 512-bin histogram [K][NZ_REPL][C][512] summed, then the
// bin that holds a rank, by a prefix sum over the bins (thread t owns bins 2 t and 2 t + 1).
//   stage 0   hist of d:       n = its total, rank (n - 1) / 2 -> stats = (n, bin, below, at)
//   stage 1   hist of d >> 8:  the same rank -> sel = (bin, below, n, 0)
//   stage 2   hist of d & 255 inside sel's bin: rank (n - 1) / 2 - sel.below -> stats = (n, 256 sel.bin + bin,
//             sel.below + below, at)
// n == 0 gives stats = (0, 0, 0, 0) and sel = (0, 0, 0, 0).
__global__ __launch_bounds__(256) void nz_select_kernel(const unsigned* hist, unsigned* sel, long long* stats, int C,
                                                        int stage) {
    __shared__ unsigned wsum[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int frame = blockIdx.x / C, ch = blockIdx.x - frame * C;
    const unsigned* hb = hist + ((long)frame * NZ_REPL * C + ch) * NZ_BINS;
    unsigned* sb = sel + (long)blockIdx.x * 4;
    long long* st = stats + (long)blockIdx.x * 4;
    unsigned h0 = 0, h1 = 0;
#pragma unroll
    for (int r = 0; r < NZ_REPL; ++r) {
        const irm_u2 v = *reinterpret_cast<const irm_u2*>(hb + (long)r * C * NZ_BINS + 2 * t);
        h0 += v.x;
        h1 += v.y;
    }
    unsigned inc = h0 + h1;                                 // inclusive prefix over the threads
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned before = inc - (h0 + h1);
    for (int w = 0; w < wave; ++w) before += wsum[w];
    const unsigned total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    unsigned n = total, base_bin = 0, base_below = 0, rank;
    if (stage == 2) {
        base_bin = sb[0] << 8;
        base_below = sb[1];
        n = sb[2];
    }
    if (n == 0) {
        if (t == 0) {
            if (stage == 1) { sb[0] = 0; sb[1] = 0; sb[2] = 0; sb[3] = 0; }
            else { st[0] = 0; st[1] = 0; st[2] = 0; st[3] = 0; }
        }
        return;
    }
    rank = (n - 1) / 2 - base_below;                        // inside this histogram: rank < total
    int bin = -1;
    unsigned below = 0, at = 0;
    if (rank >= before && rank - before < h0) { bin = 2 * t; below = before; at = h0; }
    else if (rank >= before + h0 && rank - before - h0 < h1) { bin = 2 * t + 1; below = before + h0; at = h1; }
    if (bin < 0) return;                                    // exactly one thread holds the rank
    if (stage == 1) {
        sb[0] = (unsigned)bin; sb[1] = below; sb[2] = n; sb[3] = 0;
    } else {
        st[0] = (long long)n;
        st[1] = (long long)(base_bin + (unsigned)bin);
        st[2] = (long long)(base_below + below);
        st[3] = (long long)at;
    }
}

extern "C" int irm_noise_hh_stats(const void* frames, int is_u16, int K, int H, int W, int C, long pitch,
                                  long frame_stride, int shift, int sat_lo, int sat_hi, long long* stats, void* ws,
                                  long ws_words, hipStream_t stream) {
    if (!frames || !stats || !ws) return IRM_EINVAL;
    if (!irm_frames_ok(is_u16, K, H, W, C) || H < 2 || W < 2) return IRM_EINVAL;
    const long rowv = (long)W * C;
    if (pitch < rowv || frame_stride < (long)(H - 1) * pitch + rowv) return IRM_EINVAL;
    if (shift < 0 || shift >= (is_u16 ? 16 : 8) || sat_lo < -1 || sat_hi <= sat_lo) return IRM_EINVAL;
    const uintptr_t es = is_u16 ? 2 : 1;
    if (reinterpret_cast<uintptr_t>(frames) & (es - 1)) return IRM_EINVAL;
    if ((reinterpret_cast<uintptr_t>(stats) | reinterpret_cast<uintptr_t>(ws)) & 7) return IRM_EINVAL;
    const long kc = (long)K * C;
    if (ws_words < 4098 * kc) return IRM_EINVAL;
    // ws: hist [K][NZ_REPL][C][512] u32, fine [K][NZ_REPL][C][512] u32, sel [K][C][4] u32
    unsigned* hist = reinterpret_cast<unsigned*>(ws);
    unsigned* fine = hist + kc * NZ_REPL * NZ_BINS;
    unsigned* sel = fine + kc * NZ_REPL * NZ_BINS;
    NzFrames g;
    g.frames = frames;
    g.pitch = pitch;
    g.frame_stride = frame_stride;
    g.Hb = (H / 2) * 2;
    g.Wv = (W / 2) * 2 * C;
    g.tiles_x = (g.Wv + NZ_VALS - 1) / NZ_VALS;
    const long ntiles = (long)g.tiles_x * ((g.Hb + NZ_ROWS - 1) / NZ_ROWS);
    if (ntiles > 0x7fffffffL) return IRM_EINVAL;
    g.ntiles = (int)ntiles;
    g.vec = irm_aligned16(frames) && (pitch * (long)es) % 16 == 0 && (K == 1 || (frame_stride * (long)es) % 16 == 0);
    g.shift = shift;
    g.sat_lo = sat_lo;
    g.sat_hi = sat_hi;
    const long nzero = (is_u16 ? 2 : 1) * kc * NZ_REPL * NZ_BINS;
    const dim3 grid((unsigned)(ntiles < NZ_MAX_WG ? ntiles : NZ_MAX_WG), K);
    hipLaunchKernelGGL(nz_zero_kernel, dim3((unsigned)((nzero + 255) / 256)), dim3(256), 0, stream, hist, nzero);
    if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
    return irm_dispatch_frames(is_u16, C, [&](auto kind) {
        using T = typename decltype(kind)::type;
        constexpr int CC = decltype(kind)::C;
        constexpr bool WIDE = sizeof(T) == 2;
        hipLaunchKernelGGL((nz_hist_kernel<T, CC, WIDE ? 1 : 0>), grid, dim3(256), 0, stream, g, sel, hist);
        if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
        hipLaunchKernelGGL(nz_select_kernel, dim3((unsigned)kc), dim3(256), 0, stream, hist, sel, stats, CC,
                           WIDE ? 1 : 0);
        if constexpr (WIDE) {
            if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
            hipLaunchKernelGGL((nz_hist_kernel<T, CC, 2>), grid, dim3(256), 0, stream, g, sel, fine);
            if (hipGetLastError() != hipSuccess) return IRM_ELAUNCH;
            hipLaunchKernelGGL(nz_select_kernel, dim3((unsigned)kc), dim3(256), 0, stream, fine, sel, stats, CC, 2);
        }
        return irm_launch_status();
    });
}
