// The channel-major 8 x 32 tile image and the in-register Gram part shared by fused_qkv_cm.hip (the image is filled by the
// 1x1 conv's MFMAs) and dw_gram.hip (the image is filled from the planar qkv in HBM).
#pragma once
#include "irm_common.h"

constexpr int QC_TH = 8, QC_TW = 32;
constexpr int QC_PITCH = 36;                              // pixel slots per halo row (34 used)
constexpr int QC_SLOTS = (QC_TH + 2) * QC_PITCH;          // 360
constexpr int QC_PT = 23;                                 // 16-slot MFMA tiles (368 slots)
constexpr int QC_CS = 1728;                               // bytes between channel rows
constexpr int QC_IMG = 32 * QC_CS;                        // bytes per image
constexpr int QC_NCH = 4;                                 // tiles per partial Gram record
constexpr int QC_REC = 48 * 48 + 96;                      // floats per record: G[48][48], |q|^2[48], |k|^2[48]

// byte offset of channel row c (0 .. 31) inside an image
__device__ __forceinline__ unsigned qc_row(int c) {
    const int i = c & 15;
    const int rk = i < 4 ? i : i < 12 ? i - 4 : i - 8;                 // rank inside {0-3, 12-15} or inside {4-11}
    const int o = (rk >> 1) * 4 + (rk & 1);                            // 0, 1, 4, 5, 8, 9, 12, 13
    // the row's bank-quad phase is (c CS / 16 + o) mod 16; CS / 16 = 108 = 12 (mod 16): take that out so that the phase is o
    const int fix = (16 - ((c * (QC_CS / 16)) & 15)) & 15;
    return (unsigned)(c * QC_CS + 16 * ((o + fix) & 15));
}

// The Gram state of a wave over the tiles of a chunk: 9 accumulator tiles [q tile][k tile] and the squared norms of the lane's
// channel in each tile.  (The wave's three q tiles of the current 8 x 32 tile, fp16 hi/lo MFMA operands, live per tile: the
// kernels declare them inside their item loop so that the compiler does not carry them across items.)
struct QcGram {
    f32x4 acc[3][3];
    float nq[3], nk[3];
};

__device__ __forceinline__ void qc_gram_clear(QcGram& s) {
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        s.nq[x] = 0.f; s.nk[x] = 0.f;
#pragma unroll
        for (int y = 0; y < 3; ++y) s.acc[x][y] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
}

// One 16-channel tile of stencil outputs (the lane's channel, 8 consecutive pixels of the wave's row): q tile U (U < 3) or k
// tile U - 3.  Scaled by the channel's power of two `sc` (exact), squared norm in fp32, fp16 hi/lo split; a k tile goes
// straight into the 3 x 3 MFMAs against the resident q tiles (the product order of mdta_gram_f16x3_kernel: q_lo k_hi,
// q_hi k_lo, q_hi k_hi).
template <int U>
__device__ __forceinline__ void qc_gram_unit(QcGram& s, irm_h8 (&qh)[3], irm_h8 (&ql)[3], const float (&o)[8], float sc) {
    static_assert(U >= 0 && U < 6, "three q tiles, three k tiles");
    float nn = 0.f, xs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { nn = fmaf(o[e], o[e], nn); xs[e] = o[e] * sc; }
    irm_h8 hi, lo;
    irm_split8(xs, hi, lo);
    if constexpr (U < 3) {
        s.nq[U] += nn; qh[U] = hi; ql[U] = lo;
    } else {
        s.nk[U - 3] += nn;
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            f32x4& t = s.acc[x][U - 3];
            t = irm_mfma3_f16(qh[x], ql[x], hi, lo, t);
        }
    }
}

// End of a chunk: the 8 waves' partial records meet in `scratch` (8 QC_REC floats of LDS that no wave reads or writes any
// more) in wave order and record `rec` of `part` leaves for mdta_reduce / mdta_finalize; the state is cleared.  sq, sk: the operand
// scales of the head's 48 q and 48 k channels (16-byte aligned).  Ends with the sums still being read from `scratch`.
__device__ __forceinline__ void qc_gram_flush(QcGram& s, float* scratch, const float* sq, const float* sk, float* part, long rec,
                                              int wave, int g, int r) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        s.nq[t] += __shfl_xor(s.nq[t], 16); s.nq[t] += __shfl_xor(s.nq[t], 32);
        s.nk[t] += __shfl_xor(s.nk[t], 16); s.nk[t] += __shfl_xor(s.nk[t], 32);
    }
    float* mine = scratch + wave * QC_REC;
    float isk[3];
#pragma unroll
    for (int y = 0; y < 3; ++y) isk[y] = 1.0f / sk[16 * y + r];
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const f32x4 sq4 = *reinterpret_cast<const f32x4*>(sq + 16 * x + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float isq = 1.0f / sq4[e];           // (powers of two: exact)
#pragma unroll
            for (int y = 0; y < 3; ++y) mine[(16 * x + 4 * g + e) * 48 + 16 * y + r] = s.acc[x][y][e] * (isq * isk[y]);
        }
        if (g == 0) { mine[48 * 48 + 16 * x + r] = s.nq[x]; mine[48 * 48 + 48 + 16 * x + r] = s.nk[x]; }
    }
    __syncthreads();
    const float* all = scratch;
    float* out = part + rec * QC_REC;
    for (int e = threadIdx.x; e < QC_REC; e += 512) {
        float sum = all[e];
#pragma unroll
        for (int w = 1; w < 8; ++w) sum += all[w * QC_REC + e];
        out[e] = sum;
    }
    qc_gram_clear(s);
}
