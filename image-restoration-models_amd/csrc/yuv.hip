// YUV video frames to the float32 RGB frame of the device pipeline and back: the whole grid of 4:2:0, 4:2:2 and 4:4:4 at
// 8, 10 and 12 bit (include/irm_hip_video.h) and the 4:2:0 entries for I420, NV12 and P010 (include/irm_hip_yuv.h).
// The reference has no YUV path: the arithmetic is stated in tests/yuv_model.py and tests/yuv_formats_model.py and
// restated here with the same float32 operation order, every multiply, add, subtract and divide spelled with a
// correctly rounded intrinsic so that nothing is contracted into a multiply-add.
//
// One kernel template per direction, instantiated per sample type T and chroma sub-sampling (SW, SH).  All kernels are
// streams.  A work item owns 8 x SH luma pixels and their NC = 8 / SW chroma samples per plane: at 4:2:0 four
// horizontally adjacent 2 x 2 luma blocks, otherwise eight pixels of one row.  Where pointer, pitch and width allow it,
// it moves a luma row as one 8- / 16-byte piece, its chroma as 4- to 16-byte pieces and a row of the float frame as
// 16-byte pieces (a float row starts at 12 W y bytes: W % 4 == 0); otherwise, and in a last group that is not full, it
// moves elements one by one, reads clamped to the frame and stores guarded by it.  No LDS, no atomics; nothing outside
// [H][W] of a plane is written.
#include "irm_common.h"

// The rounded intrinsics are plain operators to the compiler (inline functions of its headers), which under its default
// -ffp-contract=fast still fuses a product with the sum that takes it - G = (Y' - g_cb Cb) - .. came out one ulp off the
// model.  The Makefile therefore builds this file with -ffp-contract=off; a pragma here would not reach the headers.

#define YUV_WG 128

struct YuvConst {
    float y0, yr, c0, cr;              // code = offset + range * value
    float kr, kg, kb;                  // Y' = (kr R + kg G) + kb B
    float r_cr, b_cb, g_cb, g_cr;      // R = Y' + r_cr Cr, B = Y' + b_cb Cb, G = (Y' - g_cb Cb) - g_cr Cr
    float maxcode;
};

struct YuvArgs {
    void* y;
    void* u;
    void* v;
    float* rgb;                        // [H][W][3], or [H][W][1] with luma_only
    long pitch_y, pitch_c;             // in samples
    int H, W, CH, CW, G;               // chroma extents, groups of eight luma columns per row
    int step, shift, center, luma_only;
    int vec_rgb, vec_y, vec_c;         // the 16-byte frame path, the 8-sample luma path, the 4- / 8-sample chroma path
    YuvConst k;
};

// ---- 4 / 8 adjacent samples as one piece
__device__ __forceinline__ void load4(const uint8_t* p, int* o) {
    const uint32_t q = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (int)((q >> (8 * j)) & 0xffu);
}
__device__ __forceinline__ void load4(const uint16_t* p, int* o) {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    o[0] = (int)(q.x & 0xffffu); o[1] = (int)(q.x >> 16);
    o[2] = (int)(q.y & 0xffffu); o[3] = (int)(q.y >> 16);
}
__device__ __forceinline__ void load8(const uint8_t* p, int* o) {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = (int)((q.x >> (8 * j)) & 0xffu);
        o[4 + j] = (int)((q.y >> (8 * j)) & 0xffu);
    }
}
__device__ __forceinline__ void load8(const uint16_t* p, int* o) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    o[0] = (int)(q.x & 0xffffu); o[1] = (int)(q.x >> 16);
    o[2] = (int)(q.y & 0xffffu); o[3] = (int)(q.y >> 16);
    o[4] = (int)(q.z & 0xffffu); o[5] = (int)(q.z >> 16);
    o[6] = (int)(q.w & 0xffffu); o[7] = (int)(q.w >> 16);
}
__device__ __forceinline__ void store4(uint8_t* p, const int* c) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
}
__device__ __forceinline__ void store4(uint16_t* p, const int* c) {
    *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)c[0] | ((uint32_t)c[1] << 16), (uint32_t)c[2] | ((uint32_t)c[3] << 16));
}
__device__ __forceinline__ void store8(uint8_t* p, const int* c) {
    *reinterpret_cast<uint2*>(p) = make_uint2(
        (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24),
        (uint32_t)c[4] | ((uint32_t)c[5] << 8) | ((uint32_t)c[6] << 16) | ((uint32_t)c[7] << 24));
}
__device__ __forceinline__ void store8(uint16_t* p, const int* c) {
    *reinterpret_cast<uint4*>(p) = make_uint4((uint32_t)c[0] | ((uint32_t)c[1] << 16), (uint32_t)c[2] | ((uint32_t)c[3] << 16),
                                              (uint32_t)c[4] | ((uint32_t)c[5] << 16), (uint32_t)c[6] | ((uint32_t)c[7] << 16));
}
// N = 4 or 8 samples of one plane: the planar chroma of a group
template <int N, typename T>
__device__ __forceinline__ void load_piece(const T* p, int* o) {
    if (N == 4) load4(p, o);
    else load8(p, o);
}
template <int N, typename T>
__device__ __forceinline__ void store_piece(T* p, const int* c) {
    if (N == 4) store4(p, c);
    else store8(p, c);
}

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// ---- the eight pixels of a group in one row of the float frame, C = 3 (RGB) or 1 (luma_only) values each
template <int C>
__device__ __forceinline__ void store_frame_row(const YuvArgs& a, int row, int x0, bool full, const float* px) {
    float* o = a.rgb + ((long)row * a.W + x0) * C;
    if (full && a.vec_rgb) {
#pragma unroll
        for (int i = 0; i < 2 * C; ++i)
            reinterpret_cast<f32x4*>(o)[i] = f32x4{px[4 * i], px[4 * i + 1], px[4 * i + 2], px[4 * i + 3]};
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (x0 + j < a.W) {
#pragma unroll
                for (int c = 0; c < C; ++c) o[C * j + c] = px[C * j + c];
            }
    }
}

// The mirror image; a pixel outside the frame reads as 0.  Returns the group's first value in the frame.
template <int C>
__device__ __forceinline__ const float* load_frame_row(const YuvArgs& a, int row, int x0, bool full, float* px) {
    const float* p = a.rgb + ((long)row * a.W + x0) * C;
    if (full && a.vec_rgb) {
#pragma unroll
        for (int i = 0; i < 2 * C; ++i) {
            const f32x4 q = reinterpret_cast<const f32x4*>(p)[i];
            px[4 * i] = q.x; px[4 * i + 1] = q.y; px[4 * i + 2] = q.z; px[4 * i + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool in = x0 + j < a.W;
#pragma unroll
            for (int c = 0; c < C; ++c) px[C * j + c] = in ? p[C * j + c] : 0.0f;
        }
    }
    return p;
}

// ---------------------------------------------------------------------------
// planes -> rgb

// One chroma row of both planes for the group at cx0, clamped to the row: its NC samples and, where the row is
// up-sampled (SW == 2), one more on either side - columns cx0 - 1 .. cx0 + 4.
template <typename T, int SW>
__device__ __forceinline__ void chroma_taps(const YuvArgs& a, int row, int cx0, bool full, int* ou, int* ov) {
    constexpr int NC = 8 / SW, E = SW - 1, NT = NC + 2 * E;
    const T* U = static_cast<const T*>(a.u) + (long)row * a.pitch_c;
    const T* V = static_cast<const T*>(a.v) + (long)row * a.pitch_c;
    if (full && a.vec_c) {
        if (a.step == 2) {                                   // U0 V0 U1 V1 ..: pieces of eight hold both planes
            int t[2 * NC];
#pragma unroll
            for (int i = 0; i < NC / 4; ++i) load8(U + 2 * cx0 + 8 * i, t + 8 * i);
#pragma unroll
            for (int j = 0; j < NC; ++j) { ou[E + j] = t[2 * j]; ov[E + j] = t[2 * j + 1]; }
        } else {
            load_piece<NC>(U + cx0, ou + E);
            load_piece<NC>(V + cx0, ov + E);
        }
        if (SW == 2) {
            const long cl = (long)a.step * max(cx0 - 1, 0), cr = (long)a.step * min(cx0 + 4, a.CW - 1);
            ou[0] = (int)U[cl]; ov[0] = (int)V[cl];
            ou[5] = (int)U[cr]; ov[5] = (int)V[cr];
        }
    } else {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const long c = (long)a.step * min(max(cx0 - E + j, 0), a.CW - 1);
            ou[j] = (int)U[c];
            ov[j] = (int)V[c];
        }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) { ou[j] >>= a.shift; ov[j] >>= a.shift; }
}

template <typename T, int SW, int SH>
__global__ __launch_bounds__(YUV_WG) void yuv_to_rgb_kernel(YuvArgs a) {
    constexpr int NC = 8 / SW, NT = NC + 2 * (SW - 1);
    const long idx = (long)blockIdx.x * YUV_WG + threadIdx.x;
    if (idx >= (long)a.CH * a.G) return;                     // CH = H / SH rows of groups
    const int g = (int)(idx % a.G), cy = (int)(idx / a.G);
    const int cx0 = NC * g, x0 = 8 * g;
    const bool full = cx0 + NC <= a.CW;
    const YuvConst k = a.k;

    // chroma, vertical stage: four times the code at each luma row.  SH == 2: row 2 cy lies a quarter above its sample,
    // row 2 cy + 1 a quarter below (both sitings)
    int tu[SH][NT], tv[SH][NT];
    if (!a.luma_only) {
        int mu[NT], mv[NT];
        chroma_taps<T, SW>(a, cy, cx0, full, mu, mv);
#pragma unroll
        for (int r = 0; r < SH; ++r) {
            if (SH == 2) {
                int nu[NT], nv[NT];
                chroma_taps<T, SW>(a, r ? min(cy + 1, a.CH - 1) : max(cy - 1, 0), cx0, full, nu, nv);
#pragma unroll
                for (int j = 0; j < NT; ++j) { tu[r][j] = 3 * mu[j] + nu[j]; tv[r][j] = 3 * mv[j] + nv[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < NT; ++j) { tu[r][j] = 4 * mu[j]; tv[r][j] = 4 * mv[j]; }
            }
        }
    }

#pragma unroll
    for (int r = 0; r < SH; ++r) {
        const int row = SH * cy + r;
        const T* Y = static_cast<const T*>(a.y) + (long)row * a.pitch_y + x0;
        int yv[8];
        if (full && a.vec_y) {
            load8(Y, yv);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) yv[j] = x0 + j < a.W ? (int)Y[j] : 0;
        }
        float yp[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) yp[j] = __fdiv_rn(__fsub_rn((float)(yv[j] >> a.shift), k.y0), k.yr);

        if (a.luma_only) {
#pragma unroll
            for (int j = 0; j < 8; ++j) yp[j] = clip01(yp[j]);
            store_frame_row<1>(a, row, x0, full, yp);
            continue;
        }

        float px[24];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int su, sv;                                      // horizontal stage: sixteen times the up-sampled code
            if (SW == 1) {
                su = 4 * tu[r][j];
                sv = 4 * tv[r][j];
            } else {
                const int b = 1 + (j >> 1);                  // this pixel's chroma column in tu / tv
                if (a.center) {                              // a quarter left (even column) or right (odd) of its sample
                    const int n = (j & 1) ? b + 1 : b - 1;
                    su = 3 * tu[r][b] + tu[r][n];
                    sv = 3 * tv[r][b] + tv[r][n];
                } else if (j & 1) {                          // midway between two samples
                    su = 2 * tu[r][b] + 2 * tu[r][b + 1];
                    sv = 2 * tv[r][b] + 2 * tv[r][b + 1];
                } else {                                     // on its sample
                    su = 4 * tu[r][b];
                    sv = 4 * tv[r][b];
                }
            }
            const float cb = __fdiv_rn(__fsub_rn(__fmul_rn((float)su, 0.0625f), k.c0), k.cr);
            const float cr = __fdiv_rn(__fsub_rn(__fmul_rn((float)sv, 0.0625f), k.c0), k.cr);
            px[3 * j + 0] = clip01(__fadd_rn(yp[j], __fmul_rn(k.r_cr, cr)));
            px[3 * j + 1] = clip01(__fsub_rn(__fsub_rn(yp[j], __fmul_rn(k.g_cb, cb)), __fmul_rn(k.g_cr, cr)));
            px[3 * j + 2] = clip01(__fadd_rn(yp[j], __fmul_rn(k.b_cb, cb)));
        }
        store_frame_row<3>(a, row, x0, full, px);
    }
}

// ---------------------------------------------------------------------------
// rgb -> planes

__device__ __forceinline__ int to_code(float off, float range, float v, float maxcode) {
    return (int)rintf(fminf(fmaxf(__fadd_rn(off, __fmul_rn(range, v)), 0.0f), maxcode));      // half to even
}

template <typename T, int SW, int SH>
__global__ __launch_bounds__(YUV_WG) void rgb_to_yuv_kernel(YuvArgs a) {
    constexpr int NC = 8 / SW;
    const long idx = (long)blockIdx.x * YUV_WG + threadIdx.x;
    if (idx >= (long)a.CH * a.G) return;                     // CH = H / SH rows of groups
    const int g = (int)(idx % a.G), cy = (int)(idx / a.G);
    const int cx0 = NC * g, x0 = 8 * g;
    const bool full = cx0 + NC <= a.CW;
    const YuvConst k = a.k;

    // per row: slot 0 is the pixel left of the group (clamped to the row: the left siting's filter at SW == 2), 1..8 the
    // group's
    float cb[SH][9], cr[SH][9];
#pragma unroll
    for (int r = 0; r < SH; ++r) {
        const int row = SH * cy + r;
        int code[8];
        if (a.luma_only) {
            float yp[8];
            load_frame_row<1>(a, row, x0, full, yp);
#pragma unroll
            for (int j = 0; j < 8; ++j) code[j] = to_code(k.y0, k.yr, yp[j], k.maxcode) << a.shift;
        } else {
            float px[27];
            const float* p = load_frame_row<3>(a, row, x0, full, px + 3);
            const int l = SW == 2 && x0 > 0 ? -3 : 0;        // x0 < W always: the group exists
            px[0] = p[l]; px[1] = p[l + 1]; px[2] = p[l + 2];
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const float R = px[3 * j], G = px[3 * j + 1], B = px[3 * j + 2];
                const float yp = __fadd_rn(__fadd_rn(__fmul_rn(k.kr, R), __fmul_rn(k.kg, G)), __fmul_rn(k.kb, B));
                cb[r][j] = __fdiv_rn(__fsub_rn(B, yp), k.b_cb);
                cr[r][j] = __fdiv_rn(__fsub_rn(R, yp), k.r_cr);
                if (j > 0) code[j - 1] = to_code(k.y0, k.yr, yp, k.maxcode) << a.shift;
            }
        }
        T* Y = static_cast<T*>(a.y) + (long)row * a.pitch_y + x0;
        if (full && a.vec_y) {
            store8(Y, code);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (x0 + j < a.W) Y[j] = (T)code[j];
        }
    }
    if (a.luma_only) return;

    // The chroma filter.  Its three spellings fix the order of the additions (the float32 models): none is written in
    // terms of another, halving is not exact for subnormals.
    constexpr int r1 = SH - 1;                               // the group's second row at SH == 2
    int cu[NC], cv[NC];
#pragma unroll
    for (int b = 0; b < NC; ++b) {
        const int l = 2 * b, m = 2 * b + 1, n = 2 * b + 2;   // SW == 2: left neighbour, even column, odd column
        float fu, fv;
        if (SW == 1) {
            fu = cb[0][b + 1];
            fv = cr[0][b + 1];
        } else if (SH == 1) {
            if (a.center) {
                fu = __fmul_rn(__fadd_rn(cb[0][m], cb[0][n]), 0.5f);
                fv = __fmul_rn(__fadd_rn(cr[0][m], cr[0][n]), 0.5f);
            } else {
                fu = __fmul_rn(__fadd_rn(__fadd_rn(cb[0][l], __fadd_rn(cb[0][m], cb[0][m])), cb[0][n]), 0.25f);
                fv = __fmul_rn(__fadd_rn(__fadd_rn(cr[0][l], __fadd_rn(cr[0][m], cr[0][m])), cr[0][n]), 0.25f);
            }
        } else if (a.center) {
            fu = __fmul_rn(__fadd_rn(__fadd_rn(cb[0][m], cb[0][n]), __fadd_rn(cb[r1][m], cb[r1][n])), 0.25f);
            fv = __fmul_rn(__fadd_rn(__fadd_rn(cr[0][m], cr[0][n]), __fadd_rn(cr[r1][m], cr[r1][n])), 0.25f);
        } else {
            const float u0 = __fmul_rn(__fadd_rn(__fadd_rn(cb[0][l], __fadd_rn(cb[0][m], cb[0][m])), cb[0][n]), 0.25f);
            const float u1 = __fmul_rn(__fadd_rn(__fadd_rn(cb[r1][l], __fadd_rn(cb[r1][m], cb[r1][m])), cb[r1][n]), 0.25f);
            const float v0 = __fmul_rn(__fadd_rn(__fadd_rn(cr[0][l], __fadd_rn(cr[0][m], cr[0][m])), cr[0][n]), 0.25f);
            const float v1 = __fmul_rn(__fadd_rn(__fadd_rn(cr[r1][l], __fadd_rn(cr[r1][m], cr[r1][m])), cr[r1][n]), 0.25f);
            fu = __fmul_rn(__fadd_rn(u0, u1), 0.5f);
            fv = __fmul_rn(__fadd_rn(v0, v1), 0.5f);
        }
        cu[b] = to_code(k.c0, k.cr, fu, k.maxcode) << a.shift;
        cv[b] = to_code(k.c0, k.cr, fv, k.maxcode) << a.shift;
    }
    T* U = static_cast<T*>(a.u) + (long)cy * a.pitch_c;
    T* V = static_cast<T*>(a.v) + (long)cy * a.pitch_c;
    if (full && a.vec_c) {
        if (a.step == 2) {                                   // U0 V0 U1 V1 ..: pieces of eight hold both planes
            int uv[2 * NC];
#pragma unroll
            for (int b = 0; b < NC; ++b) { uv[2 * b] = cu[b]; uv[2 * b + 1] = cv[b]; }
#pragma unroll
            for (int i = 0; i < NC / 4; ++i) store8(U + 2 * cx0 + 8 * i, uv + 8 * i);
        } else {
            store_piece<NC>(U + cx0, cu);
            store_piece<NC>(V + cx0, cv);
        }
    } else {
#pragma unroll
        for (int b = 0; b < NC; ++b)
            if (cx0 + b < a.CW) {
                U[(long)a.step * (cx0 + b)] = (T)cu[b];
                V[(long)a.step * (cx0 + b)] = (T)cv[b];
            }
    }
}

// ---------------------------------------------------------------------------
// The checks and the plan the entry points share; IRM_EINVAL before any HIP call.
static int yuv_plan(const void* y, const void* u, const void* v, const float* rgb, int chroma_step, long pitch_y,
                    long pitch_c, int sub_w, int sub_h, int depth, int upper_bits, int matrix, int full_range, int siting,
                    int luma_only, int H, int W, YuvArgs* a) {
    if (!((sub_w == 2 && sub_h == 2) || (sub_w == 2 && sub_h == 1) || (sub_w == 1 && sub_h == 1))) return IRM_EINVAL;
    if (!y || !rgb || H <= 0 || W <= 0 || H % sub_h || W % sub_w || H > (1 << 20) || W > (1 << 20)) return IRM_EINVAL;
    if ((depth != 8 && depth != 10 && depth != 12) || (upper_bits != 0 && upper_bits != 1) || (depth == 8 && upper_bits))
        return IRM_EINVAL;
    if ((matrix != 0 && matrix != 1) || (full_range != 0 && full_range != 1) || (siting != 0 && siting != 1)
        || (luma_only != 0 && luma_only != 1)) return IRM_EINVAL;
    if (pitch_y < W || (reinterpret_cast<uintptr_t>(rgb) & 3)) return IRM_EINVAL;
    const uintptr_t es = depth == 8 ? 1 : 2;                 // bytes per sample
    if (reinterpret_cast<uintptr_t>(y) & (es - 1)) return IRM_EINVAL;
    if (!luma_only) {
        if (!u || !v || (chroma_step != 1 && chroma_step != 2) || pitch_c < (long)chroma_step * (W / sub_w)) return IRM_EINVAL;
        if ((reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(v)) & (es - 1)) return IRM_EINVAL;
    }
    const double kr = matrix ? 0.2126 : 0.299, kb = matrix ? 0.0722 : 0.114, kg = 1.0 - kr - kb;
    const double s = (double)(1 << (depth - 8)), top = (double)((1 << depth) - 1);
    YuvConst k;
    k.y0 = (float)(full_range ? 0.0 : 16.0 * s);
    k.yr = (float)(full_range ? top : 219.0 * s);
    k.c0 = (float)(128.0 * s);
    k.cr = (float)(full_range ? top : 224.0 * s);
    k.kr = (float)kr; k.kg = (float)kg; k.kb = (float)kb;
    k.r_cr = (float)(2.0 * (1.0 - kr));
    k.b_cb = (float)(2.0 * (1.0 - kb));
    k.g_cb = (float)(2.0 * kb * (1.0 - kb) / kg);
    k.g_cr = (float)(2.0 * kr * (1.0 - kr) / kg);
    k.maxcode = (float)top;
    a->y = const_cast<void*>(y); a->u = const_cast<void*>(u); a->v = const_cast<void*>(v);
    a->rgb = const_cast<float*>(rgb);
    a->pitch_y = pitch_y; a->pitch_c = pitch_c;
    a->H = H; a->W = W; a->CH = H / sub_h; a->CW = W / sub_w; a->G = (W + 7) / 8;
    a->step = chroma_step; a->shift = upper_bits ? 16 - depth : 0; a->center = siting; a->luma_only = luma_only;
    // a piece is moved whole only where every piece of its kind is aligned: the base and every row start (the sixteen
    // interleaved samples of a 4:4:4 group move as two pieces of eight)
    const uintptr_t ya = 8 * es, ca = (chroma_step == 2 || sub_w == 1 ? 8 : 4) * es;
    a->vec_rgb = (W % 4 == 0) && !(reinterpret_cast<uintptr_t>(rgb) & 15);
    a->vec_y = !((reinterpret_cast<uintptr_t>(y) | (uintptr_t)(pitch_y * (long)es)) & (ya - 1));
    a->vec_c = 0;
    if (!luma_only) {
        const uintptr_t cu = reinterpret_cast<uintptr_t>(u), cv = reinterpret_cast<uintptr_t>(v);
        const bool rows = !((uintptr_t)(pitch_c * (long)es) & (ca - 1));
        a->vec_c = chroma_step == 2 ? (rows && !(cu & (ca - 1)) && cv == cu + es)       // NV12 order: v = u + 1 sample
                                    : (rows && !((cu | cv) & (ca - 1)));
    }
    a->k = k;
    return IRM_OK;
}

// One work item per group of 8 x SH luma pixels: CH = H / SH rows of G groups
template <typename T, bool TO_RGB>
static void yuv_launch(const YuvArgs& a, int sub_w, int sub_h, hipStream_t stream) {
    const long items = (long)a.CH * a.G;
    const dim3 grid((unsigned)((items + YUV_WG - 1) / YUV_WG)), wg(YUV_WG);
    void (*kernel)(YuvArgs) =
        sub_h == 2   ? (TO_RGB ? yuv_to_rgb_kernel<T, 2, 2> : rgb_to_yuv_kernel<T, 2, 2>)
        : sub_w == 2 ? (TO_RGB ? yuv_to_rgb_kernel<T, 2, 1> : rgb_to_yuv_kernel<T, 2, 1>)
                     : (TO_RGB ? yuv_to_rgb_kernel<T, 1, 1> : rgb_to_yuv_kernel<T, 1, 1>);
    hipLaunchKernelGGL(kernel, grid, wg, 0, stream, a);
}

extern "C" int irm_yuv_to_rgb_f32(const void* y, const void* u, const void* v, int chroma_step, long pitch_y,
                                  long pitch_c, int sub_w, int sub_h, int depth, int upper_bits, int matrix,
                                  int full_range, int siting, int luma_only, int H, int W, float* rgb,
                                  hipStream_t stream) {
    YuvArgs a;
    const int rc = yuv_plan(y, u, v, rgb, chroma_step, pitch_y, pitch_c, sub_w, sub_h, depth, upper_bits, matrix,
                            full_range, siting, luma_only, H, W, &a);
    if (rc != IRM_OK) return rc;
    if (depth == 8) yuv_launch<uint8_t, true>(a, sub_w, sub_h, stream);
    else yuv_launch<uint16_t, true>(a, sub_w, sub_h, stream);
    return irm_launch_status();
}

extern "C" int irm_rgb_f32_to_yuv(const float* rgb, void* y, void* u, void* v, int chroma_step, long pitch_y,
                                  long pitch_c, int sub_w, int sub_h, int depth, int upper_bits, int matrix,
                                  int full_range, int siting, int luma_only, int H, int W, hipStream_t stream) {
    YuvArgs a;
    const int rc = yuv_plan(y, u, v, rgb, chroma_step, pitch_y, pitch_c, sub_w, sub_h, depth, upper_bits, matrix,
                            full_range, siting, luma_only, H, W, &a);
    if (rc != IRM_OK) return rc;
    if (depth == 8) yuv_launch<uint8_t, false>(a, sub_w, sub_h, stream);
    else yuv_launch<uint16_t, false>(a, sub_w, sub_h, stream);
    return irm_launch_status();
}

// The 4:2:0 entries of include/irm_hip_yuv.h: depths 8 and 10 only, as they were
extern "C" int irm_yuv420_to_rgb_f32(const void* y, const void* u, const void* v, int chroma_step, long pitch_y,
                                     long pitch_c, int depth, int upper_bits, int matrix, int full_range, int siting,
                                     int luma_only, int H, int W, float* rgb, hipStream_t stream) {
    if (depth != 8 && depth != 10) return IRM_EINVAL;
    return irm_yuv_to_rgb_f32(y, u, v, chroma_step, pitch_y, pitch_c, 2, 2, depth, upper_bits, matrix, full_range, siting,
                              luma_only, H, W, rgb, stream);
}

extern "C" int irm_rgb_f32_to_yuv420(const float* rgb, void* y, void* u, void* v, int chroma_step, long pitch_y,
                                     long pitch_c, int depth, int upper_bits, int matrix, int full_range, int siting,
                                     int luma_only, int H, int W, hipStream_t stream) {
    if (depth != 8 && depth != 10) return IRM_EINVAL;
    return irm_rgb_f32_to_yuv(rgb, y, u, v, chroma_step, pitch_y, pitch_c, 2, 2, depth, upper_bits, matrix, full_range,
                              siting, luma_only, H, W, stream);
}
