// YUV video frames to the float32 RGB frame of the device pipeline and back: 4:2:0 (I420, NV12, P010;
// include/irm_hip_yuv.h) and, further down, the whole grid of 4:2:0, 4:2:2 and 4:4:4 at 8, 10 and 12 bit
// (include/irm_hip_video.h).  The reference has no YUV path: the arithmetic is stated in tests/yuv_model.py and
// tests/yuv_formats_model.py and restated here with the same float32 operation order, every multiply, add, subtract
// and divide spelled with a correctly rounded intrinsic so that nothing is contracted into a multiply-add.
//
// All kernels are streams.  At 4:2:0 a work item owns four horizontally adjacent 2 x 2 luma blocks (8 x 2 pixels, 4 chroma
// samples per plane).  Where pointer, pitch and width allow it, it moves its luma rows as one 8- / 16-byte piece, its
// chroma as 4- to 16-byte pieces and its two rows of the float frame as 16-byte pieces (a float row starts at 12 W y
// bytes: W % 4 == 0); otherwise, and in a last group that is not full, it moves elements one by one, reads clamped to
// the frame and stores guarded by it.  No LDS, no atomics; nothing outside [H][W] of a plane is written.
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

__device__ __forceinline__ float clip01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// ---------------------------------------------------------------------------
// planes -> rgb

// One chroma row of both planes for the group at cx0: columns cx0 - 1 .. cx0 + 4, clamped to the row.
template <typename T>
__device__ __forceinline__ void chroma_row(const YuvArgs& a, int row, int cx0, bool full, int* ou, int* ov) {
    const T* U = static_cast<const T*>(a.u) + (long)row * a.pitch_c;
    const T* V = static_cast<const T*>(a.v) + (long)row * a.pitch_c;
    if (full && a.vec_c) {
        if (a.step == 2) {                                   // U0 V0 U1 V1 ..: one piece holds both planes
            int t[8];
            load8(U + 2 * cx0, t);
#pragma unroll
            for (int j = 0; j < 4; ++j) { ou[1 + j] = t[2 * j]; ov[1 + j] = t[2 * j + 1]; }
        } else {
            load4(U + cx0, ou + 1);
            load4(V + cx0, ov + 1);
        }
        const long cl = (long)a.step * max(cx0 - 1, 0), cr = (long)a.step * min(cx0 + 4, a.CW - 1);
        ou[0] = (int)U[cl]; ov[0] = (int)V[cl];
        ou[5] = (int)U[cr]; ov[5] = (int)V[cr];
    } else {
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const long c = (long)a.step * min(max(cx0 - 1 + j, 0), a.CW - 1);
            ou[j] = (int)U[c];
            ov[j] = (int)V[c];
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) { ou[j] >>= a.shift; ov[j] >>= a.shift; }
}

template <typename T>
__global__ __launch_bounds__(YUV_WG) void yuv420_to_rgb_kernel(YuvArgs a) {
    const long idx = (long)blockIdx.x * YUV_WG + threadIdx.x;
    if (idx >= (long)a.CH * a.G) return;
    const int g = (int)(idx % a.G), cy = (int)(idx / a.G);
    const int cx0 = 4 * g, x0 = 8 * g;
    const bool full = cx0 + 4 <= a.CW;
    const YuvConst k = a.k;

    // chroma, blended vertically: row 2 cy lies a quarter above its sample, row 2 cy + 1 a quarter below (both sitings)
    int tu[2][6], tv[2][6];
    if (!a.luma_only) {
        int mu[6], mv[6], nu[6], nv[6];
        chroma_row<T>(a, cy, cx0, full, mu, mv);
        chroma_row<T>(a, max(cy - 1, 0), cx0, full, nu, nv);
#pragma unroll
        for (int j = 0; j < 6; ++j) { tu[0][j] = 3 * mu[j] + nu[j]; tv[0][j] = 3 * mv[j] + nv[j]; }
        chroma_row<T>(a, min(cy + 1, a.CH - 1), cx0, full, nu, nv);
#pragma unroll
        for (int j = 0; j < 6; ++j) { tu[1][j] = 3 * mu[j] + nu[j]; tv[1][j] = 3 * mv[j] + nv[j]; }
    }

#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = 2 * cy + r;
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
            float* o = a.rgb + (long)row * a.W + x0;
            if (full && a.vec_rgb) {
                reinterpret_cast<float4*>(o)[0] = make_float4(clip01(yp[0]), clip01(yp[1]), clip01(yp[2]), clip01(yp[3]));
                reinterpret_cast<float4*>(o)[1] = make_float4(clip01(yp[4]), clip01(yp[5]), clip01(yp[6]), clip01(yp[7]));
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (x0 + j < a.W) o[j] = clip01(yp[j]);
            }
            continue;
        }

        float px[24];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int b = 1 + (j >> 1);                      // this pixel's chroma column in tu / tv
            int su, sv;                                      // sixteen times the up-sampled code
            if (a.center) {                                  // a quarter left (even column) or right (odd) of its sample
                const int n = (j & 1) ? b + 1 : b - 1;
                su = 3 * tu[r][b] + tu[r][n];
                sv = 3 * tv[r][b] + tv[r][n];
            } else if (j & 1) {                              // midway between two samples
                su = 2 * tu[r][b] + 2 * tu[r][b + 1];
                sv = 2 * tv[r][b] + 2 * tv[r][b + 1];
            } else {                                         // on its sample
                su = 4 * tu[r][b];
                sv = 4 * tv[r][b];
            }
            const float cb = __fdiv_rn(__fsub_rn(__fmul_rn((float)su, 0.0625f), k.c0), k.cr);
            const float cr = __fdiv_rn(__fsub_rn(__fmul_rn((float)sv, 0.0625f), k.c0), k.cr);
            px[3 * j + 0] = clip01(__fadd_rn(yp[j], __fmul_rn(k.r_cr, cr)));
            px[3 * j + 1] = clip01(__fsub_rn(__fsub_rn(yp[j], __fmul_rn(k.g_cb, cb)), __fmul_rn(k.g_cr, cr)));
            px[3 * j + 2] = clip01(__fadd_rn(yp[j], __fmul_rn(k.b_cb, cb)));
        }
        float* o = a.rgb + ((long)row * a.W + x0) * 3;
        if (full && a.vec_rgb) {
#pragma unroll
            for (int i = 0; i < 6; ++i)
                reinterpret_cast<float4*>(o)[i] = make_float4(px[4 * i], px[4 * i + 1], px[4 * i + 2], px[4 * i + 3]);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (x0 + j < a.W) { o[3 * j] = px[3 * j]; o[3 * j + 1] = px[3 * j + 1]; o[3 * j + 2] = px[3 * j + 2]; }
        }
    }
}

// ---------------------------------------------------------------------------
// rgb -> planes

__device__ __forceinline__ int to_code(float off, float range, float v, float maxcode) {
    return (int)rintf(fminf(fmaxf(__fadd_rn(off, __fmul_rn(range, v)), 0.0f), maxcode));      // half to even
}

template <typename T>
__global__ __launch_bounds__(YUV_WG) void rgb_to_yuv420_kernel(YuvArgs a) {
    const long idx = (long)blockIdx.x * YUV_WG + threadIdx.x;
    if (idx >= (long)a.CH * a.G) return;
    const int g = (int)(idx % a.G), cy = (int)(idx / a.G);
    const int cx0 = 4 * g, x0 = 8 * g;
    const bool full = cx0 + 4 <= a.CW;
    const YuvConst k = a.k;

    // per row: slot 0 is the pixel left of the group (clamped to the row: the left siting's filter), 1..8 the group's
    float cb[2][9], cr[2][9];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = 2 * cy + r;
        T* Y = static_cast<T*>(a.y) + (long)row * a.pitch_y + x0;
        int code[8];
        if (a.luma_only) {
            const float* p = a.rgb + (long)row * a.W + x0;
            float yp[8];
            if (full && a.vec_rgb) {
                const float4 q0 = reinterpret_cast<const float4*>(p)[0], q1 = reinterpret_cast<const float4*>(p)[1];
                yp[0] = q0.x; yp[1] = q0.y; yp[2] = q0.z; yp[3] = q0.w;
                yp[4] = q1.x; yp[5] = q1.y; yp[6] = q1.z; yp[7] = q1.w;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) yp[j] = x0 + j < a.W ? p[j] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) code[j] = to_code(k.y0, k.yr, yp[j], k.maxcode) << a.shift;
        } else {
            const float* p = a.rgb + ((long)row * a.W + x0) * 3;
            float px[27];
            if (full && a.vec_rgb) {
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    const float4 q = reinterpret_cast<const float4*>(p)[i];
                    px[3 + 4 * i] = q.x; px[4 + 4 * i] = q.y; px[5 + 4 * i] = q.z; px[6 + 4 * i] = q.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const bool in = x0 + j < a.W;
                    px[3 + 3 * j] = in ? p[3 * j] : 0.0f;
                    px[4 + 3 * j] = in ? p[3 * j + 1] : 0.0f;
                    px[5 + 3 * j] = in ? p[3 * j + 2] : 0.0f;
                }
            }
            const int l = x0 > 0 ? -3 : 0;                   // x0 < W always: the group exists
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
        if (full && a.vec_y) {
            store8(Y, code);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (x0 + j < a.W) Y[j] = (T)code[j];
        }
    }
    if (a.luma_only) return;

    int cu[4], cv[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int l = 2 * b, m = 2 * b + 1, n = 2 * b + 2;   // left neighbour, even column, odd column
        float fu, fv;
        if (a.center) {
            fu = __fmul_rn(__fadd_rn(__fadd_rn(cb[0][m], cb[0][n]), __fadd_rn(cb[1][m], cb[1][n])), 0.25f);
            fv = __fmul_rn(__fadd_rn(__fadd_rn(cr[0][m], cr[0][n]), __fadd_rn(cr[1][m], cr[1][n])), 0.25f);
        } else {
            const float u0 = __fmul_rn(__fadd_rn(__fadd_rn(cb[0][l], __fadd_rn(cb[0][m], cb[0][m])), cb[0][n]), 0.25f);
            const float u1 = __fmul_rn(__fadd_rn(__fadd_rn(cb[1][l], __fadd_rn(cb[1][m], cb[1][m])), cb[1][n]), 0.25f);
            const float v0 = __fmul_rn(__fadd_rn(__fadd_rn(cr[0][l], __fadd_rn(cr[0][m], cr[0][m])), cr[0][n]), 0.25f);
            const float v1 = __fmul_rn(__fadd_rn(__fadd_rn(cr[1][l], __fadd_rn(cr[1][m], cr[1][m])), cr[1][n]), 0.25f);
            fu = __fmul_rn(__fadd_rn(u0, u1), 0.5f);
            fv = __fmul_rn(__fadd_rn(v0, v1), 0.5f);
        }
        cu[b] = to_code(k.c0, k.cr, fu, k.maxcode) << a.shift;
        cv[b] = to_code(k.c0, k.cr, fv, k.maxcode) << a.shift;
    }
    T* U = static_cast<T*>(a.u) + (long)cy * a.pitch_c;
    T* V = static_cast<T*>(a.v) + (long)cy * a.pitch_c;
    if (full && a.vec_c) {
        if (a.step == 2) {
            const int uv[8] = {cu[0], cv[0], cu[1], cv[1], cu[2], cv[2], cu[3], cv[3]};
            store8(U + 2 * cx0, uv);
        } else {
            store4(U + cx0, cu);
            store4(V + cx0, cv);
        }
    } else {
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (cx0 + b < a.CW) {
                U[(long)a.step * (cx0 + b)] = (T)cu[b];
                V[(long)a.step * (cx0 + b)] = (T)cv[b];
            }
    }
}

// ---------------------------------------------------------------------------
// 4:2:2 and 4:4:4 (include/irm_hip_video.h): rows are independent, a work item owns eight pixels of one row and their
// SW == 2 ? four : eight chroma samples per plane.  The pieces, the element path and the arithmetic are those above.

// One chroma row of both planes at full horizontal resolution: columns x0 .. x0 + 7, clamped to the row.
template <typename T>
__device__ __forceinline__ void chroma_row8(const YuvArgs& a, int row, int x0, bool full, int* ou, int* ov) {
    const T* U = static_cast<const T*>(a.u) + (long)row * a.pitch_c;
    const T* V = static_cast<const T*>(a.v) + (long)row * a.pitch_c;
    if (full && a.vec_c) {
        if (a.step == 2) {                                   // U0 V0 U1 V1 ..: two pieces hold both planes
            int t[16];
            load8(U + 2 * x0, t);
            load8(U + 2 * x0 + 8, t + 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) { ou[j] = t[2 * j]; ov[j] = t[2 * j + 1]; }
        } else {
            load8(U + x0, ou);
            load8(V + x0, ov);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const long c = (long)a.step * min(x0 + j, a.CW - 1);
            ou[j] = (int)U[c];
            ov[j] = (int)V[c];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { ou[j] >>= a.shift; ov[j] >>= a.shift; }
}

template <typename T, int SW>
__global__ __launch_bounds__(YUV_WG) void yuv_rows_to_rgb_kernel(YuvArgs a) {
    const long idx = (long)blockIdx.x * YUV_WG + threadIdx.x;
    if (idx >= (long)a.H * a.G) return;
    const int g = (int)(idx % a.G), row = (int)(idx / a.G);
    const int x0 = 8 * g;
    const bool full = x0 + 8 <= a.W;
    const YuvConst k = a.k;

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
        float* o = a.rgb + (long)row * a.W + x0;
        if (full && a.vec_rgb) {
            reinterpret_cast<float4*>(o)[0] = make_float4(clip01(yp[0]), clip01(yp[1]), clip01(yp[2]), clip01(yp[3]));
            reinterpret_cast<float4*>(o)[1] = make_float4(clip01(yp[4]), clip01(yp[5]), clip01(yp[6]), clip01(yp[7]));
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (x0 + j < a.W) o[j] = clip01(yp[j]);
        }
        return;
    }

    int su[8], sv[8];                                        // sixteen times the up-sampled code
    if (SW == 2) {
        int tu[6], tv[6];                                    // chroma columns 4 g - 1 .. 4 g + 4
        chroma_row<T>(a, row, 4 * g, full, tu, tv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int b = 1 + (j >> 1);
            if (a.center) {                                  // a quarter left (even column) or right (odd) of its sample
                const int n = (j & 1) ? b + 1 : b - 1;
                su[j] = 12 * tu[b] + 4 * tu[n];
                sv[j] = 12 * tv[b] + 4 * tv[n];
            } else if (j & 1) {                              // midway between two samples
                su[j] = 8 * tu[b] + 8 * tu[b + 1];
                sv[j] = 8 * tv[b] + 8 * tv[b + 1];
            } else {                                         // on its sample
                su[j] = 16 * tu[b];
                sv[j] = 16 * tv[b];
            }
        }
    } else {
        chroma_row8<T>(a, row, x0, full, su, sv);
#pragma unroll
        for (int j = 0; j < 8; ++j) { su[j] *= 16; sv[j] *= 16; }
    }

    float px[24];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float cb = __fdiv_rn(__fsub_rn(__fmul_rn((float)su[j], 0.0625f), k.c0), k.cr);
        const float cr = __fdiv_rn(__fsub_rn(__fmul_rn((float)sv[j], 0.0625f), k.c0), k.cr);
        px[3 * j + 0] = clip01(__fadd_rn(yp[j], __fmul_rn(k.r_cr, cr)));
        px[3 * j + 1] = clip01(__fsub_rn(__fsub_rn(yp[j], __fmul_rn(k.g_cb, cb)), __fmul_rn(k.g_cr, cr)));
        px[3 * j + 2] = clip01(__fadd_rn(yp[j], __fmul_rn(k.b_cb, cb)));
    }
    float* o = a.rgb + ((long)row * a.W + x0) * 3;
    if (full && a.vec_rgb) {
#pragma unroll
        for (int i = 0; i < 6; ++i)
            reinterpret_cast<float4*>(o)[i] = make_float4(px[4 * i], px[4 * i + 1], px[4 * i + 2], px[4 * i + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (x0 + j < a.W) { o[3 * j] = px[3 * j]; o[3 * j + 1] = px[3 * j + 1]; o[3 * j + 2] = px[3 * j + 2]; }
    }
}

template <typename T, int SW>
__global__ __launch_bounds__(YUV_WG) void rgb_to_yuv_rows_kernel(YuvArgs a) {
    const long idx = (long)blockIdx.x * YUV_WG + threadIdx.x;
    if (idx >= (long)a.H * a.G) return;
    const int g = (int)(idx % a.G), row = (int)(idx / a.G);
    const int x0 = 8 * g;
    const bool full = x0 + 8 <= a.W;
    const YuvConst k = a.k;

    // slot 0 is the pixel left of the group (clamped to the row: the left siting's filter at 4:2:2), 1..8 the group's
    float cb[9], cr[9];
    T* Y = static_cast<T*>(a.y) + (long)row * a.pitch_y + x0;
    int code[8];
    if (a.luma_only) {
        const float* p = a.rgb + (long)row * a.W + x0;
        float yp[8];
        if (full && a.vec_rgb) {
            const float4 q0 = reinterpret_cast<const float4*>(p)[0], q1 = reinterpret_cast<const float4*>(p)[1];
            yp[0] = q0.x; yp[1] = q0.y; yp[2] = q0.z; yp[3] = q0.w;
            yp[4] = q1.x; yp[5] = q1.y; yp[6] = q1.z; yp[7] = q1.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) yp[j] = x0 + j < a.W ? p[j] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) code[j] = to_code(k.y0, k.yr, yp[j], k.maxcode) << a.shift;
    } else {
        const float* p = a.rgb + ((long)row * a.W + x0) * 3;
        float px[27];
        if (full && a.vec_rgb) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const float4 q = reinterpret_cast<const float4*>(p)[i];
                px[3 + 4 * i] = q.x; px[4 + 4 * i] = q.y; px[5 + 4 * i] = q.z; px[6 + 4 * i] = q.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool in = x0 + j < a.W;
                px[3 + 3 * j] = in ? p[3 * j] : 0.0f;
                px[4 + 3 * j] = in ? p[3 * j + 1] : 0.0f;
                px[5 + 3 * j] = in ? p[3 * j + 2] : 0.0f;
            }
        }
        const int l = SW == 2 && x0 > 0 ? -3 : 0;            // x0 < W always: the group exists
        px[0] = p[l]; px[1] = p[l + 1]; px[2] = p[l + 2];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const float R = px[3 * j], G = px[3 * j + 1], B = px[3 * j + 2];
            const float yp = __fadd_rn(__fadd_rn(__fmul_rn(k.kr, R), __fmul_rn(k.kg, G)), __fmul_rn(k.kb, B));
            cb[j] = __fdiv_rn(__fsub_rn(B, yp), k.b_cb);
            cr[j] = __fdiv_rn(__fsub_rn(R, yp), k.r_cr);
            if (j > 0) code[j - 1] = to_code(k.y0, k.yr, yp, k.maxcode) << a.shift;
        }
    }
    if (full && a.vec_y) {
        store8(Y, code);
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (x0 + j < a.W) Y[j] = (T)code[j];
    }
    if (a.luma_only) return;

    constexpr int NC = 8 / SW;                               // chroma samples of the group, per plane
    const int cx0 = NC * g;
    int cu[NC], cv[NC];
#pragma unroll
    for (int b = 0; b < NC; ++b) {
        float fu, fv;
        if (SW == 1) {
            fu = cb[b + 1];
            fv = cr[b + 1];
        } else {
            const int l = 2 * b, m = 2 * b + 1, n = 2 * b + 2;   // left neighbour, even column, odd column
            if (a.center) {
                fu = __fmul_rn(__fadd_rn(cb[m], cb[n]), 0.5f);
                fv = __fmul_rn(__fadd_rn(cr[m], cr[n]), 0.5f);
            } else {
                fu = __fmul_rn(__fadd_rn(__fadd_rn(cb[l], __fadd_rn(cb[m], cb[m])), cb[n]), 0.25f);
                fv = __fmul_rn(__fadd_rn(__fadd_rn(cr[l], __fadd_rn(cr[m], cr[m])), cr[n]), 0.25f);
            }
        }
        cu[b] = to_code(k.c0, k.cr, fu, k.maxcode) << a.shift;
        cv[b] = to_code(k.c0, k.cr, fv, k.maxcode) << a.shift;
    }
    T* U = static_cast<T*>(a.u) + (long)row * a.pitch_c;
    T* V = static_cast<T*>(a.v) + (long)row * a.pitch_c;
    if (full && a.vec_c) {
        if (a.step == 2) {
            int uv[2 * NC];
#pragma unroll
            for (int b = 0; b < NC; ++b) { uv[2 * b] = cu[b]; uv[2 * b + 1] = cv[b]; }
#pragma unroll
            for (int i = 0; i < NC / 4; ++i) store8(U + 2 * cx0 + 8 * i, uv + 8 * i);
        } else if (SW == 1) {
            store8(U + cx0, cu);
            store8(V + cx0, cv);
        } else {
            store4(U + cx0, cu);
            store4(V + cx0, cv);
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

// The launches of the two directions: (2, 2) is the 8 x 2 block kernel, the other two the row kernel
template <typename T>
static void launch_to_rgb(const YuvArgs& a, int sub_w, int sub_h, hipStream_t stream) {
    const long items = (long)(sub_h == 2 ? a.CH : a.H) * a.G;
    const dim3 grid((unsigned)((items + YUV_WG - 1) / YUV_WG)), wg(YUV_WG);
    if (sub_h == 2) hipLaunchKernelGGL(yuv420_to_rgb_kernel<T>, grid, wg, 0, stream, a);
    else if (sub_w == 2) hipLaunchKernelGGL((yuv_rows_to_rgb_kernel<T, 2>), grid, wg, 0, stream, a);
    else hipLaunchKernelGGL((yuv_rows_to_rgb_kernel<T, 1>), grid, wg, 0, stream, a);
}

template <typename T>
static void launch_to_yuv(const YuvArgs& a, int sub_w, int sub_h, hipStream_t stream) {
    const long items = (long)(sub_h == 2 ? a.CH : a.H) * a.G;
    const dim3 grid((unsigned)((items + YUV_WG - 1) / YUV_WG)), wg(YUV_WG);
    if (sub_h == 2) hipLaunchKernelGGL(rgb_to_yuv420_kernel<T>, grid, wg, 0, stream, a);
    else if (sub_w == 2) hipLaunchKernelGGL((rgb_to_yuv_rows_kernel<T, 2>), grid, wg, 0, stream, a);
    else hipLaunchKernelGGL((rgb_to_yuv_rows_kernel<T, 1>), grid, wg, 0, stream, a);
}

extern "C" int irm_yuv_to_rgb_f32(const void* y, const void* u, const void* v, int chroma_step, long pitch_y,
                                  long pitch_c, int sub_w, int sub_h, int depth, int upper_bits, int matrix,
                                  int full_range, int siting, int luma_only, int H, int W, float* rgb,
                                  hipStream_t stream) {
    YuvArgs a;
    const int rc = yuv_plan(y, u, v, rgb, chroma_step, pitch_y, pitch_c, sub_w, sub_h, depth, upper_bits, matrix,
                            full_range, siting, luma_only, H, W, &a);
    if (rc != IRM_OK) return rc;
    if (depth == 8) launch_to_rgb<uint8_t>(a, sub_w, sub_h, stream);
    else launch_to_rgb<uint16_t>(a, sub_w, sub_h, stream);
    return irm_launch_status();
}

extern "C" int irm_rgb_f32_to_yuv(const float* rgb, void* y, void* u, void* v, int chroma_step, long pitch_y,
                                  long pitch_c, int sub_w, int sub_h, int depth, int upper_bits, int matrix,
                                  int full_range, int siting, int luma_only, int H, int W, hipStream_t stream) {
    YuvArgs a;
    const int rc = yuv_plan(y, u, v, rgb, chroma_step, pitch_y, pitch_c, sub_w, sub_h, depth, upper_bits, matrix,
                            full_range, siting, luma_only, H, W, &a);
    if (rc != IRM_OK) return rc;
    if (depth == 8) launch_to_yuv<uint8_t>(a, sub_w, sub_h, stream);
    else launch_to_yuv<uint16_t>(a, sub_w, sub_h, stream);
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
