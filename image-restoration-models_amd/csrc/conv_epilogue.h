// What the dense 3x3 conv kernels share: the entry checks of irm_conv3x3_ep_f32 and irm_conv3x3_f16x3_ep_f32, and the
// epilogue of the two exact kernels of conv3x3.hip (guarded and ring).  An MFMA lane ends up with 4 consecutive pixels
// (y, x .. x+3) of one output channel co; after the bias the epilogue is act1 -> residual -> relu2 -> store, with
// PixelUnshuffle / PixelShuffle folded into the store.  conv3x3_thin.hip takes the residual rule from here.
//
// The emulated kernel (conv3x3_f16.hip) keeps a written-out copy of the same epilogue and its own argument layout.
// Measured on an MI355X on its 64 -> 64 conv (two stages, so the epilogue is a third of a workgroup's instructions):
// with a common argument struct and irm_conv_store it ran 1.4 % slower than before, with its own layout and
// irm_conv_store 1.1 %, with its own layout and its own epilogue calling only irm_conv_res 0.4 %; as it stands its
// device code is unchanged.  The stage loops were identical in every form; no single instruction accounts for it
// (profiles/conv_epilogue_resources.txt).  A change of the epilogue has to be made in both places.
#pragma once
#include "irm_common.h"

#define IRM_CONV_TW 32                // pixel-tile width of every kernel of the family

// The helpers are templates over the kernel's argument struct A and use its fields by name: Wp, X, x_bs, Y, y_bs, R,
// r_bs, bias; Ci, Co, H, W, mtiles, tiles_x; relu1, slope, res_mode, relu2, store_mode, ps_r (conv3x3.hip documents them).
// Each struct keeps its own field order: the kernel-argument layout is part of what was measured above.

// The argument checks of both entry points; fills `a` and clamps ygroups to [1, passes over the output tiles].
template <class A>
static inline int irm_conv_common(A& a, const float* wp, const float* x, long x_bs, float* y, long y_bs,
                                  const float* res, long r_bs, const float* bias, int B, int Ci, int Co, int H, int W,
                                  int act1, float slope, int res_mode, int relu2, int store_mode, int shuffle, int ct,
                                  int& ygroups) {
    if (!wp || !x || !y || B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) return IRM_EINVAL;
    if (res_mode < 0 || res_mode > 3 || (res_mode && !res) || store_mode < 0 || store_mode > 2) return IRM_EINVAL;
    if (act1 < 0 || act1 > 2 || shuffle < 2 || shuffle > 4) return IRM_EINVAL;
    if (store_mode != 0 && res_mode != 0) return IRM_EINVAL;
    if (store_mode == 1 && ((H & 1) || (W & 1))) return IRM_EINVAL;
    if (store_mode == 2 && (Co % (shuffle * shuffle))) return IRM_EINVAL;
    if (B > 65535 || ct <= 0) return IRM_EINVAL;      // (which ct > 0 exist is the caller's switch)
    a.Wp = wp; a.X = x; a.x_bs = x_bs; a.Y = y; a.y_bs = y_bs; a.R = res; a.r_bs = r_bs; a.bias = bias;
    a.Ci = Ci; a.Co = Co; a.H = H; a.W = W;
    a.mtiles = (Co + 15) / 16; a.tiles_x = (W + IRM_CONV_TW - 1) / IRM_CONV_TW;
    a.relu1 = act1; a.slope = slope; a.res_mode = res_mode; a.relu2 = relu2; a.store_mode = store_mode; a.ps_r = shuffle;
    const int nchunks = (a.mtiles + ct - 1) / ct;
    if (ygroups <= 0) ygroups = 1;
    if (ygroups > nchunks) ygroups = nchunks;
    return IRM_OK;
}

__device__ __forceinline__ float irm_conv_res(float v, float r, int mode) {
    if (mode == 1) return v + r;
    if (mode == 2) return r - v;
    if (mode == 3) return fminf(fmaxf(tanhf(v) + r, -1.0f), 1.0f);      // DeblurGANv2 output: fpn_mobilenet.py:68-70
    return v;
}

template <class A>
__device__ __forceinline__ float irm_conv_act1(float v, const A& a) {
    if (a.relu1 == 1) return fmaxf(v, 0.0f);
    if (a.relu1 == 2) return v > 0.0f ? v : v * a.slope;
    return v;
}

// Residual, relu2 and store of the pixels (y, x .. x+3) of channel co (values after bias and act1); Y, R: this image,
// plane = H * W (every caller holds it).
// vec: the 16-byte / 8-byte paths are legal (W % 4 == 0, aligned planes; then x + 3 < W as well).  GUARD: the
// PixelShuffle stores test x + e < W.  The ring and the emulated kernel run only where vec holds: <false>, vec = true.
// The guarded kernel: <true> and its run-time flag.
template <bool GUARD, class A>
__device__ __forceinline__ void irm_conv_store(float (&v)[4], int co, int y, int x, long plane, float* Y, const float* R,
                                               const A& a, bool vec) {
    if (a.store_mode == 0) {
        const long off = (long)co * plane + (long)y * a.W + x;
        if (vec) {
            if (a.res_mode) {
                const float4 rr = *reinterpret_cast<const float4*>(R + off);
                const float rv[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = irm_conv_res(v[e], rv[e], a.res_mode);
            }
            if (a.relu2) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
            }
            *reinterpret_cast<float4*>(Y + off) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (x + e < a.W) {
                    float t = v[e];
                    if (a.res_mode) t = irm_conv_res(t, R[off + e], a.res_mode);
                    if (a.relu2) t = fmaxf(t, 0.0f);
                    Y[off + e] = t;
                }
            }
        }
    } else if (a.store_mode == 1) {
        // PixelUnshuffle(2): out[co*4 + (y&1)*2 + (x&1)][y/2][x/2]; H, W even
        const int oh = a.H >> 1, ow = a.W >> 1;
        const long op = (long)oh * ow;
        const int oc = co * 4 + (y & 1) * 2;
        const long o = (long)(y >> 1) * ow + (x >> 1);
        if (vec) {
            *reinterpret_cast<float2*>(Y + (long)oc * op + o) = make_float2(v[0], v[2]);
            *reinterpret_cast<float2*>(Y + (long)(oc + 1) * op + o) = make_float2(v[1], v[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < a.W) Y[(long)(oc + (e & 1)) * op + o + (e >> 1)] = v[e];
        }
    } else if (a.ps_r == 2) {
        // PixelShuffle(2): out[co/4][2y + ((co>>1)&1)][2x + (co&1)]
        const int ow = a.W * 2;
        const long op = (long)a.H * 2 * ow;
        const int oc = co >> 2, i = (co >> 1) & 1, jx = co & 1;
        float* o = Y + (long)oc * op + (long)(2 * y + i) * ow + 2 * x + jx;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (!GUARD || x + e < a.W) o[2 * e] = v[e];
    } else {
        // PixelShuffle(r): out[co/r^2][r y + (co/r)%r][r x + co%r]
        const int pr = a.ps_r, ow = a.W * pr;
        const long op = (long)a.H * pr * ow;
        const int oc = co / (pr * pr), i = (co / pr) % pr, jx = co % pr;
        float* o = Y + (long)oc * op + (long)(pr * y + i) * ow + pr * x + jx;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (!GUARD || x + e < a.W) o[pr * e] = v[e];
    }
}
