/* irm_hip_inception.h - the kernels of the Inception-ResNet-v2 encoder of DeblurGANv2's FPN-Inception generator that the
 * rest of the C ABI of irm_hip.h does not have: a dense K_h x K_w convolution with stride and zero padding, and the two
 * 3x3 poolings.
 *
 * Included by irm_hip.h at its end, inside its extern "C" block: include irm_hip.h, not this file (the return codes,
 * irm_stream_t and the conventions on pointers and streams are those of irm_hip.h).  The Python binding mirrors this
 * file one to one in _hip.SIGNATURES_INCEPTION.  Tensors are planar NCHW float32; x_bs, y_bs, r_bs are the batch
 * strides in floats, so that an operand may be a channel slice of a larger buffer (a branch of an Inception block
 * writes into, or reads from, its slice of the concat buffer).
 * Null pointers, non-positive sizes and unknown enum values return IRM_EINVAL before any HIP call. */
#pragma once

/* y = relu2?( act1( conv(x, W) + bias ) + res ), a dense kh x kw convolution with `stride` and zero padding
 * (pad_h, pad_w) on the exact-f32 MFMA: output [B][Co][OH][OW], OH = (H + 2 pad_h - kh) / stride + 1 (OW alike; H, W
 * are the INPUT size; rows and columns that no window reaches are ignored).
 *   (kh, kw, stride)  (3,3,2), (3,3,1), (5,5,1), (1,7,1), (7,1,1) and (1,1,1); any other triple is IRM_EINVAL.
 *                     0 <= pad_h < kh, 0 <= pad_w < kw, and at least one output pixel.
 *   wp                packed [kh kw][ceil(Co/16)][ceil(Ci/4)][64]:
 *                     wp[tap][mt][ks][l] = W[16 mt + (l & 15)][4 ks + (l >> 4)][tap / kw][tap % kw], zero beyond Co, Ci
 *                     (_hip.pack_convkxk_weight).  Any Ci >= 1, any Co >= 1.
 *   bias              [Co] or null.    act1: 0 none, 1 ReLU, applied after the bias.
 *   res, res_mode     res_mode 1 adds res [B][Co][OH][OW] AFTER act1 (res may be y itself); 0: res is not read.
 *   relu2             ReLU after the residual.  The closer of an Inception-ResNet block, relu(x + s (W cat + b)), is
 *                     (1,1,1) with s folded into wp and bias, act1 0, res = x, res_mode 1, relu2 1.
 *   ct                output-channel tiles (of 16) a workgroup accumulates per pass: 1, 2 or 4 (5x5: 1 or 2).
 *   ygroups           workgroups that share the passes of one 8 x 32 pixel tile (clamped to [1, passes]).
 * Rows are stored in 16-byte pieces where OW % 4 == 0 and y, res and their batch strides are 16-byte aligned, element
 * by element otherwise. */
int irm_convkxk_f32(const float* wp, const float* x, long x_bs, float* y, long y_bs, const float* res, long r_bs,
                    const float* bias, int B, int Ci, int Co, int H, int W, int kh, int kw, int stride, int pad_h,
                    int pad_w, int act1, int res_mode, int relu2, int ct, int ygroups, irm_stream_t stream);

/* 3x3 pooling of x [B][C][H][W] into y.
 *   mode 0  MaxPool2d(3, stride 2), no padding: y [B][C][(H-3)/2+1][(W-3)/2+1], H, W >= 3; the maximum starts at -inf.
 *   mode 1  AvgPool2d(3, stride 1, padding 1, count_include_pad=False): y [B][C][H][W], the sum of the taps inside the
 *           image divided by their number (4 at corners, 6 at edges, 9 inside). */
int irm_pool3x3_f32(const float* x, long x_bs, float* y, long y_bs, int B, int C, int H, int W, int mode,
                    irm_stream_t stream);
