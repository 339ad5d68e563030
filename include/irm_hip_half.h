/* irm_hip_half.h - the fp16 entry points of libirm_hip.so, an extension of the C ABI of irm_hip.h.
 *
 * Included by irm_hip.h at its end, inside its extern "C" block: include irm_hip.h, not this file (the return codes,
 * irm_stream_t and the conventions on pointers, streams and batch strides are those of irm_hip.h).  The Python binding
 * mirrors this file one to one in _hip.SIGNATURES_HALF, next to _hip.SIGNATURES for irm_hip.h. */
#pragma once

/* ---- fp16 inference mode of the conv stacks (conv3x3_h.hip; DnCNN network_dncnn.py:40-71, REDNet rednet.py:64-136).
 * Hidden activations are fp16 CHANNEL-LAST, [B][H][W][C] with C in {64, 128}: element (b, y, x, c) at
 * base[b*bs + (y*W + x)*C + c], batch strides in fp16 elements and multiples of 8, bases 16-byte aligned (`void*` =
 * fp16 data).  All three kernels: stride 1, zero pad 1, any H and W.  A value stored as fp16 is ONE round-to-nearest-
 * even conversion of the fp32 epilogue result: beyond +-65504 it is +-inf, NaN stays NaN (the ReLUs pass NaN), there is
 * no clamp.  This mode is not reference-parity: every hidden activation is rounded to 11 significant bits.
 *
 * irm_conv3x3_h_in_f32: x fp32 planar [B][Ci <= 3][H][W] -> y fp16 channel-last, Co in {64, 128};
 *   v = conv(x)[co] + bias[co] (fp32 FMAs on the vector pipe); if relu1: v = max(v, 0).  w: the plain weight
 *   [Co][Ci][3][3] fp32 (device).  The first layer of both nets. */
int irm_conv3x3_h_in_f32(const float* w, const float* x, long x_bs, void* y, long y_bs, const float* bias, int B, int Ci,
                         int Co, int H, int W, int relu1, irm_stream_t stream);
/* irm_conv3x3_h_f16: x, y (and res) fp16 channel-last, Ci, Co in {64, 128}; one v_mfma_f32_16x16x32_f16 per k-step,
 * fp32 accumulation; the halo tile arrives by LDS-DMA straight into the operand image (no conversion pass), border
 * pixels read a zero page.  Epilogue in fp32: v = acc * inv_scale + bias[co]; if relu1: v = max(v, 0); res_mode 1:
 * v += res (REDNet's skips); if relu2: v = max(v, 0).
 * wp [Ci/64 stages][9 taps][Co/16][2 k-steps][64 lanes][8 halves]: lane = 16 g + m, half j of (stage, tap, mtile, ks) =
 * RNE_fp16(W[16 mtile + m][64 stage + 32 ks + 8 g + j][tap] * s), s a power of two with max|W| s in [2^13, 2^14) (small
 * BN-merged weights stay out of the fp16 subnormals); inv_scale = 1 / s, applied in fp32 (exact). */
int irm_conv3x3_h_f16(const void* wp, float inv_scale, const void* x, long x_bs, void* y, long y_bs, const void* res,
                      long r_bs, const float* bias, int B, int Ci, int Co, int H, int W, int relu1, int res_mode,
                      int relu2, irm_stream_t stream);
/* irm_conv3x3_h_out_f32: x fp16 channel-last, Ci in {64, 128} -> y fp32 planar [B][Co <= 3][H][W] (not rounded to fp16);
 *   v = conv(x)[co] + bias[co] (fp32 FMAs on the vector pipe); res_mode 1: v + res (REDNet's + x), 2: res - v (DnCNN's
 *   x - n), res fp32 planar like y.  w: the plain weight [Co][Ci][3][3] fp32 (device).  The last layer of both nets. */
int irm_conv3x3_h_out_f32(const float* w, const void* x, long x_bs, float* y, long y_bs, const float* res, long r_bs,
                          const float* bias, int B, int Ci, int Co, int H, int W, int res_mode, irm_stream_t stream);
