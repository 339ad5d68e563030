/* irm_hip_gram.h - the Gram pass that runs the depth-wise conv of q, k itself, an extension of the C ABI of irm_hip.h.
 *
 * Included by irm_hip.h at its end, inside its extern "C" block: include irm_hip.h, not this file (the return codes,
 * irm_stream_t and the conventions on pointers, streams and batch strides are those of irm_hip.h).  The Python binding
 * mirrors this file one to one in _hip.SIGNATURES_GRAM, next to _hip.SIGNATURES for irm_hip.h. */
#pragma once

/* irm_dw_gram_cm_f16x3_f32 (dw_gram.hip): the depth-wise 3x3 conv of q, k inside the Gram pass, for the levels whose 1x1 conv
 * is a GEMM of its own (C = 192, 384: C / heads == 48).  qkv: the RAW planar output of the qkv GEMM, [B][>= 2C][H][W] with
 * batch stride bs (q channels [0, C), k channels [C, 2C); zero padding outside the image, bias included); taps [2C][9] and
 * bias [2C] (or NULL): q, k rows of qkv_dwconv; gscale [2C]: the powers of two of irm_mdta_gram_f16x3_f32.  dw(q), dw(k) are
 * never written: per chunk of 4 consecutive 8 x 32 tiles of one (image, head) one partial record
 * [48 x 48 Gram | 48 |q|^2 | 48 |k|^2] goes to part [B][heads][H W / 1024][2400] (the format of irm_mdta_gram_*:
 * irm_mdta_finalize_* reduces it with nchunk = H W / 1024).  The chunks are fixed sets of tiles of one image, so the result
 * does not depend on the batch.  H % 8 == 0, W % 32 == 0, (H / 8) (W / 32) % 4 == 0, bs % 4 == 0, qkv and gscale 16-byte
 * aligned, 3 C H W < 2^30.  Replaces irm_dwconv3x3_f32 on q, k + irm_mdta_gram_f16x3_f32 (restormer.py:106, 116-121). */
int irm_dw_gram_cm_f16x3_f32(const float* qkv, long bs, const float* taps, const float* bias, const float* gscale, float* part,
                             int B, int C, int heads, int H, int W, irm_stream_t stream);
