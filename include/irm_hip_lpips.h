/* irm_hip_lpips.h - the two kernels around the conv trunk of LPIPS v0.1 (net = 'alex'), an extension of the C ABI of
 * irm_hip.h: the frame front end and the distance head.  The trunk itself is irm_convkxk_f32, irm_pool3x3_f32 and the
 * dense 3x3 convs.
 *
 * Included by irm_hip.h at its end, inside its extern "C" block: include irm_hip.h, not this file (the return codes,
 * irm_stream_t and the conventions on pointers and streams are those of irm_hip.h).  The Python binding mirrors this
 * file one to one in _hip.SIGNATURES_LPIPS.
 * Null pointers, zero or negative sizes, overlapping rows, frames or maps, misaligned pointers and a short workspace
 * return IRM_EINVAL before any HIP call.  Nothing is allocated and the host is not synchronised. */
#pragma once

/* K frames [H][W][3] -> z [K][48][OH + 2][OW + 2] float32 planar, OH = (H - 7) / 4 + 1, OW = (W - 7) / 4 + 1:
 *   z[k][c 16 + i 4 + j][Y][X] = u_c(frame k at row 4 Y + i - 2, column 4 X + j - 2),   u_c(raw) = fma(raw, a_c, b_c)
 * in float32 with one rounding, and exactly 0 where that row or column lies outside the part of the frame that the
 * stride reaches (rows 0 .. min(H, 4 OH + 5) - 1, columns alike): this is the frame zero padded by 2 and folded
 * space-to-depth by 4.  An 11 x 11 convolution of stride 4 and padding 2 over u is the 3 x 3 stride-1 pad-0 convolution
 * over z with W3[o][c 16 + i 4 + j][p][q] = W12[o][c][4 p + i][4 q + j], W12 the 11 x 11 kernel zero extended to 12 x 12.
 * Rows and columns that no window reaches are never read.
 *   frames     DEVICE pointer; kind 0: uint8, 1: 16-bit words, 2: float32, aligned to its sample.  Row r of frame k
 *              starts at frames + k frame_stride + r pitch, both in SAMPLES: pitch >= 3 W and
 *              frame_stride >= (H - 1) pitch + 3 W, so a row-pitched frame is read where it lies; nothing outside
 *              [H][3 W] of a frame is read.  H, W >= 7; 1 <= K <= 65535; 3 H W < 2^31; OH + 2 <= 65535.
 *   a0..b2     the affine of the three channels, made by the host (in float64, rounded once).
 *   z          4-byte aligned; frame k at z + k z_bs floats, z_bs >= 48 (OH + 2) (OW + 2); every element of the
 *              [48][OH + 2][OW + 2] block of a frame is written and nothing else.
 * One launch. */
int irm_lpips_pack(const void* frames, int kind, int K, int H, int W, long pitch, long frame_stride, float a0, float a1,
                   float a2, float b0, float b1, float b2, float* z, long z_bs, irm_stream_t stream);

/* The distance of one tap for K pairs of feature maps.  f: 2 K maps [C][H][W] planar float32, map m at f + m f_bs
 * floats (f_bs >= C H W); maps 0 .. K - 1 are the predictions' and K .. 2 K - 1 the targets'.  lin: [C] float32.
 *   out[k out_stride] = 1 / (H W) sum_{y, x} sum_c lin[c] ( f_c / (n_f + 1e-10) - g_c / (n_g + 1e-10) )^2,   k < K,
 * f = map k, g = map K + k, n_f(y, x) = sqrt(sum_c f_c^2).  The difference is formed directly, in float32, as
 * f_c r_f - g_c r_g with r_f = 1 / (n_f + 1e-10) (never expanded into squares and a product), so identical maps give
 * exactly 0.0 and a pixel whose channels are all zero contributes 0; the channel sums, the pixel sum and the mean are
 * float64.  Bitwise reproducible: one partial per workgroup in ws, added in a fixed order by a second launch,
 * no atomics; a pair's value does not depend on K.
 *   1 <= K <= 65535; 1 <= C <= 4096; H, W >= 1; C H W < 2^31; out_stride >= 1 (in doubles).
 *   f, lin     4-byte aligned;  out, ws  8-byte aligned DEVICE pointers.
 *   ws         workspace of 8-byte words, ws_words >= K * ceil(H W / 64).
 * Two launches. */
int irm_lpips_head(const float* f, long f_bs, const float* lin, int K, int C, int H, int W, double* out,
                   long out_stride, void* ws, long ws_words, irm_stream_t stream);
