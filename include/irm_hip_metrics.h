/* irm_hip_metrics.h - PSNR / SSIM of float32 frames and of YUV 4:2:0 planes on the device, an extension of the C ABI of
 * irm_hip.h (irm_frame_metrics there scores uint8 / uint16 frames).
 *
 * Included by irm_hip.h at its end, inside its extern "C" block: include irm_hip.h, not this file (the return codes,
 * irm_stream_t and the conventions on pointers and streams are those of irm_hip.h).  The Python binding mirrors this
 * file one to one in _hip.SIGNATURES_METRICS.
 *
 * Both entry points compute, per frame or per plane,
 *   the squared error   the sum of (x - y)^2 over every value, and
 *   the SSIM            skimage's structural_similarity with its defaults, as irm_frame_metrics does: 7 x 7 uniform
 *                       window, K1 = .01, K2 = .03, sample covariance 49/48, mean over the (H-6) x (W-6) interior (and
 *                       over the channels of a float frame).
 * Output tiles are 16 rows x 192 values (pixels x channels); each leaves two 8-byte words in the workspace `ws`, and a
 * second launch sums them in a fixed order.  No atomics: a result is bitwise the same on every call, and for a float
 * frame whatever K.  Identical operands give SSIM exactly 1.0 and a squared error of exactly 0.
 * sse, ssim and ws are 8-byte aligned DEVICE pointers.  Null pointers and bad extents return IRM_EINVAL before any HIP
 * call; both entries enqueue two launches on the stream and allocate nothing. */
#pragma once

/* K prediction / target frames, contiguous float32 [K][H][W][C], 4-byte aligned.  C = 1 or 3; H, W >= 7;
 * 1 <= K <= 65535; H W C < 2^31; data_range > 0 and finite (c1 = (.01 data_range)^2, c2 = (.03 data_range)^2).
 *   sse[K]    fp64: the sum of (double(x) - double(y))^2, every square rounded to fp64, summed in a fixed order.
 *   ssim[K]   fp64.  The five window moments are summed in fp64, seven rows and then seven columns (a float32 product
 *             is exact in fp64).
 *   ws        ws_words >= 2 K ceil((H - 6) / 16) ceil((W - 6) / (192 / C)) words of 8 bytes.
 * Rows move in 16-byte pieces where W C % 4 == 0 and both frames are 16-byte aligned, element by element otherwise.
 * Non-finite values (NaN, infinities) are outside the contract: the results are then unspecified. */
int irm_frame_metrics_f32(const float* pred, const float* target, int K, int H, int W, int C, double data_range,
                          double* sse, double* ssim, void* ws, long ws_words, irm_stream_t stream);

/* The planes of one YUV 4:2:0 frame against the target's.  Each side is given as irm_yuv420_to_rgb_f32 takes its planes
 * (irm_hip_yuv.h): y [H][W], u and v [H/2][W/2], DEVICE pointers to uint8 samples (depth 8) or 16-bit words (depth 10)
 * aligned to the sample size; step = 1 planar (I420) or 2 interleaved (NV12, P010: v = u + 1 sample), the same on both
 * sides; pitch_y >= W and pitch_c >= step W / 2 in SAMPLES.  The two sides may have different pitches.  Nothing outside
 * [H][W] of a plane is read.
 *   depth      8 or 10.        is_p010   depth 10 only: 1 = the code is the word shifted right by six (its low six
 *                                        bits are ignored), 0 = the word itself.  Must be 0 for depth 8.
 *   luma_only  1 = Y alone: u, v are not read and may be null, entries 1 and 2 of sse and ssim are not written.
 *   H, W       even, at least 14 (a chroma plane must hold one 7 x 7 window; at least 8 with luma_only), at most 2^20.
 *   sse[3]     u64: the exact integer squared error of the codes of Y, U and V.
 *   ssim[3]    fp64: the SSIM of Y (H x W) and of U and V (H/2 x W/2), data_range 255 (depth 8) or 1023 (depth 10).
 *              The window moments are exact integers, 32-bit for depth 8 and 64-bit for depth 10.
 *   ws         ws_words >= 2 (t(H, W) + 2 t(H/2, W/2)) words of 8 bytes, t(h, w) = ceil((h - 6) / 16) ceil((w - 6) / 192);
 *              2 t(H, W) with luma_only.
 * One launch covers the tiles of all three components.  A plane moves in 16-byte pieces where step is 1 and its base
 * and pitch are 16-byte aligned, sample by sample otherwise. */
int irm_yuv420_metrics(const void* pred_y, const void* pred_u, const void* pred_v, int pred_step, long pred_pitch_y,
                       long pred_pitch_c, const void* target_y, const void* target_u, const void* target_v,
                       int target_step, long target_pitch_y, long target_pitch_c, int depth, int is_p010, int luma_only,
                       int H, int W, unsigned long long* sse, double* ssim, void* ws, long ws_words,
                       irm_stream_t stream);
