/* irm_hip_video.h - YUV video frames of every sampling structure and depth the pipeline takes (4:2:0, 4:2:2, 4:4:4 at
 * 8, 10 and 12 bit) to and from the float32 RGB frame, and their PSNR / SSIM per component: an extension of the C ABI of
 * irm_hip.h that generalises irm_hip_yuv.h and the YUV entry of irm_hip_metrics.h.
 *
 * Included by irm_hip.h at its end, inside its extern "C" block: include irm_hip.h, not this file (the return codes,
 * irm_stream_t and the conventions on pointers and streams are those of irm_hip.h).  The Python binding mirrors this
 * file one to one in _hip.SIGNATURES_VIDEO.  The reference has no YUV path; the arithmetic is this package's own and is
 * stated once, operation by operation, in tests/yuv_formats_model.py (DESIGN.md section 23 has the formulas).
 *
 * Operands the three entry points share, beyond those irm_hip_yuv.h describes (y, u, v, chroma_step, pitch_y, pitch_c,
 * matrix, full_range, siting, luma_only, rgb)
 *   sub_w, sub_h  the chroma sub-sampling: (2, 2) = 4:2:0, (2, 1) = 4:2:2, (1, 1) = 4:4:4.  The chroma planes are
 *                 [H / sub_h][W / sub_w]; pitch_c >= chroma_step W / sub_w in SAMPLES.
 *   depth         8, 10 or 12 bits per sample: uint8 samples at depth 8, 16-bit words otherwise.
 *   upper_bits    16-bit depths only: 1 = the code sits in the upper bits of its word (P010, P210, P412, ..:
 *                 code = word >> (16 - depth), stored as code << (16 - depth) with the low bits zero), 0 = the code is
 *                 the word.  Must be 0 for depth 8.
 *   H, W          positive, at most 2^20; W a multiple of sub_w and H a multiple of sub_h.
 * The constants are those of irm_hip_yuv.h with k = 2^(depth - 8) and top = 2^depth - 1.  With (2, 2) at depth 8 or 10
 * the two conversions are irm_yuv420_to_rgb_f32 and irm_rgb_f32_to_yuv420 bit for bit (the same kernels).
 * Null pointers, sizes that do not divide, unknown (sub_w, sub_h), depths and enum values return IRM_EINVAL before any
 * HIP call. */
#pragma once

/* planes -> rgb.  Chroma is up-sampled linearly on the integer codes, edges clamped: 4:2:0 as irm_yuv420_to_rgb_f32;
 * 4:2:2 horizontally only (siting 0: the sample itself on an even column, the mean of its two neighbours on an odd one;
 * siting 1: 3/4 of the nearer and 1/4 of the farther sample); 4:4:4 not at all (siting is checked and ignored).  The
 * up-sampled code is an integer number of sixteenths, exact in float32.  Then Y', Cb, Cr, R, G, B and the clip as in
 * irm_hip_yuv.h, every operation rounded separately.  One launch; a work item owns eight pixels of one row (4:2:2,
 * 4:4:4) or an 8 x 2 block (4:2:0). */
int irm_yuv_to_rgb_f32(const void* y, const void* u, const void* v, int chroma_step, long pitch_y, long pitch_c,
                       int sub_w, int sub_h, int depth, int upper_bits, int matrix, int full_range, int siting,
                       int luma_only, int H, int W, float* rgb, irm_stream_t stream);

/* rgb -> planes.  Y', Cb, Cr per pixel as irm_rgb_f32_to_yuv420; the chroma filter is that entry's for 4:2:0, for 4:2:2
 * its row filter alone (siting 1: (c[2i] + c[2i+1]) * 0.5; siting 0: ((c[2i-1] + (c[2i] + c[2i])) + c[2i+1]) * 0.25 with
 * c[-1] = c[0]) and none for 4:4:4; codes rint(clip(offset + range * value, 0, 2^depth - 1)), half to even.  Nothing
 * outside [H][W] of a plane is written. */
int irm_rgb_f32_to_yuv(const float* rgb, void* y, void* u, void* v, int chroma_step, long pitch_y, long pitch_c,
                       int sub_w, int sub_h, int depth, int upper_bits, int matrix, int full_range, int siting,
                       int luma_only, int H, int W, irm_stream_t stream);

/* The planes of one frame against the target's, per component, as irm_yuv420_metrics scores them (irm_hip_metrics.h:
 * the same two launches, fixed-order sums, no atomics; sse, ssim and ws are 8-byte aligned DEVICE pointers).
 *   step, pitch   per side as in irm_yuv420_metrics, with pitch_c >= step W / sub_w; the step is the same on both sides.
 *   H, W          H / sub_h and W / sub_w at least 7, so that a chroma plane holds one 7 x 7 window (H, W at least 7
 *                 with luma_only); W a multiple of sub_w, H of sub_h; at most 2^20.
 *   sse[3]        u64: the exact integer squared error of the codes of Y, U and V.
 *   ssim[3]       fp64: the SSIM of Y (H x W) and of U and V (H / sub_h x W / sub_w), data_range 255, 1023 or 4095.
 *                 The window moments are exact integers, 32-bit for depth 8 and 64-bit for depths 10 and 12
 *                 ((49 * 4095)^2 = 4.0e10).
 *   ws            ws_words >= 2 (t(H, W) + 2 t(H / sub_h, W / sub_w)) words of 8 bytes,
 *                 t(h, w) = ceil((h - 6) / 16) ceil((w - 6) / 192); 2 t(H, W) with luma_only. */
int irm_yuv_metrics(const void* pred_y, const void* pred_u, const void* pred_v, int pred_step, long pred_pitch_y,
                    long pred_pitch_c, const void* target_y, const void* target_u, const void* target_v,
                    int target_step, long target_pitch_y, long target_pitch_c, int sub_w, int sub_h, int depth,
                    int upper_bits, int luma_only, int H, int W, unsigned long long* sse, double* ssim, void* ws,
                    long ws_words, irm_stream_t stream);
