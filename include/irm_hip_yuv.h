/* irm_hip_yuv.h - YUV 4:2:0 video frames (I420, NV12, P010) to and from the float32 RGB frame of the device pipeline,
 * an extension of the C ABI of irm_hip.h.
 *
 * Included by irm_hip.h at its end, inside its extern "C" block: include irm_hip.h, not this file (the return codes,
 * irm_stream_t and the conventions on pointers and streams are those of irm_hip.h).  The Python binding mirrors this
 * file one to one in _hip.SIGNATURES_YUV.  The reference has no YUV path; the arithmetic is this package's own and is
 * stated once, operation by operation, in tests/yuv_model.py (DESIGN.md section 16 has the formulas).
 *
 * Operands the two entry points share
 *   y, u, v       the luma plane [H][W] and the two chroma planes [H/2][W/2], DEVICE pointers to uint8 samples
 *                 (depth 8) or to 16-bit words (depth 10), aligned to the sample size.  u and v are not read or
 *                 written with luma_only and may then be null.
 *   chroma_step   distance in samples between two neighbours of one chroma plane: 1 planar (I420), 2 interleaved
 *                 (NV12, P010: v = u + 1 sample, one UV plane [H/2][W/2][2]).
 *   pitch_y,      row pitch in SAMPLES of the luma plane and of the chroma planes (decoder surfaces are pitched):
 *   pitch_c       pitch_y >= W and pitch_c >= chroma_step W / 2, else IRM_EINVAL.  Nothing is written outside [H][W]
 *                 of a plane: the pitch padding is the caller's.
 *   depth         8 or 10 bits per sample.
 *   upper_bits    depth 10 only: 1 = the code sits in the upper bits of its word (P010: code = word >> 6, stored as
 *                 code << 6 with the low bits zero), 0 = in the lower bits.  Must be 0 for depth 8.
 *   matrix        0 = BT.601 (Kr 0.299, Kb 0.114), 1 = BT.709 (Kr 0.2126, Kb 0.0722).
 *   full_range    0 = limited range (y 16..235, chroma 16..240, times 2^(depth-8)), 1 = full range (0 .. 2^depth - 1).
 *   siting        0 = left (chroma co-sited with the even luma column, midway between the two rows: MPEG-2 / H.264),
 *                 1 = centre (chroma in the middle of its 2 x 2 luma block: JPEG / MPEG-1).
 *   luma_only     1 = the float frame is [H][W][1] and holds Y' alone; the chroma planes are not touched.
 *   H, W          even, positive, at most 2^20.
 *   rgb           the float32 frame [H][W][3] (or [H][W][1]), contiguous, 4-byte aligned.  It moves in 16-byte pieces
 *                 where W % 4 == 0 and the pointer is 16-byte aligned, element by element otherwise; the planes move
 *                 in pieces of eight luma / four chroma samples where pointer and pitch are aligned to such a piece.
 * Null pointers, odd or non-positive sizes and unknown enum values return IRM_EINVAL before any HIP call. */
#pragma once

/* planes -> rgb: chroma up-sampled linearly on the integer codes (edges clamped; weights in sixteenths, exact),
 * Y' = (y - y0) / yr, Cb = (u - c0) / cr, Cr = (v - c0) / cr, R = Y' + 2(1-Kr) Cr, B = Y' + 2(1-Kb) Cb,
 * G = (Y' - 2 Kb (1-Kb) / Kg Cb) - 2 Kr (1-Kr) / Kg Cr, every operation rounded separately, clipped to [0, 1]. */
int irm_yuv420_to_rgb_f32(const void* y, const void* u, const void* v, int chroma_step, long pitch_y, long pitch_c,
                          int depth, int upper_bits, int matrix, int full_range, int siting, int luma_only,
                          int H, int W, float* rgb, irm_stream_t stream);

/* rgb -> planes: Y' = (Kr R + Kg G) + Kb B, Cb = (B - Y') / (2(1-Kb)), Cr = (R - Y') / (2(1-Kr)) per pixel, chroma
 * filtered to its site (centre: the mean of the 2 x 2 block; left: (l + 2m + r) / 4 on each of the two rows, centred on
 * the even column with the edge clamped, then their mean), codes rint(clip(y0 + yr Y', 0, 2^depth - 1)) and
 * rint(clip(c0 + cr C, 0, 2^depth - 1)), half to even.  Inputs outside [0, 1] are legal: the codes are clipped. */
int irm_rgb_f32_to_yuv420(const float* rgb, void* y, void* u, void* v, int chroma_step, long pitch_y, long pitch_c,
                          int depth, int upper_bits, int matrix, int full_range, int siting, int luma_only,
                          int H, int W, irm_stream_t stream);
