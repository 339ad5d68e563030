/* irm_hip_resize.h - resize of frames to any size from per-axis tap tables, an extension of the C ABI of irm_hip.h.
 *
 * Included by irm_hip.h at its end, inside its extern "C" block: include irm_hip.h, not this file (the return codes,
 * irm_stream_t and the conventions on pointers and streams are those of irm_hip.h).  The Python binding mirrors this
 * file one to one in _hip.SIGNATURES_RESIZE.
 *
 * irm_imresize_bicubic (irm_hip.h) is the resize of the super-resolution protocol: bicubic, the factors 2, 3, 4 and
 * their reciprocals, integer frames.  irm_resize_taps takes the filter, the scale of each axis and the antialiasing
 * from the tables, so one kernel makes any output size with any separable filter; with the tables of
 * irm_imresize_bicubic it returns that entry's bits. */
#pragma once

/* K frames [K][H][W][C] interleaved, C = 1 or 3, DEVICE pointer:
 *   in_kind    0: uint8, 1: uint16 (2-byte aligned), 2: float32 (taken as it is; a frame in [0, 1] nominal).
 *   out        [K][OH][OW][C], every element is written:
 *   out_kind   0: the input's integer type - clamp to [0, 1], x 255 (65535) in fp32, round half to even (in_kind 2
 *                 returns IRM_EINVAL: there is no integer type to return to);
 *              1: float32, unrounded and unclamped (a bicubic or Lanczos result overshoots [0, 1]);
 *              2: float32 clamped to [0, 1].
 * Tables (DEVICE, built by the host in float64: resize.resize_taps): per axis and output coordinate P taps, wh [OH][PH]
 * / ww [OW][PW] float32 weights, each row normalised to sum 1, and ih / iw int32 source indices, 0-based and reflected
 * into the frame; PH and PW are independent, 1 <= P <= 128 and P <= the side it reads (one reflection must reach
 * every tap).  The source indices of the taps of any run of consecutive output columns must cover a contiguous range
 * of columns (reflection keeps them so).
 *   tow        output columns per workgroup: 8, 16, 32, 64 or 128.  A workgroup makes 8 rows x tow columns.
 *   ncol_max   the largest number of source columns the taps of any aligned run of tow output columns touch,
 *              1 <= ncol_max <= W.  The intermediate of a workgroup, 8 x ncol_max x C floats, stays in LDS: more than
 *              32768 bytes returns IRM_EINVAL (choose a narrower tow).
 * H, W <= 32768; OH, OW >= 1; OH OW C, OH PH and OW PW < 2^31; 1 <= K <= 65535.
 * Arithmetic: integer inputs v / 255 (or / 65535) in fp32; the H pass first, then the W pass, each tap sum an fp32 FMA
 * chain in ascending tap order.  A value depends on its own taps only, not on K, tow, the tiling or the run; no
 * atomics.  Indices are clamped to the frame and to the window: a wrong table or a short ncol_max gives wrong pixels,
 * never an access outside the operands.  Null pointers and bad arguments return IRM_EINVAL before any HIP call.  One
 * launch on the stream, nothing is allocated. */
int irm_resize_taps(const void* in, int in_kind, void* out, int out_kind, const float* wh, const int* ih,
                    const float* ww, const int* iw, int K, int H, int W, int C, int OH, int OW, int PH, int PW,
                    int tow, int ncol_max, irm_stream_t stream);

/* The store rule of out_kind 0 on its own, for a float32 frame that has no integer type of its own (the frame between
 * the stages of a chain): n float32 values (DEVICE) -> uint8 (is_u16 = 0) or uint16 (is_u16 = 1, 2-byte aligned):
 * clamp to [0, 1], x 255 (65535) in fp32, round half to even.  irm_resize_taps with out_kind 2 followed by this call
 * gives the bits of out_kind 0.  1 <= n; null pointers and bad arguments return IRM_EINVAL before any HIP call. */
int irm_unit_quantise(const float* in, void* out, int is_u16, long n, irm_stream_t stream);
