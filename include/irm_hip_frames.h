/* irm_hip_frames.h - float32 frames in the tiled-patch loop, an extension of the C ABI of irm_hip.h.
 *
 * Included by irm_hip.h at its end, inside its extern "C" block: include irm_hip.h, not this file (the return codes,
 * irm_stream_t and the conventions on pointers and streams are those of irm_hip.h).  The Python binding mirrors this
 * file one to one in _hip.SIGNATURES_FRAMES, next to _hip.SIGNATURES for irm_hip.h.
 *
 * The three entry points share one operand, `range`: three floats on the DEVICE, {lo, hi, mul}.  The reference takes
 * a float frame as it is, or divided by its maximum where that exceeds 1 (normalize, src/utils.py:159-171), and
 * returns np.clip(acc * max, min, max) (utils.py:450-454): lo = min, hi = mul = max of the frame.  A caller whose
 * frames are in [0, 1] by contract passes the constant {0, 1, 1}: nothing is divided and the result is clip(acc, 0, 1).
 * The kernels read `range` themselves, so the host never waits for the reduction. */
#pragma once

/* range[0] = min, range[1] = range[2] = max of the n floats at img (4-byte aligned; 16-byte loads from the first
 * 16-byte boundary on, scalar head and tail).  No atomics: per-workgroup partials go to ws, a second launch folds
 * them; min and max do not depend on the order, so for finite input the result is bitwise np.min / np.max on every
 * run.  Non-finite input is outside the contract (a NaN may or may not reach the result).  Workspace: ws_floats >=
 * 2048 is always enough; with less, fewer workgroups run (at least 2 floats). */
int irm_frame_minmax_f32(const float* img, long n, float* range, float* ws, long ws_floats, irm_stream_t stream);

/* irm_tile_extract for a float32 frame: img [H][W][C] float32 -> tiles [T][C][ph][pw], same indexing, reflect / zero
 * padding and noise (added in double, clipped to [0, 1], cast to float) as irm_tile_extract.  The value is
 * raw / range[1] (one correctly rounded fp32 division) where range[1] > 1, else raw. */
int irm_tile_extract_f32(const float* img, const float* range, const int* origins, const double* noise, float* tiles,
                         int H, int W, int C, int th, int tw, int ph, int pw, int T, int pad_zero,
                         irm_stream_t stream);

/* irm_window_blend_scaled with a float32 frame as the result: the same accumulation (tile order, separately rounded
 * multiply and add, division by max(weight sum, 1e-8)), then out[H scale][W scale][Co] float32 =
 * min(max(v * range[2], range[0]), range[1]), not rounded to any grid.  H, W, th, tw, ph, pw, ps and the origins are
 * in INPUT pixels, pred is [T][Cp][scale ph][scale pw], window [scale ps][scale ps]; scale in 1..8 (1: the plain
 * blend).  There is no target / squared-error operand. */
int irm_window_blend_f32(const float* pred, const int* origins, const float* window, float* out, const float* range,
                         int H, int W, int Co, int Cp, int th, int tw, int ph, int pw, int ps, int T, int scale,
                         irm_stream_t stream);
