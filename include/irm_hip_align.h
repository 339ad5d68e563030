/* irm_hip_align.h - the aligned scoring protocol of beam-splitter pairs (RealBlur): one gain, a homography by the
 * forward additive ECC iteration, a bicubic warp of the prediction onto the target and PSNR / SSIM under the validity
 * mask of that warp.  An extension of the C ABI of irm_hip.h.
 *
 * Included by irm_hip.h at its end, inside its extern "C" block: include irm_hip.h, not this file (the return codes,
 * irm_stream_t and the conventions on pointers and streams are those of irm_hip.h).  The Python binding mirrors this
 * file one to one in _hip.SIGNATURES_ALIGN.  The arithmetic is this package's own statement of the published protocol
 * (parity with OpenCV / skimage is unpinned); it is stated once, operation by operation, in float64 numpy, in
 * irm_amd/align.py (DESIGN.md section 24 has the contract).
 *
 * Operands the three entry points share
 *   pred, target  the frames [H][W][3] where they lie: uint8, or 16-bit words with is_u16 = 1 (peak 255 or 65535).
 *   H, W          both at least 11 (one SSIM window) and H W 3 below 2^31.
 *   gain          one fp64 in DEVICE memory: sum(target pred) / sum(pred pred) over the integer codes.
 *   map           nine fp64 in DEVICE memory, the 3 x 3 homography row by row; map[8] stays 1.  A target pixel (x, y)
 *                 reads the prediction at ((m0 x + m1 y) + m2, (m3 x + m4 y) + m5) / ((m6 x + m7 y) + 1).
 *   status        one int in DEVICE memory: 0 = fine, 1 = failed.  Every kernel of irm_ecc_iterate reads it first and
 *                 does nothing once it is set.
 *   ws            8-byte aligned DEVICE workspace of ws_words words of 8 bytes; each entry states its minimum.
 * fp64 and workspace pointers are 8-byte aligned, float planes 4-byte aligned, 16-bit frames 2-byte aligned.  Every sum
 * is made per workgroup in a fixed order, left in a workspace slot of its own and finished in a fixed order by one
 * workgroup: no atomics, no barrier across workgroups, results bitwise the same on every call.  Null pointers (where
 * not marked optional), sizes out of range and a workspace below the minimum return IRM_EINVAL before any HIP call. */
#pragma once

/* Gain and the four planes of the iteration.  gain as above (0 and status = 1 where sum(pred pred) is 0, else
 * status = 0).  With x = target / peak and zs = gain pred / peak in fp64: the grey planes (0.299 R + 0.587 G) + 0.114 B
 * of x (the template) and of zs (the image), each through the separable 5-tap Gaussian of sigma 1.1 (taps normalised to
 * 1, rows along x first, then along y, borders reflected without repeating the edge sample), rounded to float32:
 * tmpl and img [H][W].  gx, gy [H][W]: 0.5 (img[x + 1] - img[x - 1]) along each axis of the float32 img, the same
 * border rule, rounded to float32.  Four launches.
 *   ws   ws_words >= 2 ceil(3 H W / 4096) */
int irm_align_prepare(const void* pred, const void* target, int is_u16, int H, int W, double* gain, int* status,
                      float* tmpl, float* img, float* gx, float* gy, void* ws, long ws_words, irm_stream_t stream);

/* `iterations` (1 .. 10000) rounds of (accumulate, solve) enqueued on the stream, no host synchronisation between
 * them, from the map and the status that lie in device memory (the caller writes the identity and, without
 * irm_align_prepare, status 0).  Accumulate: a workgroup owns 16 x 64 target pixels; per pixel, in fp64, the source
 * position, the bilinear samples of img, gx and gy at that exact position (taps outside the frame read 0), the mask
 * (the position rounded to nearest lies inside the frame) and the Jacobian row; the workgroup leaves 66 sums in
 * ws[66 b + k], b = tile_y ceil(W / 64) + tile_x:
 *   k = 0..5    n, sum I, sum T, sum I^2, sum T^2, sum I T
 *   k = 6..41   the upper triangle of J^T J, row by row
 *   k = 42..65  J^T I, J^T T, J^T 1 (eight each)
 * Solve (one workgroup): the slots summed in ascending b, the zero-mean quantities from them, the 8 x 8 Cholesky
 * factorisation, rho (written before the update), lambda and dp; dp is added to m0, m3, m6, m1, m4, m7, m2, m5 in that
 * order.  An empty mask, a Hessian that is not positive definite or lambda_d <= 0 sets status = 1 and leaves the map.
 *   rho  one fp64 in DEVICE memory: the correlation at the map BEFORE the last update; untouched by a failing round.
 *   ws   ws_words >= 66 ceil(H / 16) ceil(W / 64) */
int irm_ecc_iterate(const float* tmpl, const float* img, const float* gx, const float* gy, int H, int W, int iterations,
                    double* map, double* rho, int* status, void* ws, long ws_words, irm_stream_t stream);

/* The final warp and the scores for a gain and a map in device memory.  Per target pixel in fp64: the source position,
 * cr = 1 where it, rounded to nearest (half to even), lies inside the frame; q = rint(32 position), the 4 x 4 bicubic
 * sample (A = -0.75, 32-phase table) of zs at q >> 5 with phase q & 31, borders reflected with the edge sample repeated;
 * zr = sample cr, xr = x cr.  Two launches.
 *   out[9]  fp64: sum (xr - zr)^2; sum cr; the three per-channel sums of (SSIM map x cr) over the valid region
 *           (H - 10) x (W - 10), 11-tap Gaussian window of sigma 1.5, data range 1; the three sums of cr over that
 *           region; sum cr / (H W).
 *   status  optional: set to 1 where sum cr is 0, otherwise untouched.
 *   zr      optional float32 [H][W][3], cr optional uint8 [H][W]: the warped frame and its mask.
 *   ws      ws_words >= 6 ceil((H - 10) / 16) ceil((W - 10) / 32) */
int irm_aligned_metrics(const void* pred, const void* target, int is_u16, int H, int W, const double* gain,
                        const double* map, double* out, int* status, float* zr, unsigned char* cr, void* ws,
                        long ws_words, irm_stream_t stream);
