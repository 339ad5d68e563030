/* irm_hip_noise.h - the noise level of integer frames from the diagonal Haar detail band, an extension of the C ABI of
 * irm_hip.h.
 *
 * Included by irm_hip.h at its end, inside its extern "C" block: include irm_hip.h, not this file (the return codes,
 * irm_stream_t and the conventions on pointers and streams are those of irm_hip.h).  The Python binding mirrors this
 * file one to one in _hip.SIGNATURES_NOISE.
 *
 * The statistic, per channel of a frame, on the samples v = word >> shift:
 *   blocks     the floor(H/2) x floor(W/2) non-overlapping 2 x 2 blocks (a trailing odd row or column is never read);
 *              for the block at (2i, 2j): a = v[2i][2j], b = v[2i][2j+1], c = v[2i+1][2j], e = v[2i+1][2j+1] and
 *              d = |a - b - c + e|;
 *   counted    a block counts unless min(a, b, c, e) <= sat_lo or max(a, b, c, e) >= sat_hi;
 *   stats      four int64 values (n, m, below, at): n the number of counted blocks, m the lower median of their d (the
 *              order statistic with 0-based index (n - 1) / 2), below the number of counted d < m and at the number of
 *              counted d == m.  n == 0 gives (0, 0, 0, 0).
 * Donoho's estimate sigma = median / 0.6745 follows on the host from these integers (noise.py).  The median is exact: it
 * is read off histograms of d (one of 512 bins for uint8 samples, two levels of 512 bins for 16-bit words), whose
 * counts are summed with integer atomics, so a result is the same on every call and whatever K. */
#pragma once

/* K frames [H][W][C] of uint8 samples (is_u16 = 0) or 16-bit words (is_u16 = 1, 2-byte aligned), DEVICE pointer.
 * Row r of frame k starts at frames + k frame_stride + r pitch, both in SAMPLES: pitch >= W C and
 * frame_stride >= (H - 1) pitch + W C, so a row-pitched plane (C = 1) is read where it lies; nothing outside [H][W C] of
 * a frame is read.  C = 1 or 3; H, W >= 2; 1 <= K <= 65535; H W C < 2^31.
 *   shift      0 <= shift < 8 (uint8) or 16 (16-bit words): 6 for the Y plane of P010.
 *   sat_lo     >= -1, sat_hi > sat_lo: see `counted` above (-1 and 2 peak + 1 count every block).
 *   stats      [K][C][4] int64, 8-byte aligned DEVICE pointer; every element is written.
 *   ws         8-byte aligned DEVICE workspace, ws_words >= 4098 K C words of 8 bytes.
 * Rows move in 16-byte pieces where frames, pitch and (for K > 1) frame_stride are 16-byte aligned, sample by sample
 * otherwise.  Null pointers and bad arguments return IRM_EINVAL before any HIP call.  Three launches (uint8) or five
 * (16-bit words) are enqueued on the stream, with no host synchronisation; nothing is allocated. */
int irm_noise_hh_stats(const void* frames, int is_u16, int K, int H, int W, int C, long pitch, long frame_stride,
                       int shift, int sat_lo, int sat_hi, long long* stats, void* ws, long ws_words,
                       irm_stream_t stream);
