// Data movement of the x8 self-ensemble with partitioned forward (MaIR+, mairplus_model.py): the 8 dihedral
// variants of an image (augment, :119-130) cut into overlapping partitions ("chop and shave", one_img_test :12-55) in
// ONE pass, and the stitch of the partition interiors (:65-77, 103), the inverse transforms and the mean of the 8
// results (gather, :107-117) in ONE pass.  Both kernels are HBM streamers: every global access of a wave runs along a
// row (forwards or backwards); the four transposing variants turn their tile round in LDS (64 x 65 floats: the odd
// row stride keeps both the row-wise store and the column-wise load free of bank conflicts).
//
// Geometry comes from one int32 table on the device (irm_amd/ensemble.py builds and caches it per input shape):
//   rows 0..7      variant e:   {nh, nw, split_h, split_w, shave_h, shave_w, p0, 0}   (grid of the AUGMENTED image,
//                               its partitions are rows 8 + p0 + i * nw + j)
//   rows 8..8+P-1  partition p: {e, y0, x0, ph, pw, pix_off, 0, 0}                    (origin in the padded
//                               augmented image, extent, pixel offset of image 0's copy in the packed buffer)
// Variant e = vf + 2 hf + 4 tr: aug = transpose^tr(hflip^hf(vflip^vf(img))).  Packed buffers hold, for partition p
// and image b, a dense [C][ph][pw] block at float offset (pix_off + b ph pw) C (predictions: x scale^2, C = Co).
#include "irm_common.h"

#define ENS_TILE 64
#define ENS_LDS_STRIDE 65
#define ENS_ROWS_PER_THREAD 16      // 64 x 64 tile, 256 threads
#define ENS_TAB 8                   // ints per table row

struct ChopArgs {
    const float* src;   // [B][C][H][W]
    const int* tab;
    float* dst;         // packed partitions
    long dst_pixels;    // capacity of dst in pixels (floats / C)
    int B, C, H, W, P, tiles_x;
};

__global__ __launch_bounds__(256) void dihedral_chop_kernel(ChopArgs a) {
    __shared__ float tile[ENS_TILE * ENS_LDS_STRIDE];
    const int* t = a.tab + (8 + (int)blockIdx.y) * ENS_TAB;
    const int e = t[0], y0 = t[1], x0 = t[2], ph = t[3], pw = t[4], off = t[5];
    const int py0 = ((int)blockIdx.x / a.tiles_x) * ENS_TILE, px0 = ((int)blockIdx.x % a.tiles_x) * ENS_TILE;
    // a partition smaller than the grid's largest one; a table row that does not fit the buffer is not written
    if (py0 >= ph || px0 >= pw) return;
    if (e < 0 || e > 7 || y0 < 0 || x0 < 0 || off < 0 || (long)off + (long)a.B * ph * pw > a.dst_pixels) return;
    const int b = (int)blockIdx.z / a.C, c = (int)blockIdx.z % a.C;
    const bool vf = e & 1, hf = e & 2, tr = e & 4;
    const int ha = tr ? a.W : a.H, wa = tr ? a.H : a.W;       // extents of the augmented image
    const float* src = a.src + ((long)b * a.C + c) * a.H * a.W;
    float* dst = a.dst + ((long)off + (long)b * ph * pw) * a.C + (long)c * ph * pw;
    const int lane = threadIdx.x & 63, kq = threadIdx.x >> 6;
    // source pixel of partition pixel (py, px): origin, reflect pad (no edge repeat) of the augmented image, inverse
    // transposition, inverse flips; clamped, so that no table can make the read leave the plane
    auto source = [&](int py, int px) -> float {
        int ay = y0 + py, ax = x0 + px;
        ay = ay < ha ? ay : 2 * ha - 2 - ay;
        ax = ax < wa ? ax : 2 * wa - 2 - ax;
        int r = tr ? ax : ay, cc = tr ? ay : ax;
        r = min(max(r, 0), a.H - 1);
        cc = min(max(cc, 0), a.W - 1);
        return src[(long)(vf ? a.H - 1 - r : r) * a.W + (hf ? a.W - 1 - cc : cc)];
    };
    if (!tr) {
        const int px = px0 + lane;
        if (px >= pw) return;
#pragma unroll 4
        for (int it = 0; it < ENS_ROWS_PER_THREAD; ++it) {
            const int py = py0 + kq + 4 * it;
            if (py < ph) dst[(long)py * pw + px] = source(py, px);
        }
        return;
    }
    // transposing variants: a partition ROW runs along a source COLUMN.  Load with the lanes along the partition's
    // rows (consecutive source columns), store with the lanes along its columns.
#pragma unroll 4
    for (int it = 0; it < ENS_ROWS_PER_THREAD; ++it) {
        const int k = kq + 4 * it;
        const int py = py0 + lane, px = px0 + k;
        tile[k * ENS_LDS_STRIDE + lane] = (py < ph && px < pw) ? source(py, px) : 0.0f;
    }
    __syncthreads();
    const int px = px0 + lane;
    if (px >= pw) return;
#pragma unroll 4
    for (int it = 0; it < ENS_ROWS_PER_THREAD; ++it) {
        const int k = kq + 4 * it;
        const int py = py0 + k;
        if (py < ph) dst[(long)py * pw + px] = tile[lane * ENS_LDS_STRIDE + k];
    }
}

extern "C" int irm_dihedral_chop_f32(const float* src, const int* table, float* dst, long dst_pixels, int B, int C,
                                     int H, int W, int P, int max_ph, int max_pw, hipStream_t stream) {
    if (!src || !table || !dst || dst_pixels <= 0 || B <= 0 || C <= 0 || H <= 0 || W <= 0 || P <= 0) return IRM_EINVAL;
    if (max_ph <= 0 || max_pw <= 0 || P > 65535 || (long)B * C > 65535) return IRM_EINVAL;
    if (H > (1 << 20) || W > (1 << 20) || max_ph > (1 << 20) || max_pw > (1 << 20)) return IRM_EINVAL;
    const int tiles_x = (max_pw + ENS_TILE - 1) / ENS_TILE, tiles_y = (max_ph + ENS_TILE - 1) / ENS_TILE;
    ChopArgs a{src, table, dst, dst_pixels, B, C, H, W, P, tiles_x};
    hipLaunchKernelGGL(dihedral_chop_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)P, (unsigned)(B * C)),
                       dim3(256), 0, stream, a);
    return irm_launch_status();
}

// ---------------------------------------------------------------------------
struct MergeArgs {
    const float* pred;  // packed predictions, partition p / image b: [Co][s ph][s pw] at ((pix_off + b ph pw) s^2) Co
    const int* tab;
    float* out;         // [B][Co][s H][s W]
    long pred_pixels;   // capacity of pred in INPUT pixels (floats / (Co s^2))
    int B, Co, H, W, P, s;
};

// One axis of a variant's grid at output scale: n cells of `split`, partition i keeps `shave` more on each inner side.
struct EnsAxis {
    int n, split, shave;
    // cell of augmented coordinate v, from the hint i (the cell of a neighbouring pixel): no division per pixel
    __device__ __forceinline__ int cell(int v, int i) const {
        while (i + 1 < n && v >= (i + 1) * split) ++i;
        while (i > 0 && v < i * split) --i;
        return i;
    }
    __device__ __forceinline__ int first(int v) const { return min(max(v / split, 0), n - 1); }
    __device__ __forceinline__ int extent(int i) const { return split + (i > 0 ? shave : 0) + (i + 1 < n ? shave : 0); }
    __device__ __forceinline__ int local(int v, int i) const {          // the shaved offset (:69-76)
        return min(max(v - i * split + (i > 0 ? shave : 0), 0), extent(i) - 1);
    }
};

// One workgroup per 64 x 64 output tile of one (image, channel) plane.  The 8 members are added as the balanced tree
// ((m0 + m1) + (m2 + m3)) + ((m4 + m5) + (m6 + m7)) - a fixed order, and every partial sum of 8 EQUAL values is exact
// (2x, 4x, 8x), so an equivariant network gives back its single forward bit for bit - then x 0.125.
__global__ __launch_bounds__(256) void ensemble_merge_kernel(MergeArgs a) {
    __shared__ float tile[ENS_TILE * ENS_LDS_STRIDE];
    const int s = a.s, sH = s * a.H, sW = s * a.W;
    const int tiles_x = (sW + ENS_TILE - 1) / ENS_TILE;
    const int Y0 = ((int)blockIdx.x / tiles_x) * ENS_TILE, X0 = ((int)blockIdx.x % tiles_x) * ENS_TILE;
    const int b = (int)blockIdx.y / a.Co, c = (int)blockIdx.y % a.Co;
    const int lane = threadIdx.x & 63, kq = threadIdx.x >> 6;
    const long ss = (long)s * s;
    float total[ENS_ROWS_PER_THREAD], quad[ENS_ROWS_PER_THREAD], pair[ENS_ROWS_PER_THREAD];
#pragma unroll 1
    for (int e = 0; e < 8; ++e) {
        const int* g = a.tab + e * ENS_TAB;
        const EnsAxis rows{g[0], s * g[2], s * g[4]}, cols{g[1], s * g[3], s * g[5]};     // of the augmented image
        const int nw = g[1], p0 = g[6];
        const bool vf = e & 1, hf = e & 2, tr = e & 4;
        // lanes run along output X (plain variants) or output Y (transposing ones: the tile is turned in LDS); either
        // way they run along a ROW of the augmented prediction, forwards or backwards
        const int lo = tr ? Y0 + lane : X0 + lane;                    // output coordinate of this lane
        const bool lane_ok = lo < (tr ? sH : sW);
        const int ax = tr ? (vf ? sH - 1 - lo : lo) : (hf ? sW - 1 - lo : lo);
        const int j = cols.first(lane_ok ? ax : 0);
        const int lx = cols.local(ax, j), pw = cols.extent(j);
        int i = -1;
#pragma unroll
        for (int it = 0; it < ENS_ROWS_PER_THREAD; ++it) {
            const int k = kq + 4 * it;
            const int ko = tr ? X0 + k : Y0 + k;                      // output coordinate along the other axis
            const bool ok = lane_ok && ko < (tr ? sW : sH);
            float v = 0.0f;
            if (ok) {
                const int ay = tr ? (hf ? sW - 1 - ko : ko) : (vf ? sH - 1 - ko : ko);
                i = i < 0 ? rows.first(ay) : rows.cell(ay, i);
                const int ly = rows.local(ay, i), ph = rows.extent(i);
                const int p = p0 + i * nw + j;
                if (p >= 0 && p < a.P) {
                    const long off = a.tab[(8 + p) * ENS_TAB + 5];
                    // ph, pw are at output scale here: (off + b ph pw / s^2) s^2 = off s^2 + b ph pw
                    if (ph > 0 && pw > 0 && off >= 0 && off + ((long)a.B * ph * pw) / ss <= a.pred_pixels)
                        v = a.pred[(off * ss + (long)b * ph * pw) * a.Co + ((long)c * ph + ly) * pw + lx];
                }
            }
            if (!tr) {
                if (e & 1) pair[it] += v; else pair[it] = v;
            } else {
                tile[k * ENS_LDS_STRIDE + lane] = v;
            }
        }
        if (tr) {
            __syncthreads();
#pragma unroll
            for (int it = 0; it < ENS_ROWS_PER_THREAD; ++it) {
                const float v = tile[lane * ENS_LDS_STRIDE + kq + 4 * it];
                if (e & 1) pair[it] += v; else pair[it] = v;
            }
            __syncthreads();
        }
        if (e & 1) {
#pragma unroll
            for (int it = 0; it < ENS_ROWS_PER_THREAD; ++it) {
                if (e & 2) quad[it] += pair[it]; else quad[it] = pair[it];
            }
        }
        if ((e & 3) == 3) {
#pragma unroll
            for (int it = 0; it < ENS_ROWS_PER_THREAD; ++it) {
                if (e & 4) total[it] += quad[it]; else total[it] = quad[it];
            }
        }
    }
    const int X = X0 + lane;
    if (X >= sW) return;
    float* out = a.out + ((long)b * a.Co + c) * sH * sW;
#pragma unroll
    for (int it = 0; it < ENS_ROWS_PER_THREAD; ++it) {
        const int Y = Y0 + kq + 4 * it;
        if (Y < sH) out[(long)Y * sW + X] = total[it] * 0.125f;
    }
}

extern "C" int irm_ensemble_merge_f32(const float* pred, const int* table, float* out, long pred_pixels, int B, int Co,
                                      int H, int W, int P, int scale, hipStream_t stream) {
    if (!pred || !table || !out || pred_pixels <= 0 || B <= 0 || Co <= 0 || H <= 0 || W <= 0 || P <= 0) return IRM_EINVAL;
    if (scale < 1 || scale > 4 || P > 65535 || (long)B * Co > 65535) return IRM_EINVAL;
    if ((long)H * scale > (1L << 20) || (long)W * scale > (1L << 20)) return IRM_EINVAL;   // int coordinates in the kernel
    const long tiles = (long)((H * scale + ENS_TILE - 1) / ENS_TILE) * ((W * scale + ENS_TILE - 1) / ENS_TILE);
    if (tiles >= (1L << 31)) return IRM_EINVAL;
    MergeArgs a{pred, table, out, pred_pixels, B, Co, H, W, P, scale};
    hipLaunchKernelGGL(ensemble_merge_kernel, dim3((unsigned)tiles, (unsigned)(B * Co)), dim3(256), 0, stream, a);
    return irm_launch_status();
}
