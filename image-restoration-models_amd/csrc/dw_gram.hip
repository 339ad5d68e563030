// The q, k depth-wise 3x3 conv INSIDE the Gram pass, for the C >= 192 levels (48 channels per head):
//
//   part[(b, head, chunk)] = partial G = dw(q) dw(k)^T, |dw(q)|^2, |dw(k)|^2      (restormer.py:116-121, before the softmax)
//
// On these levels the 1x1 conv is a GEMM of its own (gemm_ps.hip) that leaves qkv planar in HBM.  dw(q), dw(k) exist only to be
// reduced to a 48 x 48 Gram per head: written once by the depth-wise kernel, read once by the Gram pass.  Here raw q, k are read
// once, with the 1-pixel halo of an 8 x 32 tile, the stencil runs out of LDS with the CHANNEL on the lane, and its outputs ARE
// the fragments of the Gram MFMA - the back half of qkv_cm_kernel<2, true> (fused_qkv_cm.hip), whose image layout, stencil
// mapping and Gram part (gram_cm.h) this kernel shares; the front half - the image filled by MFMAs there - is a fill from HBM.
//
//   work      an item is (image, head, 8 x 32 tile); a persistent workgroup walks whole chunks of QC_NCH consecutive tiles of ONE
//             (image, head) and emits one record per chunk: a record covers the same pixels whatever the batch.  Consecutive
//             chunks go to the workgroups of one XCD, so that neighbouring tiles' halos meet in its L2.
//   stages    the head's 96 channels (48 q, 48 k) pass in three stages of 32: q 0-31 | q 32-47, k 0-15 | k 16-47, through two
//             channel-major images [32 channels][10 rows x 36 slots], alternating.  A chunk runs STAGE-major: the 32 channels of
//             a stage for each of its tiles, then the next 32 (the q operands of all QC_NCH tiles stay in registers, 96 of them).
//   fill      register staged: a thread owns up to 6 of the 2880 16-byte pieces (32 channels x 10 halo rows x 9 pieces) of a
//             stage.  The halo row starts one pixel before a 16-byte boundary of the plane, the image rows are aligned for the
//             stencil's ds_read_b128: the global loads are the 4-byte aligned ones.  Every load stays inside the plane: rows
//             outside the image are loaded from the nearest row and replaced by zeros (the reference zero-pads qkv, bias
//             included), the first piece of a row at the left border and the last one at the right border load the nearest
//             whole piece and shift.  The loads of stage s + 1 (across the item and chunk boundary too) are requested before the
//             stencil of stage s and parked in the other image behind it: one barrier per stage.
//   stencil   wave w owns output row w, lane (i, g) channel i of a 16-channel tile and the pixels 8 g .. 8 g + 7; the 9 taps +
//             bias of the head's 96 channels sit in LDS ([10][96], rewritten per chunk).
//   Gram      gram_cm.h: scaled by the channel's power of two, fp16 hi/lo split, q_lo k_hi + q_hi k_lo + q_hi k_hi onto the
//             wave's 9 accumulator tiles; at the end of a chunk the 8 waves' partials meet in LDS (the image area) in wave order.
#include "irm_common.h"
#include "gram_cm.h"

struct DgArgs {
    const float* qkv; long bs;                   // [B][>= 2C][H][W] planar: q channels [0, C), k channels [C, 2C)
    const float* taps;                           // [2C][9]
    const float* bias;                           // [2C] or null
    const float* gscale;                         // [2C] power-of-two operand scales of q, k (_hip.gram_scales)
    float* part;                                 // [B heads][cpi][QC_REC]
    int C, heads, H, W;
    int tiles_x, cpi, units, gpx;                // tiles per row, chunks per (image, head), chunks in all, workgroups per XCD
};

constexpr int DG_PIECES = 32 * (QC_TH + 2) * 9;  // 16-byte pieces of a stage
constexpr int DG_PF = (DG_PIECES + 511) / 512;   // per thread (6)
constexpr int DG_TAP_OFF = 2 * QC_IMG;           // [10][96] floats behind the two images
constexpr int DG_LDS = DG_TAP_OFF + 10 * 96 * 4;
typedef float dg_f4u __attribute__((ext_vector_type(4), aligned(4)));

__global__ __launch_bounds__(512) void dw_gram_kernel(DgArgs a) {
    static_assert(8 * QC_REC * 4 <= 2 * QC_IMG, "the chunk-end reduction fits in the image area");
    static_assert(15 * 16 + QC_SLOTS * 4 <= QC_CS, "row + phase shift inside the row stride");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    irm_lc* lds = (irm_lc*)smem;

    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, r = lane & 15;
    const unsigned plane = (unsigned)(a.H * a.W);
    const int per = (a.units + 7) >> 3;
    const int xcd = blockIdx.x & 7, pos = blockIdx.x >> 3;
    auto unit_of = [&](int k) {
        const int i = k * a.gpx + pos, u = xcd * per + i;
        return i < per && u < a.units ? u : a.units;
    };
    int k = 0, unit = unit_of(0);
    if (unit >= a.units) return;

    // ---- the pieces of this thread: piece e = tid + 512 j is (channel e / 90, halo row (e % 90) / 9, piece e % 9); the threads
    // beyond the last piece repeat it (the same value to the same place)
    unsigned pdst[DG_PF], pdesc[DG_PF];          // byte offset inside an image; channel | halo row << 8 | piece << 16
#pragma unroll
    for (int j = 0; j < DG_PF; ++j) {
        const int e = min(tid + 512 * j, DG_PIECES - 1);
        const int ch = e / 90, row = (e % 90) / 9, pc = e % 9;
        pdesc[j] = (unsigned)(ch | row << 8 | pc << 16);
        pdst[j] = qc_row(ch) + (unsigned)((row * QC_PITCH + 4 * pc) * 4);
    }

    // a stage in flight: the raw pieces and what they need on their way into the image
    f32x4 pv[DG_PF];
    unsigned prowok = 0;                         // bit j: the piece's halo row lies inside the image
    bool pleft = false, pright = false;          // the tile touches the left / right border
    auto request = [&](int u, int t, int s) {
        const int bh = u / a.cpi, tile = (u - bh * a.cpi) * QC_NCH + t;
        const int b = bh / a.heads, head = bh - b * a.heads;
        const int ty0 = (tile / a.tiles_x) * QC_TH, tx0 = (tile % a.tiles_x) * QC_TW;
        const float* src = a.qkv + (long)b * a.bs;
        pleft = tx0 == 0;
        pright = tx0 + QC_TW == a.W;
        prowok = 0;
#pragma unroll
        for (int j = 0; j < DG_PF; ++j) {
            // (opaque: otherwise the compiler hoists every stage's address arithmetic out of the tile loop and spills it)
            const unsigned d = irm_opaque(pdesc[j]);
            const int pc = (int)(d >> 16);
            const int cc = 32 * s + (int)(d & 255);                                // 0 .. 95: q 0-47, k 0-47 of the head
            const int ch = head * 48 + (cc < 48 ? cc : a.C + cc - 48);
            const int gy = ty0 - 1 + (int)((d >> 8) & 255);
            if (gy >= 0 && gy < a.H) prowok |= 1u << j;
            // columns tx0 - 1 + 4 p .. + 3; the first piece starts at column tx0 on the left border, the last one (two columns
            // used) at tx0 + 28 on the right border
            const int gx = tx0 - 1 + 4 * pc + ((pc == 0 && pleft) ? 1 : 0) - ((pc == 8 && pright) ? 3 : 0);
            const unsigned off = (unsigned)ch * plane + (unsigned)(min(max(gy, 0), a.H - 1) * a.W + gx);
            pv[j] = *reinterpret_cast<const dg_f4u*>(src + off);
        }
    };
    auto park = [&](unsigned img) {              // img: byte offset of the image
#pragma unroll
        for (int j = 0; j < DG_PF; ++j) {
            f32x4 v = pv[j];
            const int pc = (int)(irm_opaque(pdesc[j]) >> 16);
            if (pc == 0 && pleft) v = (f32x4){0.f, v[0], v[1], v[2]};
            if (pc == 8 && pright) v = (f32x4){v[3], 0.f, 0.f, 0.f};
            if (!((prowok >> j) & 1)) v = (f32x4){0.f, 0.f, 0.f, 0.f};
            irm_st<f32x4>(lds, pdst[j] + img, 0, v);
        }
    };
    // taps + bias of the head's 96 channels: [t][cc]
    auto put_taps = [&](int u) {
        const int bh = u / a.cpi, head = bh % a.heads;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int e = tid + 512 * j;
            if (e < 960) {
                const int t = e / 96, cc = e - 96 * t;
                const int ch = head * 48 + (cc < 48 ? cc : a.C + cc - 48);
                const float v = t < 9 ? a.taps[ch * 9 + t] : (a.bias ? a.bias[ch] : 0.f);
                irm_st<float>(lds, (unsigned)(DG_TAP_OFF + e * 4), 0, v);
            }
        }
    };

    QcGram gram;
    qc_gram_clear(gram);
    const unsigned vrow0 = qc_row(r) + (unsigned)((wave * QC_PITCH + 8 * g) * 4);
    const unsigned vrow1 = qc_row(16 + r) + (unsigned)((wave * QC_PITCH + 8 * g) * 4);
    // (the tap table lies beyond the 16-bit offset field of the DS instructions: its base goes into the address register)
    const unsigned vtap = irm_opaque((unsigned)(DG_TAP_OFF + r * 4));

    put_taps(unit);
    request(unit, 0, 0);
    park(0);
    __syncthreads();
    for (;;) {
        const int bh = unit / a.cpi;
        const int head = bh % a.heads;
        const float* sq = a.gscale + head * 48;
        const float* sk = a.gscale + a.C + head * 48;
        const int nunit = unit_of(k + 1);
        float gsc[6];
#pragma unroll
        for (int u = 0; u < 6; ++u) gsc[u] = (u < 3 ? sq : sk)[16 * (u % 3) + r];
        irm_h8 gqh[QC_NCH][3], gql[QC_NCH][3];   // the wave's q tiles of the chunk's tiles as MFMA operands
        // STAGE-major over the chunk: the 32 channels of a stage for tile 0 .. QC_NCH - 1, then the next 32.  A tile's
        // left / right halo columns lie in the 128-byte lines of its neighbours, which are the chunk's previous / next tile
        // where the image is QC_NCH tiles wide: one stage later those lines are still in L2 (tile-major they were three
        // stages = the whole L2 away and came from HBM again).  Every accumulator still sees the tiles in the order 0, 1, ...
        irm_for<3>([&](auto SC) {
            irm_for<QC_NCH>([&](auto TC) {
                constexpr int s = decltype(SC)::value, t = decltype(TC)::value;
                constexpr bool last = s == 2 && t + 1 == QC_NCH;
                constexpr int IMG = ((s * QC_NCH + t) & 1) * QC_IMG, NIMG = QC_IMG - IMG;
                static_assert((3 * QC_NCH) % 2 == 0, "a chunk starts in image 0");
                // ---- request the next stage (the chunk's next tile, its next 32 channels, the next chunk's first stage)
                const bool more = !last || nunit < a.units;
                if (more) {
                    if constexpr (t + 1 < QC_NCH) request(unit, t + 1, s);
                    else if constexpr (s < 2) request(unit, 0, s + 1);
                    else request(nunit, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
                // ---- stencil + Gram of the stage's two 16-channel tiles
                irm_for<2>([&](auto HC) {
                    constexpr int hct = decltype(HC)::value, U = 2 * s + hct;
                    const unsigned vr = hct ? vrow1 : vrow0;
                    f32x4 sp0[3], sp1[3];
                    irm_v2 sp2[3];
                    float stap[10];
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy) {
                        sp0[dy] = irm_ld<f32x4>(lds, vr, IMG + dy * QC_PITCH * 4);
                        sp1[dy] = irm_ld<f32x4>(lds, vr, IMG + dy * QC_PITCH * 4 + 16);
                        sp2[dy] = irm_ld<irm_v2>(lds, vr, IMG + dy * QC_PITCH * 4 + 32);
                    }
#pragma unroll
                    for (int tp = 0; tp < 10; ++tp) stap[tp] = irm_ld<float>(lds, vtap, (tp * 96 + 16 * U) * 4);
                    float o[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = stap[9];
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy) {
                        const float P[10] = {sp0[dy][0], sp0[dy][1], sp0[dy][2], sp0[dy][3], sp1[dy][0], sp1[dy][1], sp1[dy][2],
                                             sp1[dy][3], sp2[dy][0], sp2[dy][1]};
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) {
                            const float tp = stap[dy * 3 + dx];
#pragma unroll
                            for (int e = 0; e < 8; ++e) o[e] = fmaf(tp, P[e + dx], o[e]);
                        }
                    }
                    qc_gram_unit<U>(gram, gqh[t], gql[t], o, gsc[U]);
                    // (pin the squared norms here: otherwise the compiler sinks their FMA chains to the end of the chunk and
                    // keeps every unit's stencil outputs alive until then)
                    irm_tie(gram.nq[0], gram.nq[1], gram.nq[2], gram.nk[0], gram.nk[1], gram.nk[2]);
                    __builtin_amdgcn_sched_barrier(0);
                });
                if constexpr (last) {
                    // ---- end of the chunk: every wave is done with the images, which take the 8 partial records
                    __syncthreads();
                    qc_gram_flush(gram, smem, sq, sk, a.part, (long)unit, wave, g, r);
                    __syncthreads();
                    if (more) put_taps(nunit);
                }
                if (more) park((unsigned)NIMG);
                __syncthreads();
            });
        });
        if (nunit >= a.units) break;
        unit = nunit;
        ++k;
    }
}

// Header: include/irm_hip_gram.h.
extern "C" int irm_dw_gram_cm_f16x3_f32(const float* qkv, long bs, const float* taps, const float* bias, const float* gscale,
                                        float* part, int B, int C, int heads, int H, int W, hipStream_t stream) {
    if (!qkv || !taps || !gscale || !part || B <= 0 || C <= 0 || heads <= 0 || H <= 0 || W <= 0) return IRM_EINVAL;
    if (C % heads || C / heads != 48 || (H & 7) || (W & 31)) return IRM_EINVAL;
    const long tiles = (long)(H / QC_TH) * (W / QC_TW);
    if (tiles % QC_NCH || (long)3 * C * H * W >= (1L << 30) || bs < (long)2 * C * H * W) return IRM_EINVAL;
    if ((bs & 3) || !irm_aligned16(qkv) || !irm_aligned16(gscale) || (reinterpret_cast<uintptr_t>(part) & 3) ||
        (reinterpret_cast<uintptr_t>(taps) & 3) || (reinterpret_cast<uintptr_t>(bias) & 3)) return IRM_EINVAL;
    const long units = (long)B * heads * (tiles / QC_NCH);
    if (units >= (1L << 28)) return IRM_EINVAL;
    IRM_ALLOW_BIG_LDS((&dw_gram_kernel));
    int n = 0;
    if (irm_cu_count(n) != IRM_OK) return IRM_ELAUNCH;
    DgArgs a;
    a.qkv = qkv; a.bs = bs; a.taps = taps; a.bias = bias; a.gscale = gscale; a.part = part;
    a.C = C; a.heads = heads; a.H = H; a.W = W;
    a.tiles_x = W / QC_TW; a.cpi = (int)(tiles / QC_NCH); a.units = (int)units;
    const int per = (a.units + 7) >> 3;
    a.gpx = (n + 7) / 8;
    if (a.gpx > per) a.gpx = per;
    hipLaunchKernelGGL(dw_gram_kernel, dim3(a.gpx * 8), dim3(512), DG_LDS, stream, a);
    return irm_launch_status();
}
