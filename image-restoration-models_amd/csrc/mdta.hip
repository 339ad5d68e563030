// MDTA core (src/restormer/restormer.py:115-129): transposed (channel)
// attention.  The reference L2-normalises q and k along HW, forms the c x c
// logits per head, softmaxes the rows and multiplies by v, then applies the
// 1x1 project_out.  Here:
//
//   pass 1 (irm_mdta_gram_f32)    raw Gram G = q k^T and the squared row norms
//                                 of q and k, accumulated over HW in one sweep
//                                 of q,k on the exact-f32 MFMA; per-chunk
//                                 partials go to a workspace (no atomics).
//   pass 2 (irm_mdta_finalize_f32) fixed-order reduction of the partials,
//                                 A = softmax_j(G_ij/(max(|q_i|,eps) max(|k_j|,eps)) * temperature),
//                                 folded with project_out into ONE C x C matrix
//                                 per image, Mfold = W_out * blockdiag(A_heads),
//                                 written in the packed layout of gemm_pw.hip.
//   pass 3 = irm_gemm1x1_f32(Mfold, v, residual x): attn@v, project_out and the
//            residual add in one GEMM.
//
// Gram kernel mapping: one WAVE = one (batch, head, 16*SB x 16*SB sub-block of
// G, chunk of HW).  HW is the MFMA reduction axis; any bijection between HW
// positions and (k-step, k-slot) is legal as long as q and k use the same one,
// so each lane loads 16-byte pieces straight from global memory: lane (r, g)
// of load j reads row r, positions slab + 16 j + 4 g .. +3, and the 4 elements
// feed 4 successive MFMAs.  No LDS, no barriers; the next 32 positions are prefetched into a
// second register set while the current ones are multiplied.
#include "irm_common.h"

struct GramArgs {
    const float* qkv; long bs;     // [B][3C][N]; q rows [0,C), k rows [C,2C)
    float* part;                   // [B][heads][nchunk][c*c + 2c]
    int C, heads, N, chunk, nchunk;
    int tm;                        // f16x3 ring kernel: q, k tile-major [B][N / 256][2C][256] inside the q, k part of the buffer
};

template <int SB, bool VEC>
__global__ __launch_bounds__(256) void mdta_gram_kernel(GramArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int c = a.C / a.heads;
    const int nsb = c / (16 * SB);                 // sub-blocks per side
    const int nsub = nsb * nsb;
    // unit id: sub-block fastest so that waves sharing q/k rows sit in one workgroup
    const long unit = (long)blockIdx.x * 4 + wave;
    const long units_per_bh = (long)nsub * a.nchunk;
    const int b = blockIdx.y;
    if (unit >= a.heads * units_per_bh) return;
    const int head = (int)(unit / units_per_bh);
    const long rem = unit % units_per_bh;
    const int chunk_id = (int)(rem / nsub);
    const int sub = (int)(rem % nsub);
    const int si = sub / nsb, sj = sub % nsb;

    const int r = lane & 15, g = lane >> 4;
    const float* q = a.qkv + (long)b * a.bs + (long)(head * c + si * 16 * SB + r) * a.N;
    const float* k = a.qkv + (long)b * a.bs + (long)(a.C + head * c + sj * 16 * SB + r) * a.N;

    f32x4 acc[SB][SB];
    float nq[SB], nk[SB];
#pragma unroll
    for (int i = 0; i < SB; ++i) {
        nq[i] = 0.f; nk[i] = 0.f;
#pragma unroll
        for (int j = 0; j < SB; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

    const int nbeg = chunk_id * a.chunk;
    const int nend = min(nbeg + a.chunk, a.N);
    // 32 positions per step (2 x 16 bytes per lane and tile), operands of step i+1 are fetched while
    // the MFMAs of step i run (two register sets, static indexing through the 2x unrolled body)
    float4 qa[2][SB][2], ka[2][SB][2];
    auto fetch = [&](int set, int slab) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = slab + 16 * j + 4 * g;
            const bool ok = n < nend;
#pragma unroll
            for (int i = 0; i < SB; ++i) {
                qa[set][i][j] = ok ? irm_ld4<VEC>(q + (long)i * 16 * a.N, n, nend) : make_float4(0.f, 0.f, 0.f, 0.f);
                ka[set][i][j] = ok ? irm_ld4<VEC>(k + (long)i * 16 * a.N, n, nend) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    };
    auto consume = [&](int set) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < SB; ++i) {
                const float4 x = qa[set][i][j], y = ka[set][i][j];
                nq[i] += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
                nk[i] += y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w;
            }
#pragma unroll
            for (int ii = 0; ii < SB; ++ii)
#pragma unroll
                for (int jj = 0; jj < SB; ++jj) {
                    acc[ii][jj] = irm_mfma16(qa[set][ii][j].x, ka[set][jj][j].x, acc[ii][jj]);
                    acc[ii][jj] = irm_mfma16(qa[set][ii][j].y, ka[set][jj][j].y, acc[ii][jj]);
                    acc[ii][jj] = irm_mfma16(qa[set][ii][j].z, ka[set][jj][j].z, acc[ii][jj]);
                    acc[ii][jj] = irm_mfma16(qa[set][ii][j].w, ka[set][jj][j].w, acc[ii][jj]);
                }
        }
    };
    fetch(0, nbeg);
    for (int slab = nbeg; slab < nend; slab += 64) {
        fetch(1, slab + 32);           // positions >= nend read as zero
        consume(0);
        fetch(0, slab + 64);
        consume(1);
    }

    // partial record of this (b, head, chunk): G[c][c], nq[c], nk[c]
    const long rec = (long)c * c + 2 * c;
    float* out = a.part + (((long)b * a.heads + head) * a.nchunk + chunk_id) * rec;
#pragma unroll
    for (int ii = 0; ii < SB; ++ii)
#pragma unroll
        for (int jj = 0; jj < SB; ++jj) {
            const int col = sj * 16 * SB + jj * 16 + r;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = si * 16 * SB + ii * 16 + g * 4 + e;
                out[(long)row * c + col] = acc[ii][jj][e];
            }
        }
    // squared norms: sum the 4 lane groups (lanes r, r+16, r+32, r+48)
#pragma unroll
    for (int i = 0; i < SB; ++i) {
        float vq = nq[i], vk = nk[i];
        vq += __shfl_xor(vq, 16); vq += __shfl_xor(vq, 32);
        vk += __shfl_xor(vk, 16); vk += __shfl_xor(vk, 32);
        if (g == 0) {
            if (sj == 0) out[(long)c * c + si * 16 * SB + i * 16 + r] = vq;
            if (si == 0) out[(long)c * c + c + sj * 16 * SB + i * 16 + r] = vk;
        }
    }
}

// ---------------------------------------------------------------------------
// Fast path (c = 48 or 96, N % 64 == 0, 16-byte aligned): one workgroup = one (batch, head, chunk of HW) and
// the whole c x c Gram.  Stages of BP pixels x 2c rows (24 KiB: q rows then k rows of the head) stream through
// a 3-deep LDS-DMA ring in full 128/256-byte row segments.  Each 1 KiB DMA instruction covers RPB rows; the
// 16-byte pieces of a row are ROTATED by the row number on the way in (the per-lane source address is
// free), so that the MFMA operand reads - 16 different rows at the same pixel quad - hit 16 different bank
// quads: conflict-free ds_read_b32 with one address register per k-step and immediate offsets per tile.
//   T = 3 (c = 48): BP = 64, the 4 waves split the 16 k-steps of a stage, partial Grams are summed through
//                   LDS in wave order at the end (deterministic);
//   T = 6 (c = 96): BP = 32, wave (wa, wb) owns the 48 x 48 quadrant (wa, wb) for all 8 k-steps.
// GramStage holds what this kernel and mdta_gram_f16x3_kernel below share as ONE definition: the stage geometry and the
// DMA issue of a stage.  (The guarded mdta_gram_kernel above has no ring; gram_cm.h's qc_gram_flush combines 8 waves of 512
// threads that hold other tiles: both stay on their own.)
template <int T, int NS>
struct GramStage {
    static constexpr int c = 16 * T;
    static constexpr int BP = T == 3 ? 64 : 32;    // pixels per stage
    static constexpr int CPR = BP / 4;             // 16-byte pieces per row segment
    static constexpr int RPB = 64 / CPR;           // rows per 1 KiB DMA instruction
    static constexpr int NI = 2 * c / RPB;         // DMA instructions per stage (24)
    static constexpr int LPS = NI / 4;             // per wave (6)
    static constexpr int STG = NI * 256;           // floats per stage
    static constexpr int REC = c * c + 2 * c;      // floats per partial record: G[c][c], nq[c], nk[c]
    static_assert((NS - 2) * LPS <= 63, "vmcnt field");

    // stage s of the workgroup whose first block starts at pixel nbeg and whose blocks lie sstep pixels apart, into ring
    // slot s % NS: this wave's LPS instructions from its lanes' sources src (stage 0) + the stage's offset
    static __device__ __forceinline__ void issue(const GramArgs& a, const float* const (&src)[LPS], int wave, int nbeg,
                                                 long sstep, int s) {
        extern __shared__ __attribute__((aligned(16))) float smem[];
        float* dst = smem + (s % NS) * STG + wave * 256;
        long so = s * sstep;
        if (a.tm) {
            const long n0 = (long)nbeg + so;                 // first pixel (tile order) of this stage's block
            so = (n0 >> 8) * (2L * a.C * 256) + (n0 & 255);
        }
#pragma unroll
        for (int j = 0; j < LPS; ++j) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[j] + so),
                                             (__attribute__((address_space(3))) void*)(dst + j * 1024), 16, 0, 0);
        }
    }
};

template <int T, int NS>
__global__ __launch_bounds__(256, 2) void mdta_gram_ring_kernel(GramArgs a) {
    using Stage = GramStage<T, NS>;
    constexpr int c = Stage::c, BP = Stage::BP, CPR = Stage::CPR, RPB = Stage::RPB, LPS = Stage::LPS, STG = Stage::STG;
    constexpr int KS = BP / 4;                     // k-steps per stage
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, kk = lane >> 4;
    const int b = blockIdx.y;
    const int head = blockIdx.x / a.nchunk, chunk_id = blockIdx.x % a.nchunk;
    // interleaved pixel blocks: workgroup j takes the BP-pixel blocks j, j + nchunk, ... (why: at the emulated kernel)
    const int nbeg = chunk_id * BP;
    const int nblocks = a.N / BP;
    const int S = chunk_id < nblocks ? (nblocks - chunk_id + a.nchunk - 1) / a.nchunk : 0;
    const long sstep = (long)a.nchunk * BP;
    // (a.tm: q, k tile-major, described there too)
    const float* base = a.qkv + (long)b * a.bs + (a.tm ? 0 : nbeg);
    const long rowstride = a.tm ? 256 : a.N;

    // DMA sources of this lane: instruction j of this wave covers rows RPB*(4j + wave) ..; lane = rr*CPR + p
    // fetches piece (p - rot(row)) mod CPR of its row, rot(row) = row mod 16 (T = 3) or (row >> 1) mod 8
    const float* src[LPS];
#pragma unroll
    for (int j = 0; j < LPS; ++j) {
        const int row = RPB * (4 * j + wave) + lane / CPR, p = lane % CPR;
        const int rot = (T == 3 ? row : row >> 1) & (CPR - 1);
        const int ch = row < c ? head * c + row : a.C + head * c + (row - c);
        src[j] = base + (long)ch * rowstride + 4 * ((p - rot) & (CPR - 1));
    }
    auto issue = [&](int s) { Stage::issue(a, src, wave, nbeg, sstep, s); };

    // operand reads: row 16m + i (+ c for k), pixel quad ks, element kk
    //   T = 3: float offset 1024 m + (i>>2)*256 + (i&3)*64 + 4*((ks + i) & 15) + kk        (k rows: + 3072)
    //   T = 6: float offset  512 m + (i>>3)*256 + (i&7)*32 + 4*((ks + (i>>1)) & 7) + kk    (k rows: + 3072)
    const int rot = T == 3 ? i : i >> 1;
    const int lbase = (T == 3 ? (i >> 2) * 256 + (i & 3) * 64 : (i >> 3) * 256 + (i & 7) * 32) + kk;
    constexpr int MT = T == 3 ? 1024 : 512;        // float stride between 16-row tiles
    const int wa = wave >> 1, wb = wave & 1;
    const int qt0 = T == 3 ? 0 : 3 * wa, kt0 = T == 3 ? 0 : 3 * wb;     // first q / k tile of this wave
    const bool do_q = T == 3 || wa != wb, do_k = T == 3 || wa == wb;    // who accumulates which squared norms

    f32x4 acc[3][3];
    float nq[3] = {0.f, 0.f, 0.f}, nk[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
        for (int y = 0; y < 3; ++y) acc[x][y] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int j = 0; j < NS - 1; ++j)
        if (j < S) issue(j);

    for (int s = 0; s < S; ++s) {
        const int rem = min(NS - 2, S - 1 - s);
        if (rem >= NS - 2 && NS >= 3) irm_wait_vmcnt<(NS - 2) * LPS>();
        else irm_wait_vmcnt<0>();
        asm volatile("s_barrier" ::: "memory");
        if (s + NS - 1 < S) issue(s + NS - 1);
        const float* xb = smem + (s % NS) * STG + lbase;
#pragma unroll
        for (int t = 0; t < (T == 3 ? KS / 4 : KS); ++t) {
            const int ks = T == 3 ? 4 * wave + t : t;                   // T = 3: waves split the k-steps
            const float* pq = xb + 4 * ((ks + rot) & (CPR - 1));
            float qf[3], kf[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                qf[m] = pq[(qt0 + m) * MT];
                kf[m] = pq[3072 + (kt0 + m) * MT];
            }
            if (do_q) {
#pragma unroll
                for (int m = 0; m < 3; ++m) nq[m] = fmaf(qf[m], qf[m], nq[m]);
            }
            if (do_k) {
#pragma unroll
                for (int m = 0; m < 3; ++m) nk[m] = fmaf(kf[m], kf[m], nk[m]);
            }
#pragma unroll
            for (int x = 0; x < 3; ++x)
#pragma unroll
                for (int y = 0; y < 3; ++y) acc[x][y] = irm_mfma16(qf[x], kf[y], acc[x][y]);
        }
    }

    // squared norms: sum the 4 pixel slots (lanes i, i+16, i+32, i+48)
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        nq[m] += __shfl_xor(nq[m], 16); nq[m] += __shfl_xor(nq[m], 32);
        nk[m] += __shfl_xor(nk[m], 16); nk[m] += __shfl_xor(nk[m], 32);
    }
    constexpr int REC = Stage::REC;
    float* out = a.part + (((long)b * a.heads + head) * a.nchunk + chunk_id) * REC;
    if (T == 6) {
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    out[(long)((qt0 + x) * 16 + kk * 4 + e) * c + (kt0 + y) * 16 + i] = acc[x][y][e];
        if (kk == 0) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                if (do_q) out[c * c + (qt0 + m) * 16 + i] = nq[m];
                if (do_k) out[c * c + c + (kt0 + m) * 16 + i] = nk[m];
            }
        }
    } else {
        // the 4 waves hold partial sums over different k-steps: combine through LDS in wave order
        asm volatile("s_barrier" ::: "memory");      // every wave is done reading the ring
        float* mine = smem + wave * REC;
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int y = 0; y < 3; ++y)
#pragma unroll
                for (int e = 0; e < 4; ++e) mine[(x * 16 + kk * 4 + e) * c + y * 16 + i] = acc[x][y][e];
        if (kk == 0) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                mine[c * c + m * 16 + i] = nq[m];
                mine[c * c + c + m * 16 + i] = nk[m];
            }
        }
        __syncthreads();
        for (int e = tid; e < REC; e += 256)
            out[e] = ((smem[e] + smem[REC + e]) + smem[2 * REC + e]) + smem[3 * REC + e];
    }
}

// ---------------------------------------------------------------------------
// The same Gram pass as an fp32 emulation on the fp16 matrix cores (irm_mdta_gram_f16x3_f32): the f32-input MFMA
// above needs 2304 matrix cycles per wave and 24 KiB stage - 6.4 TB/s at best with two workgroups per CU -, the
// emulation 432 (27 v_mfma_f32_16x16x32_f16) plus ~400 cycles of vector work for the hi/lo split, so the sweep over
// q, k becomes a memory stream.  The LDS-DMA ring of mdta_gram_ring_kernel (GramStage) with the piece rotation gr_rot below; an operand fragment
// (row, 8 consecutive pixels) is two conflict-free ds_read_b128, scaled by the row's power-of-two factor
// (`scale`, host side: 2^14-ish / a static bound of |q_c|, |k_c| - exact), split into fp16 hi + lo, and multiplied
// as lo*hi + hi*lo + hi*hi with fp32 accumulation.  The squared norms stay on the fp32 vector pipe.  Records leave
// the kernel unscaled (power-of-two factors: exact), so the reduction and the softmax are unchanged.
//   T = 6 (c = 96): BP = 32, wave (wa, wb) owns the 48 x 48 quadrant (wa, wb), one 32-pixel k-step per stage.
//   T = 3 (c = 48): BP = 64, wave w takes the 32-pixel half w & 1 of the stage and q tiles {0, 1} (w < 2) or {2}.

// Piece rotation of the f16x3 Gram pass.  A ds_read_b128 is served in four groups of 16 lanes that are NOT contiguous
// (MI355X_MICROARCH.md, LDS: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32): with lane = 16 g + i a group
// holds rows A = {0-3, 12-15} at pixel group g and rows B = {4-11} at pixel group g + 1 (or the other way round), two
// 16-byte pieces further on.  Conflict free <=> the pieces of A and the pieces of B + 2 are all different <=> the
// rotations of A are the even values and those of B the odd ones (round 2 rotated by the plain row number, built for
// contiguous lane groups: every group had four to eight 2-way conflicts, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.5).
//   T = 3 (256-byte rows, 16 pieces): rot(i) = 2 rank_A(i) for i in A, 2 (i - 4) + 1 for i in B;
//   T = 6 (128-byte rows, two rows per bank row, 8 pieces): the same on h = i >> 1 within each row parity.
template <int T>
__device__ __forceinline__ int gr_rot(int row) {
    if (T == 3) return (int)((0xECA8FDB975316420ull >> (4 * (row & 15))) & 15);     // [0,2,4,6, 1,3,5,7,9,11,13,15, 8,10,12,14]
    return (int)((0x64753120u >> (4 * ((row >> 1) & 7))) & 7);                       // h: [0,2, 1,3,5,7, 4,6]
}

template <int T, int NS>
__global__ __launch_bounds__(256, 2) void mdta_gram_f16x3_kernel(GramArgs a, const float* __restrict__ scale) {
    using Stage = GramStage<T, NS>;
    constexpr int c = Stage::c, BP = Stage::BP, CPR = Stage::CPR, RPB = Stage::RPB, LPS = Stage::LPS, STG = Stage::STG;
    extern __shared__ __attribute__((aligned(16))) float smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int b = blockIdx.y;
    const int head = blockIdx.x / a.nchunk, chunk_id = blockIdx.x % a.nchunk;
    // INTERLEAVED pixel blocks: workgroup j of an (image, head) takes the BP-pixel blocks j, j + nchunk, j + 2 nchunk, ...
    // The nchunk workgroups run side by side and advance together: at any moment they read ONE contiguous run of
    // nchunk x BP pixels of every channel row (10 KiB instead of nchunk runs of 128 bytes, 12 KiB apart) - DRAM pages
    // are used whole.  The partial records cover other pixel sets than with contiguous chunks; their fixed-order sum
    // is the same Gram matrix.
    const int nbeg = chunk_id * BP;
    const int nblocks = a.N / BP;
    const int S = chunk_id < nblocks ? (nblocks - chunk_id + a.nchunk - 1) / a.nchunk : 0;
    const long sstep = (long)a.nchunk * BP;
    // Tile-major q, k (a.tm; written by irm_qkv_dw_fused_tm_f16x3_f32): the 256 pixels of an 8 x 32 tile are contiguous per
    // channel and the 2C channel rows of a tile follow one another - a stage reads 2c row segments 1 KiB apart inside ONE
    // contiguous 2C KiB block instead of 2c segments a whole plane apart.  Pixel blocks are numbered in tile order; which
    // pixels a block holds does not matter to the Gram sum as long as q and k agree.
    const float* base = a.qkv + (long)b * a.bs + (a.tm ? 0 : nbeg);
    const long rowstride = a.tm ? 256 : a.N;

    const float* src[LPS];
#pragma unroll
    for (int j = 0; j < LPS; ++j) {
        const int row = RPB * (4 * j + wave) + lane / CPR, p = lane % CPR;
        const int rot = gr_rot<T>(row);
        const int ch = row < c ? head * c + row : a.C + head * c + (row - c);
        src[j] = base + (long)ch * rowstride + 4 * ((p - rot) & (CPR - 1));
    }
    auto issue = [&](int s) { Stage::issue(a, src, wave, nbeg, sstep, s); };

    // this wave's tiles
    const int wa = wave >> 1, wb = wave & 1;
    constexpr int NQ = T == 3 ? 2 : 3;                                  // q tiles held (T = 3, w >= 2: only the first is used)
    const int qt0 = T == 3 ? 2 * wa : 3 * wa, kt0 = T == 3 ? 0 : 3 * wb;
    const int nq_used = T == 3 ? (wa ? 1 : 2) : 3;
    const bool do_q = T == 3 || wa != wb, do_k = T == 3 ? wa == 1 : wa == wb;   // who accumulates which squared norms
    // fragment addresses: row R, pixels 8 g .. 8 g + 7 of this wave's 32-pixel k-step = source pieces ph + 2 g, + 1
    const int rot = gr_rot<T>(i);
    const int ph = T == 3 ? 8 * wb : 0;
    const int o0 = 4 * ((ph + 2 * g + rot) & (CPR - 1)), o1 = 4 * ((ph + 2 * g + 1 + rot) & (CPR - 1));
    float sq[NQ], sk[3];
#pragma unroll
    for (int m = 0; m < NQ; ++m) sq[m] = scale[head * c + min(16 * (qt0 + m), c - 16) + i];
#pragma unroll
    for (int m = 0; m < 3; ++m) sk[m] = scale[a.C + head * c + 16 * (kt0 + m) + i];

    f32x4 acc[NQ][3];
    float nq[NQ], nk[3];
#pragma unroll
    for (int x = 0; x < NQ; ++x) {
        nq[x] = 0.f;
#pragma unroll
        for (int y = 0; y < 3; ++y) acc[x][y] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int y = 0; y < 3; ++y) nk[y] = 0.f;

    auto fragment = [&](const float* rowp, float sc, bool norm, float& nacc, irm_h8& hi, irm_h8& lo) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(rowp + o0);
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(rowp + o1);
        float xs[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x = e < 4 ? v0[e] : v1[e - 4];
            if (norm) nacc = fmaf(x, x, nacc);
            xs[e] = x * sc;                                // power-of-two factor: exact
        }
        irm_split8(xs, hi, lo);
    };

#pragma unroll
    for (int j = 0; j < NS - 1; ++j)
        if (j < S) issue(j);

    for (int s = 0; s < S; ++s) {
        const int rem = min(NS - 2, S - 1 - s);
        if (rem >= NS - 2 && NS >= 3) irm_wait_vmcnt<(NS - 2) * LPS>();
        else irm_wait_vmcnt<0>();
        asm volatile("s_barrier" ::: "memory");
        if (s + NS - 1 < S) issue(s + NS - 1);
        const float* xb = smem + (s % NS) * STG + i * BP;
        irm_h8 qh[NQ], ql[NQ], kh[3], kl[3];
#pragma unroll
        for (int m = 0; m < NQ; ++m)
            if (m < nq_used) fragment(xb + (qt0 + m) * 16 * BP, sq[m], do_q, nq[m], qh[m], ql[m]);
#pragma unroll
        for (int m = 0; m < 3; ++m) fragment(xb + (c + (kt0 + m) * 16) * BP, sk[m], do_k, nk[m], kh[m], kl[m]);
#pragma unroll
        for (int x = 0; x < NQ; ++x) {
            if (x < nq_used) {
#pragma unroll
                for (int y = 0; y < 3; ++y) {
                    acc[x][y] = irm_mfma3_f16(qh[x], ql[x], kh[y], kl[y], acc[x][y]);
                }
            }
        }
    }

    // squared norms: sum the 4 pixel groups (lanes i, i+16, i+32, i+48)
#pragma unroll
    for (int m = 0; m < NQ; ++m) { nq[m] += __shfl_xor(nq[m], 16); nq[m] += __shfl_xor(nq[m], 32); }
#pragma unroll
    for (int m = 0; m < 3; ++m) { nk[m] += __shfl_xor(nk[m], 16); nk[m] += __shfl_xor(nk[m], 32); }
    constexpr int REC = Stage::REC;
    float* out = a.part + (((long)b * a.heads + head) * a.nchunk + chunk_id) * REC;
    // undo the operand scales (exact): element (q row, k row) by 1 / (s_q s_k)
    float isk[3];
#pragma unroll
    for (int y = 0; y < 3; ++y) isk[y] = 1.0f / sk[y];
    const float* sqp = scale + head * c;
    if (T == 6) {
#pragma unroll
        for (int x = 0; x < 3; ++x)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = (qt0 + x) * 16 + g * 4 + e;
                const float isq = 1.0f / sqp[row];
#pragma unroll
                for (int y = 0; y < 3; ++y) out[(long)row * c + (kt0 + y) * 16 + i] = acc[x][y][e] * (isq * isk[y]);
            }
        if (g == 0) {
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                if (do_q) out[c * c + (qt0 + m) * 16 + i] = nq[m];
                if (do_k) out[c * c + c + (kt0 + m) * 16 + i] = nk[m];
            }
        }
    } else {
        // waves 0/1 hold q tiles {0, 1} over the two pixel halves, waves 2/3 q tile 2 and the k norms:
        // combine through LDS in wave order
        asm volatile("s_barrier" ::: "memory");      // every wave is done reading the ring
        float* mine = smem + wave * REC;
#pragma unroll
        for (int x = 0; x < NQ; ++x) {
            if (x < nq_used) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = (qt0 + x) * 16 + g * 4 + e;
                    const float isq = 1.0f / sqp[row];
#pragma unroll
                    for (int y = 0; y < 3; ++y) mine[row * c + y * 16 + i] = acc[x][y][e] * (isq * isk[y]);
                }
                if (g == 0) mine[c * c + (qt0 + x) * 16 + i] = nq[x];
            }
        }
        if (g == 0 && do_k) {
#pragma unroll
            for (int m = 0; m < 3; ++m) mine[c * c + c + m * 16 + i] = nk[m];
        }
        __syncthreads();
        for (int e = tid; e < REC; e += 256) {
            const int row = e < c * c ? e / c : (e < c * c + c ? e - c * c : 32);     // k norms live with waves 2, 3
            const int w0 = row < 32 ? 0 : 2;
            out[e] = smem[w0 * REC + e] + smem[(w0 + 1) * REC + e];
        }
    }
}

template <int T>
static int launch_gram_f16x3(const GramArgs& a, const float* scale, int B, hipStream_t stream) {
    constexpr int NS = 3;
    const size_t lds = (size_t)NS * 24 * 1024;
    IRM_ALLOW_BIG_LDS((&mdta_gram_f16x3_kernel<T, NS>));
    hipLaunchKernelGGL((mdta_gram_f16x3_kernel<T, NS>), dim3(a.heads * a.nchunk, B), dim3(256), lds, stream, a, scale);
    return irm_launch_status();
}

template <int T>
static int launch_gram_ring(const GramArgs& a, int B, hipStream_t stream) {
    constexpr int NS = 3;
    const size_t lds = (size_t)NS * 24 * 1024;
    IRM_ALLOW_BIG_LDS((&mdta_gram_ring_kernel<T, NS>));
    hipLaunchKernelGGL((mdta_gram_ring_kernel<T, NS>), dim3(a.heads * a.nchunk, B), dim3(256), lds, stream, a);
    return irm_launch_status();
}

// The argument check of the four Gram entries: fills `a` or returns IRM_EINVAL.
//   pix     the multiple of pixels the entry needs of N: 64 or 256 for the ring-only entries, which also need 16-byte
//           aligned rows and a grid within 2^31; 0 for the entry whose guarded kernel takes what the ring cannot;
//   ring_c  c = C / heads must be 48 or 96 (else: a multiple of 16);
//   tm      q, k tile-major.
static int gram_check(GramArgs& a, const float* qkv, long bs, float* part, int B, int C, int heads, int N, int chunk,
                      int pix, bool ring_c, int tm) {
    if (!qkv || !part || B <= 0 || C <= 0 || heads <= 0 || N <= 0 || chunk <= 0) return IRM_EINVAL;
    if (C % heads || (chunk & 63) || B > 65535) return IRM_EINVAL;
    const int c = C / heads, nchunk = (N + chunk - 1) / chunk;
    if (ring_c ? (c != 48 && c != 96) : c % 16 != 0) return IRM_EINVAL;
    if (pix && ((N & (pix - 1)) || (bs & 3) || !irm_aligned16(qkv) || (long)heads * nchunk > 2147483647L)) return IRM_EINVAL;
    a = GramArgs{qkv, bs, part, C, heads, N, chunk, nchunk, tm};
    return IRM_OK;
}

static int gram_f16x3_entry(const float* qkv, long bs, const float* scale, float* part, int B, int C, int heads, int N,
                            int chunk, int pix, int tm, hipStream_t stream) {
    GramArgs a;
    if (!scale || gram_check(a, qkv, bs, part, B, C, heads, N, chunk, pix, true, tm) != IRM_OK) return IRM_EINVAL;
    return C / heads == 48 ? launch_gram_f16x3<3>(a, scale, B, stream) : launch_gram_f16x3<6>(a, scale, B, stream);
}

extern "C" int irm_mdta_gram_f16x3_f32(const float* qkv, long bs, const float* scale, float* part, int B, int C,
                                       int heads, int N, int chunk, hipStream_t stream) {
    return gram_f16x3_entry(qkv, bs, scale, part, B, C, heads, N, chunk, 64, 0, stream);
}

// The same pass over tile-major q, k (header): N % 256 == 0.
extern "C" int irm_mdta_gram_tm_f16x3_f32(const float* qkv, long bs, const float* scale, float* part, int B, int C,
                                          int heads, int N, int chunk, hipStream_t stream) {
    return gram_f16x3_entry(qkv, bs, scale, part, B, C, heads, N, chunk, 256, 1, stream);
}

// The f32-input ring pass over tile-major q, k (header): c = 48 / 96, N % 256 == 0.
extern "C" int irm_mdta_gram_tm_f32(const float* qkv, long bs, float* part, int B, int C, int heads, int N, int chunk,
                                    hipStream_t stream) {
    GramArgs a;
    if (gram_check(a, qkv, bs, part, B, C, heads, N, chunk, 256, true, 1) != IRM_OK) return IRM_EINVAL;
    return C / heads == 48 ? launch_gram_ring<3>(a, B, stream) : launch_gram_ring<6>(a, B, stream);
}

extern "C" int irm_mdta_gram_f32(const float* qkv, long bs, float* part, int B, int C, int heads, int N,
                                 int chunk, hipStream_t stream) {
    GramArgs a;
    if (gram_check(a, qkv, bs, part, B, C, heads, N, chunk, 0, false, 0) != IRM_OK) return IRM_EINVAL;
    const int c = C / heads;
    const bool vec = !(N & 3) && !(bs & 3) && irm_aligned16(qkv);
    if (vec && !(N & 63) && (c == 48 || c == 96) && (long)heads * a.nchunk <= 2147483647L)
        return c == 48 ? launch_gram_ring<3>(a, B, stream) : launch_gram_ring<6>(a, B, stream);
    const int sb = (c % 48 == 0) ? 3 : (c % 32 == 0) ? 2 : 1;
    const int nsb = c / (16 * sb);
    const long units = (long)heads * nsb * nsb * a.nchunk;
    dim3 grid((unsigned)((units + 3) / 4), B);
    if (vec) {
        if (sb == 3) hipLaunchKernelGGL((mdta_gram_kernel<3, true>), grid, dim3(256), 0, stream, a);
        else if (sb == 2) hipLaunchKernelGGL((mdta_gram_kernel<2, true>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((mdta_gram_kernel<1, true>), grid, dim3(256), 0, stream, a);
    } else {
        if (sb == 3) hipLaunchKernelGGL((mdta_gram_kernel<3, false>), grid, dim3(256), 0, stream, a);
        else if (sb == 2) hipLaunchKernelGGL((mdta_gram_kernel<2, false>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((mdta_gram_kernel<1, false>), grid, dim3(256), 0, stream, a);
    }
    return irm_launch_status();
}

// ---------------------------------------------------------------------------
// reduce: fixed-order sum of the per-chunk partial records.  A workgroup owns
// 64 consecutive record elements; its 4 waves each sum every 4th chunk and the
// four sums are combined in wave order through LDS, so the result does not
// depend on scheduling.
__global__ __launch_bounds__(256) void mdta_reduce_kernel(const float* __restrict__ part,
                                                          float* __restrict__ gsum, int rec, int nchunk) {
    __shared__ float sm[4][64];
    const int e = blockIdx.x * 64 + (threadIdx.x & 63);
    const int w = threadIdx.x >> 6;
    const long bh = blockIdx.y;
    float s = 0.0f;
    if (e < rec) {
        const float* p = part + bh * nchunk * (long)rec + e;
        int ch = w;
        for (; ch + 12 < nchunk; ch += 16) {             // four loads in flight, summed in chunk order
            const float v0 = p[(long)ch * rec], v1 = p[(long)(ch + 4) * rec], v2 = p[(long)(ch + 8) * rec],
                        v3 = p[(long)(ch + 12) * rec];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; ch < nchunk; ch += 4) s += p[(long)ch * rec];
    }
    sm[w][threadIdx.x & 63] = s;
    __syncthreads();
    if (w == 0 && e < rec) {
        const int l = threadIdx.x;
        gsum[bh * rec + e] = ((sm[0][l] + sm[1][l]) + sm[2][l]) + sm[3][l];
    }
}


// finalize: one workgroup per (batch, head).
//  1. one thread per row: logits, max, exp, sum -> A row in LDS;
//  2. Mfold[co][head*c + j] = sum_i Wout[co][head*c + i] * A[i][j], stored packed:
//     Wp[mtile][kstep][lane] = Mfold[16 mtile + (lane&15)][4 kstep + (lane>>4)].
struct FinArgs {
    const float* gsum;          // [B][heads][c*c + 2c]
    const float* temperature;   // [heads]
    const float* wout;          // [C][C] project_out weight (row-major, [co][ci])
    float* mfold;               // [B][mtiles][ksteps][64]
    float* attn;                // optional [B][heads][c][c] (tests) or null
    int C, heads, ksteps;
    int split;                  // layout of mfold, one of:
};
enum {
    FIN_PACKED = 0,             // packed fp32 (irm_gemm1x1_f32)
    FIN_SPLIT = 1,              // irm_gemm1x1_f16x3_f32's fp16 hi/lo order
    FIN_FRAG = 2,               // 16x16x32 MFMA fragments [mtile][KS][hi|lo][64 lanes][8 halves] (irm_attn_gdfn_fused_f16x3_f32)
};

// 16 waves: the softmax rows are chains of dependent cross-lane reductions (latency, not throughput), 6 rows per wave
// instead of 24
__global__ __launch_bounds__(1024) void mdta_finalize_kernel(FinArgs a) {
    constexpr int NT = 1024;
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int c = a.C / a.heads;
    const int head = blockIdx.x, b = blockIdx.y;
    const int rec = c * c + 2 * c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* G = sm;                 // [c][c], overwritten by A
    float* nrm = sm + c * c;       // [2c] squared norms of q rows, k rows
    const float* p = a.gsum + ((long)b * a.heads + head) * rec;
    if ((rec & 3) == 0 && rec <= 4 * NT * 3 && irm_aligned16(p)) {
        // all loads of a thread in flight at once (a plain copy loop is 37 dependent round trips at c = 96)
        const float4* p4 = reinterpret_cast<const float4*>(p);
        const int n4 = rec >> 2;
        float4 v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = threadIdx.x + NT * k;
            v[k] = e < n4 ? p4[e] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = threadIdx.x + NT * k;
            if (e < n4) reinterpret_cast<float4*>(sm)[e] = v[k];
        }
    } else {
        for (int e = threadIdx.x; e < rec; e += NT) sm[e] = p[e];
    }
    __syncthreads();
    // squared norms -> 1 / max(|q_i|, 1e-12), 1 / max(|k_j|, 1e-12) once (F.normalize's eps), instead of a square root
    // and a division per logit
    for (int e = threadIdx.x; e < 2 * c; e += NT) nrm[e] = 1.0f / fmaxf(sqrtf(nrm[e]), 1e-12f);
    __syncthreads();
    const float temp = a.temperature[head];
    // softmax: one wave per row, lanes over the columns
    for (int i = wave; i < c; i += NT / 64) {
        const float qi = nrm[i] * temp;
        float m = -INFINITY;
        for (int j = lane; j < c; j += 64) {
            const float l = G[i * c + j] * (qi * nrm[c + j]);
            G[i * c + j] = l;
            m = fmaxf(m, l);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        float ssum = 0.0f;
        for (int j = lane; j < c; j += 64) {
            const float e = expf(G[i * c + j] - m);
            G[i * c + j] = e;
            ssum += e;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ssum += __shfl_xor(ssum, o);
        const float inv = 1.0f / ssum;
        for (int j = lane; j < c; j += 64) G[i * c + j] *= inv;
    }
    __syncthreads();
    if (a.attn && blockIdx.z == 0) {
        float* o = a.attn + ((long)b * a.heads + head) * c * c;
        for (int e = threadIdx.x; e < c * c; e += NT) o[e] = G[e];
    }
    // fold with project_out; the output rows are split over gridDim.z workgroups
    const int mtiles = (a.C + 15) / 16;
    const int KS32 = (a.C + 31) / 32;
    float* mf = a.mfold + (a.split == FIN_FRAG ? (long)b * 2 * KS32 * KS32 * 512 : (long)b * mtiles * a.ksteps * 64);
    const int rows_per = (a.C + gridDim.z - 1) / gridDim.z;
    const int co0 = blockIdx.z * rows_per, co1 = min(co0 + rows_per, a.C);
    // this workgroup's rows of project_out (columns of this head) into LDS: the dot products below then read LDS only
    float* Wl = sm + c * c + 2 * c;                    // [rows_per][c]
    for (int e = threadIdx.x; e < (co1 - co0) * c; e += NT)
        Wl[e] = a.wout[(long)(co0 + e / c) * a.C + head * c + e % c];
    __syncthreads();
    for (int e = co0 * c + threadIdx.x; e < co1 * c; e += NT) {
        const int co = e / c, j = e % c;
        const float* wrow = Wl + (co - co0) * c;
        float acc = 0.0f;
#pragma unroll 8
        for (int i = 0; i < c; ++i) acc += wrow[i] * G[i * c + j];
        const int kcol = head * c + j;
        if (a.split == FIN_FRAG) {
            // fragment (mtile, 32-channel k-step): lane 16 g + m holds W[16 mtile + m][32 ks + 8 g + e], e = 0..7; hi then lo
            _Float16* frag = reinterpret_cast<_Float16*>(mf) + ((long)((co >> 4) * KS32 + (kcol >> 5)) * 2) * 512;
            const int slot = (((kcol & 31) >> 3) * 16 + (co & 15)) * 8 + (kcol & 7);
            const _Float16 hi = (_Float16)acc;
            frag[slot] = hi;
            frag[512 + slot] = (_Float16)(acc - (float)hi);
        } else if (a.split != FIN_PACKED) {
            // record of (mtile, 16-channel stage): 64 lanes x 4 hi halves, then 64 lanes x 4 lo halves;
            // lane (g, m) slot jj holds W[m][16 stage + 4 jj + g]
            _Float16* rec = reinterpret_cast<_Float16*>(mf + ((long)(co >> 4) * (a.ksteps >> 2) + (kcol >> 4)) * 256);
            const int slot = ((kcol & 3) * 16 + (co & 15)) * 4 + ((kcol & 15) >> 2);
            const _Float16 hi = (_Float16)acc;
            rec[slot] = hi;
            rec[256 + slot] = (_Float16)(acc - (float)hi);
        } else {
            const int ln = (co & 15) + 16 * (kcol & 3);
            mf[((long)(co >> 4) * a.ksteps + (kcol >> 2)) * 64 + ln] = acc;
        }
    }
}

static int mdta_finalize(const float* part, float* gsum, const float* temperature, const float* wout, float* mfold,
                         float* attn, int B, int C, int heads, int nchunk, int split, hipStream_t stream) {
    if (!part || !gsum || !temperature || !wout || !mfold || B <= 0 || C <= 0 || heads <= 0 || nchunk <= 0)
        return IRM_EINVAL;
    if (C % heads || (long)B * heads > 65535) return IRM_EINVAL;
    const int c = C / heads;
    const int rec = c * c + 2 * c;
    // output rows split over zsplit workgroups per (image, head), each repeating the (cheap) softmax: 8, or fewer when that is
    // more than two rounds of the chip (C = 384, 8 heads, 24 tiles: 1536 workgroups of 1024 threads took 56 us; 384 take 25).
    // The result does not depend on the split (every output element is the same dot product).
    auto lds_of = [&](int z) { return ((size_t)rec + (size_t)((C + z - 1) / z) * c) * sizeof(float); };
    int zsplit = 8;
    while (zsplit > 1 && (long)B * heads * zsplit > 512 && lds_of(zsplit / 2) <= 64 * 1024) zsplit >>= 1;
    const size_t lds = lds_of(zsplit);
    if (lds > 64 * 1024) return IRM_EINVAL;
    hipLaunchKernelGGL(mdta_reduce_kernel, dim3((rec + 63) / 64, B * heads), dim3(256), 0, stream, part, gsum,
                       rec, nchunk);
    int rc = irm_launch_status();
    if (rc != IRM_OK) return rc;
    // padded rows/cols of the packed matrix stay zero: the caller clears mfold once at allocation
    // (C is a multiple of 16 at every Restormer level, so normally there is no padding at all)
    FinArgs a{gsum, temperature, wout, mfold, attn, C, heads, 4 * ((C + 15) / 16), split};
    hipLaunchKernelGGL(mdta_finalize_kernel, dim3(heads, B, zsplit), dim3(1024), lds, stream, a);
    return irm_launch_status();
}

extern "C" int irm_mdta_finalize_f32(const float* part, float* gsum, const float* temperature,
                                     const float* wout, float* mfold, float* attn, int B, int C, int heads,
                                     int nchunk, hipStream_t stream) {
    return mdta_finalize(part, gsum, temperature, wout, mfold, attn, B, C, heads, nchunk, FIN_PACKED, stream);
}

extern "C" int irm_mdta_finalize_frag_f16x3_f32(const float* part, float* gsum, const float* temperature,
                                                const float* wout, float* mfold_frag, float* attn, int B, int C,
                                                int heads, int nchunk, hipStream_t stream) {
    if (C & 15) return IRM_EINVAL;
    return mdta_finalize(part, gsum, temperature, wout, mfold_frag, attn, B, C, heads, nchunk, FIN_FRAG, stream);
}

extern "C" int irm_mdta_finalize_f16x3_f32(const float* part, float* gsum, const float* temperature,
                                           const float* wout, float* mfold_split, float* attn, int B, int C,
                                           int heads, int nchunk, hipStream_t stream) {
    return mdta_finalize(part, gsum, temperature, wout, mfold_split, attn, B, C, heads, nchunk, FIN_SPLIT, stream);
}
