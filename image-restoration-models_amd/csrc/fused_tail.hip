// GDFN tail of the C = 192 level of Restormer in ONE kernel (round 3):
//
//   x += project_out( gelu(dw(h)[:hid]) * dw(h)[hid:] ) + bias2        (FeedForward.dwconv / chunk / gelu * / project_out and the
//                                                                       block's residual, restormer.py:84-93, 148)
//
// with h = project_in(LN(x)) written by irm_ln_gemm_presplit_cl_f16x3_f32 tile-major channel-last, its two halves padded to
// HP channels each, in chunks of 64 channels ([tile][2 HP / 64][256 pixels][64]: the producer's chunk of 64 channels is one
// contiguous run per pixel tile).  Before: a gated depth-wise kernel wrote g (hid planes) and a streaming GEMM
// read it back - 1.2 GB per 12-tile block at C = 192 - as two launches; here g never leaves the CU.
//
// This is the second half of the GDFN branch kernel of the C <= 96 levels (fused_block.hip) with the h image filled from
// HBM instead of by the project_in MFMAs: one persistent workgroup (8 waves) per CU walks (image, 8 x 32 tile) items; per
// stage of 16 gate pairs (32 channels of h) every lane fetches five or six 16-byte pieces (pixel, 4 channels) of the 10 x 34
// halo tile ONE STAGE AHEAD into registers (channel-last: whole lines, nothing wasted; halo pixels outside the image read a
// zero page - the reference zero-pads h) and parks them in the channel-minor LDS image [pixel][32 channels + pad] (160-byte
// pixel stride: the stencil's ds_read_b128 are conflict free) that fused_block.hip's stencil expects; the depth-wise 3x3,
// the erf-GELU gate, the fp16 hi/lo split of the gate (x 2^-4, saturating) and the fp32-emulated project_out (three
// v_mfma_f32_16x16x32_f16 per product, CT = C / 16 = 12 accumulator tiles x 2 rows per wave) are that kernel's.  The block's
// residual is read and written in place in the epilogue (a tile reads h with its halo, x only inside the tile).
#include "irm_common.h"

struct TailArgs {
    const float* Hh; long h_bs;           // [B][tiles][CB / 64][256][64]
    float* X; long x_bs;                  // [B][C][H][W], updated in place
    const float* rec;                     // [S][512]: depth-wise taps [10][32] of stage s (9 taps + bias; second half x 2^-4), pad
    const float* w2;                      // [ceil(S/2)][CT][hi|lo][64 lanes][8 halves], as irm_gdfn_fused_f16x3_f32
    const float* bias2;                   // [C] or null
    int C, H, W, S, HP, CB;
    float inv_s2;
    int tiles_x, tiles, items, gpx;
};

template <int CT>
__global__ __launch_bounds__(512, 2) void gdfn_tail_kernel(TailArgs a) {
    constexpr int RECF = 512;                      // floats per tap record
    constexpr int W2F = CT * 512, W2P = CT * 2;
    constexpr int SLOT_B = RECF * 4, W2_OFF = 2 * SLOT_B, PL_OFF = W2_OFF + W2F * 4, PL_B = IRM_PLF * 4;
    constexpr int PARK_OFF = PL_OFF + 2 * PL_B;
    constexpr int NK = (IRM_NP * 8 + 511) / 512;    // 16-byte pieces per lane and stage (6; the last one partly)
    static_assert(PARK_OFF + 8192 <= 160 * 1024, "LDS");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    irm_lc* lds = (irm_lc*)smem;
    float* slots = smem;
    float* w2a = smem + W2_OFF / 4;

    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const long plane = (long)a.H * a.W;
    const int S = a.S;
    const int per = (a.items + 7) >> 3;
    const int xcd = blockIdx.x & 7, pos = blockIdx.x >> 3;
    auto item_of = [&](int round) { const int i = round * a.gpx + pos; return i < per ? xcd * per + i : a.items; };

    int round = 0;
    int item = item_of(0);
    if (item >= a.items) return;

    for (;;) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63, g = lane >> 4, r = lane & 15;
        const int b = item / a.tiles, tile = item - b * a.tiles;
        const int ty0 = (tile / a.tiles_x) * IRM_TH, tx0 = (tile % a.tiles_x) * IRM_TW;
        const float* Hh = a.Hh + (long)b * a.h_bs;
        const unsigned vw = irm_opaque((unsigned)(lane * 16));
        const unsigned vc = irm_opaque((unsigned)(16 * g));
        const int sp0 = (2 * (wave >> 1)) * IRM_HC + 16 * (wave & 1) + r;
        const unsigned vp0 = irm_opaque((unsigned)(PL_OFF + (sp0 * IRM_PS + 4 * g) * 4));
        const unsigned vp1 = irm_opaque(vp0 + PL_B);

        // this lane's pieces of a stage: piece idx = k 512 + tid -> (halo pixel idx >> 3, 16-byte piece idx & 7: channels
        // 4 (piece & 3) .. + 3 of half piece >> 2).  goff: float offset of the piece in h for stage 0, or -1 (pixel outside the
        // image / beyond the tile: the zero page); loff: byte offset in LDS image 0
        int goff[NK];
        unsigned loff[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int idx = k * 512 + tid, px = idx >> 3, pc = idx & 7;
            const int hr = px / IRM_HC, hc = px - hr * IRM_HC;
            const int gy = ty0 - 1 + hr, gx = tx0 - 1 + hc;
            const bool valid = px < IRM_NP, inside = valid && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
            // h: [tile][CB / 64 chunks][256 pixels][64 channels]; the multiplier half starts HP / 64 chunks further on
            goff[k] = inside ? ((gy >> 3) * a.tiles_x + (gx >> 5)) * 256 * a.CB + ((gy & 7) * IRM_TW + (gx & 31)) * 64 + (pc & 3) * 4 +
                               (pc >> 2) * (a.HP / 64) * (256 * 64)
                             : -1;
            loff[k] = (unsigned)(PL_OFF + ((valid ? px : IRM_NP + (tid & 15)) * IRM_PS) * 4 + (pc & 3) * 16 + (pc >> 2) * 64);
        }
        f32x4 hreg[NK];
        const float* const zero_page = irm_zero_page;      // (named here, not inside the lambda: irm_common.h)
        auto load_h = [&](int s) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const float* src = goff[k] >= 0 ? Hh + goff[k] + (s >> 2) * (256 * 64) + (s & 3) * 16 : zero_page;
                hreg[k] = *reinterpret_cast<const f32x4*>(src);
            }
        };
        auto park_h = [&](int img) {
#pragma unroll
            for (int k = 0; k < NK; ++k) irm_st<f32x4>(lds, loff[k], img * PL_B, hreg[k]);
        };

        const int nitem = item_of(round + 1);

        // the previous item's last barrier has passed: every LDS region is free
        irm_dma<2>(a.rec, slots, wave, lane);                                // taps of stage 0 -> slot 0
        irm_dma<W2P>(a.w2, w2a, wave, lane);
        load_h(0);
        f32x4 acc2[2][CT];
        const unsigned vpark = irm_opaque((unsigned)(PARK_OFF + threadIdx.x * 16));
#pragma unroll
        for (int c = 0; c < CT; ++c) { acc2[0][c] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc2[1][c] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
        irm_st<f32x4>(lds, vpark, 0, acc2[1][CT - 1]);
        park_h(0);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();

        float o[2][2][4];
        f32x4 kprev[3];

        irm_u4 Gh[2], Gl[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) { Gh[q] = (irm_u4){0u, 0u, 0u, 0u}; Gl[q] = (irm_u4){0u, 0u, 0u, 0u}; }

        // iteration it: stencil + gate of stage it (image it & 1, taps in slot it & 1); the pieces of stage it + 1 are requested
        // at its start and parked in the other image at its end; project_out every second stage
        auto iter = [&](auto PAR, auto MORE, int it) {
            constexpr int par = decltype(PAR)::value;
            constexpr bool more = decltype(MORE)::value;
            if constexpr (more) {
                load_h(it + 1);
                irm_dma<2>(a.rec + (long)(it + 1) * RECF, slots + (par ^ 1) * RECF, wave, lane);
            }
            if (par == 0 && it > 0) irm_dma<W2P>(a.w2 + (long)(it >> 1) * W2F, w2a, wave, lane);
            {
                const unsigned vp = par ? vp1 : vp0;
                f32x4 P[2][3], K[2][3], KB[1];
                auto loads = [&](auto IC, auto NC) {
                    constexpr int I = decltype(IC)::value, n = decltype(NC)::value;
                    constexpr int hf = I >> 2, dy = I & 3;
                    constexpr int cf = par * SLOT_B + hf * 64;
                    if constexpr (dy == 0) irm_dsr<cf + 9 * 128>(KB[0], vc);
                    if constexpr (dy < 3) {
                        irm_dsr<cf + (dy * 3 + 0) * 128>(K[n][0], vc);
                        irm_dsr<cf + (dy * 3 + 1) * 128>(K[n][1], vc);
                        irm_dsr<cf + (dy * 3 + 2) * 128>(K[n][2], vc);
                    }
                    irm_dsr<(dy * IRM_HC + 0) * (IRM_PS * 4) + hf * 64>(P[n][0], vp);
                    irm_dsr<(dy * IRM_HC + 1) * (IRM_PS * 4) + hf * 64>(P[n][1], vp);
                    irm_dsr<(dy * IRM_HC + 2) * (IRM_PS * 4) + hf * 64>(P[n][2], vp);
                };
                loads(irm_ic<0>{}, irm_ic<0>{});
                irm_for<8>([&](auto IC) {
                    constexpr int I = decltype(IC)::value, c = I & 1, n = c ^ 1;
                    constexpr int hf = I >> 2, dy = I & 3;
                    if constexpr (I + 1 < 8) loads(irm_ic<I + 1>{}, irm_ic<n>{});
                    constexpr int J = I + 1, jdy = J & 3;
                    constexpr int nnext = J < 8 ? 3 + (jdy < 3 ? 3 : 0) + (jdy == 0 ? 1 : 0) : 0;
                    irm_wait_lgkmcnt<nnext>();
                    irm_tie(P[c][0], P[c][1], P[c][2]);
                    if constexpr (dy < 3) irm_tie(K[c][0], K[c][1], K[c][2]);
                    if constexpr (dy == 0) irm_tie(KB[0]);
                    irm_stencil_step(dy, o[hf], kprev, P[c], K[c], KB[0]);
                    __builtin_amdgcn_sched_barrier(0);
                });
            }
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int e = 0; e < 4; e += 2) {
                    // (taps and bias of the second half are pre-scaled by 2^-4 on the host: o[1] = dw(h2) / 16, exact)
                    unsigned hh, ll;
                    irm_gate_split2(o[0][q][e], o[0][q][e + 1], o[1][q][e], o[1][q][e + 1], hh, ll);
                    Gh[q][2 * par + e / 2] = hh;
                    Gl[q][2 * par + e / 2] = ll;
                }
#pragma unroll
            for (int q = 0; q < 2; ++q) asm volatile("" : "+v"(Gh[q]), "+v"(Gl[q]));
            if (par == 1 || !more) {
                if constexpr (par == 0) {
                    // odd stage count: this super-stage's project_out weights were requested in this very iteration
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                }
                f32x4 accp = irm_ld<f32x4>(lds, vpark, 0);
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const irm_h8 bh = irm_ld<irm_h8>(lds, vw, W2_OFF + (c * 2) * 1024);
                    const irm_h8 bl = irm_ld<irm_h8>(lds, vw, W2_OFF + (c * 2 + 1) * 1024);
#pragma unroll
                    for (int q = 0; q < 2; ++q) {
                        f32x4& t = (q == 1 && c == CT - 1) ? accp : acc2[q][c];
                        t = irm_mfma3_f16(__builtin_bit_cast(irm_h8, Gh[q]), __builtin_bit_cast(irm_h8, Gl[q]), bh, bl, t);
                    }
                }
                irm_st<f32x4>(lds, vpark, 0, accp);
#pragma unroll
                for (int q = 0; q < 2; ++q) { Gh[q] = (irm_u4){0u, 0u, 0u, 0u}; Gl[q] = (irm_u4){0u, 0u, 0u, 0u}; }
            }
            if constexpr (more) park_h(par ^ 1);            // (the other image: its stencil finished before the last barrier)
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        };
        {
            const std::integral_constant<int, 0> P0; const std::integral_constant<int, 1> P1;
            const std::true_type T; const std::false_type F;
            int it = 0;
            for (; it + 2 < S; it += 2) { iter(P0, T, it); iter(P1, T, it + 1); }
            if (it + 2 == S) { iter(P0, T, it); iter(P1, F, it + 1); }
            else iter(P0, F, it);
        }

        // ------------------------------------------------------------ epilogue: x += acc / s2 + bias2, 16-byte accesses, in place
        {
            int t3 = threadIdx.x;
            asm volatile("" : "+v"(t3));
            const int r3 = t3 & 15, ox = tx0 + 16 * (wave & 1) + 4 * ((t3 & 63) >> 4), oy0 = ty0 + 2 * (wave >> 1);
            float* X = a.X + (long)b * a.x_bs;
            acc2[1][CT - 1] = irm_ld<f32x4>(lds, vpark, 0);
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const int co = 16 * c + r3;
                if (co >= a.C || ox >= a.W) continue;
                const float bv = a.bias2 ? a.bias2[co] : 0.0f;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    if (oy0 + q >= a.H) continue;
                    float4* px = reinterpret_cast<float4*>(X + (long)co * plane + (long)(oy0 + q) * a.W + ox);
                    const float4 xv = *px;
                    *px = make_float4(fmaf(acc2[q][c][0], a.inv_s2, xv.x + bv), fmaf(acc2[q][c][1], a.inv_s2, xv.y + bv),
                                      fmaf(acc2[q][c][2], a.inv_s2, xv.z + bv), fmaf(acc2[q][c][3], a.inv_s2, xv.w + bv));
                }
            }
        }
        if (nitem >= a.items) break;
        item = nitem;
        ++round;
        // (no barrier: behind the last iteration's barrier a wave touches only its own parked tile)
    }
}

extern "C" int irm_gdfn_tail_f16x3_f32(const float* h_cl, long h_bs, const float* rec, const float* w2, const float* bias2,
                                       float* x, long x_bs, float inv_s2, int B, int C, int hid, int hid_pad, int H, int W,
                                       hipStream_t stream) {
    if (!h_cl || !rec || !w2 || !x || B <= 0 || C <= 0 || hid <= 0 || H <= 0 || W <= 0) return IRM_EINVAL;
    if (C != 192 || (H & 7) || (W & 31) || hid_pad < hid || (hid_pad & 63)) return IRM_EINVAL;
    if ((h_bs & 3) || (x_bs & 3) || !irm_aligned16(h_cl) || !irm_aligned16(x) || !irm_aligned16(rec) || !irm_aligned16(w2)) return IRM_EINVAL;
    if ((long)(H / 8) * (W / 32) * 256 * 2 * hid_pad >= (1L << 31)) return IRM_EINVAL;       // 32-bit piece offsets
    TailArgs a;
    a.Hh = h_cl; a.h_bs = h_bs; a.X = x; a.x_bs = x_bs; a.rec = rec; a.w2 = w2; a.bias2 = bias2;
    a.C = C; a.H = H; a.W = W; a.S = (hid + 15) / 16; a.HP = hid_pad; a.CB = 2 * hid_pad; a.inv_s2 = inv_s2;
    a.tiles_x = W / IRM_TW; a.tiles = a.tiles_x * (H / IRM_TH); a.items = B * a.tiles;
    constexpr int CT = 12;
    const size_t lds = (size_t)(2 * 512 + CT * 512 + 2 * IRM_PLF + 2048) * sizeof(float);
    IRM_ALLOW_BIG_LDS((&gdfn_tail_kernel<CT>));
    int n = 0;
    if (irm_cu_count(n) != IRM_OK) return IRM_ELAUNCH;
    const int per = (a.items + 7) >> 3;
    a.gpx = (n + 7) / 8;
    if (a.gpx > per) a.gpx = per;
    hipLaunchKernelGGL((gdfn_tail_kernel<CT>), dim3(a.gpx * 8), dim3(512), lds, stream, a);
    return irm_launch_status();
}
