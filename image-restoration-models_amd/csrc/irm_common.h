// Shared helpers for the gfx950 kernels of libirm_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <utility>

#define IRM_OK 0
#define IRM_EINVAL (-1)
#define IRM_ELAUNCH (-2)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float irm_v2 __attribute__((ext_vector_type(2)));
typedef _Float16 irm_h4 __attribute__((ext_vector_type(4)));
typedef _Float16 irm_h8 __attribute__((ext_vector_type(8)));
typedef unsigned irm_u2 __attribute__((ext_vector_type(2)));
typedef unsigned irm_u4 __attribute__((ext_vector_type(4)));

// activation codes shared by the GEMM / conv epilogues
#define IRM_ACT_NONE 0
#define IRM_ACT_RELU 1
#define IRM_ACT_GELU 2   // exact erf GELU (torch F.gelu default)
#define IRM_ACT_SILU 3

// LayerNorm prologue modes (restormer.py:25-70)
#define IRM_LN_NONE 0
#define IRM_LN_WITHBIAS 1
#define IRM_LN_BIASFREE 2

// Kernels that use more than 64 KiB of LDS: raise the limit once per (kernel instantiation, device).
#define IRM_ALLOW_BIG_LDS(kernel_ptr)                                                                              \
    do {                                                                                                           \
        static unsigned char irm_done_[64] = {0};                                                                  \
        int irm_dev_ = 0;                                                                                          \
        if (hipGetDevice(&irm_dev_) != hipSuccess || irm_dev_ < 0 || irm_dev_ >= 64) return IRM_ELAUNCH;           \
        if (!irm_done_[irm_dev_]) {                                                                                \
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel_ptr),                                     \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)         \
                return IRM_ELAUNCH;                                                                                \
            irm_done_[irm_dev_] = 1;                                                                               \
        }                                                                                                          \
    } while (0)

static inline int irm_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? IRM_OK : IRM_ELAUNCH;
}

// Compute units of the current device, for the persistent-grid launchers (one workgroup per CU): asked once per device.
static inline int irm_cu_count(int& n) {
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return IRM_ELAUNCH;
    if (!cus[dev]) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return IRM_ELAUNCH;
        cus[dev] = v;
    }
    n = cus[dev];
    return IRM_OK;
}

__device__ __forceinline__ float irm_gelu(float x) {
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}

__device__ __forceinline__ float irm_act(float v, int act) {
    if (act == IRM_ACT_RELU) return fmaxf(v, 0.0f);
    if (act == IRM_ACT_GELU) return irm_gelu(v);
    if (act == IRM_ACT_SILU) return v / (1.0f + __expf(-v));
    return v;
}

// D(16x16) += A(16x4) * B(4x16), exact f32.  Lane l supplies A[l&15][l>>4] and
// B[l>>4][l&15]; it receives D[(l>>4)*4 + r][l&15] in element r of the result.
__device__ __forceinline__ f32x4 irm_mfma16(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// 4 consecutive floats at row[n..n+3]; VEC: one 16-byte access (row + n 16-byte aligned, n + 3 < N
// whenever n < N), else guarded scalars (elements at or beyond N read as 0 / are not written).
template <bool VEC>
__device__ __forceinline__ float4 irm_ld4(const float* row, int n, int N) {
    if (VEC) return *reinterpret_cast<const float4*>(row + n);
    float4 v;
    v.x = n < N ? row[n] : 0.0f;
    v.y = n + 1 < N ? row[n + 1] : 0.0f;
    v.z = n + 2 < N ? row[n + 2] : 0.0f;
    v.w = n + 3 < N ? row[n + 3] : 0.0f;
    return v;
}
template <bool VEC>
__device__ __forceinline__ void irm_st4(float* row, int n, int N, float4 v) {
    if (VEC) { *reinterpret_cast<float4*>(row + n) = v; return; }
    if (n < N) row[n] = v.x;
    if (n + 1 < N) row[n + 1] = v.y;
    if (n + 2 < N) row[n + 2] = v.z;
    if (n + 3 < N) row[n + 3] = v.w;
}
// fp16 hi/lo splits behind a FIXED scale (2^-4: gated activations, v, un-normalised GEMM inputs): the scaled value is
// saturated at +-65000 before the split, so an out-of-range activation (|x| > ~1e6) gives a clamped, finite operand instead
// of fp16 infinities and a NaN tile (one v_med3_f32; the scaled splits behind a LayerNorm or a pack-time bound cannot
// overflow and do not clamp).
__device__ __forceinline__ float irm_sat_h(float x) { return __builtin_amdgcn_fmed3f(x, -65000.0f, 65000.0f); }

// fp16 hi/lo split of fp32 values that are ALREADY rounded (register operands, opaque to the compiler): hi = rn16(x),
// lo = rn16(x - hi).  The difference is exact in fp32, so v_fma_mix{lo,hi}_f16 (f16 source widened, one rounding of the
// result) gives exactly the two-step value: cvt_pk + 2 mix instructions per PAIR instead of 2 x (cvt, cvt back, sub, cvt);
// hipcc does not form it from the source expression, and left alone it may fuse a preceding multiply into the lo part
// only (hi from the rounded product, lo from the exact one: 2^-11 outliers on double-rounding ties).
__device__ __forceinline__ void irm_split2(float a, float b, unsigned& hi, unsigned& lo) {
    unsigned h, l;
    asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(h) : "v"(a), "v"(b));
    asm("v_fma_mixlo_f16 %0, -%1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(l) : "v"(h), "v"(a));
    asm("v_fma_mixhi_f16 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(l) : "v"(h), "v"(b));
    hi = h;
    lo = l;
}
template <typename H8>
__device__ __forceinline__ void irm_split8(const float (&x)[8], H8& hi, H8& lo) {
    static_assert(sizeof(H8) == 16, "8 halves");
    irm_u4 h, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) { unsigned hh, ll; irm_split2(x[2 * e], x[2 * e + 1], hh, ll); h[e] = hh; l[e] = ll; }
    hi = __builtin_bit_cast(H8, h);
    lo = __builtin_bit_cast(H8, l);
}
template <typename H4>
__device__ __forceinline__ void irm_split4(const float (&x)[4], H4& hi, H4& lo) {
    static_assert(sizeof(H4) == 8, "4 halves");
    irm_u2 h, l;
#pragma unroll
    for (int e = 0; e < 2; ++e) { unsigned hh, ll; irm_split2(x[2 * e], x[2 * e + 1], hh, ll); h[e] = hh; l[e] = ll; }
    hi = __builtin_bit_cast(H4, h);
    lo = __builtin_bit_cast(H4, l);
}

__host__ __device__ static inline bool irm_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// 16 zero bytes in global memory: where a halo chunk lies outside the image, its load (LDS-DMA or register) is pointed
// here.  The library is built without relocatable device code, so every kernel file is its own code object and gets
// its own copy.  Name it in the kernel body itself, not inside a lambda (pass the pointer in): hipcc counts a lambda's use
// as a host-side use, makes the symbol global and then reaches it through the GOT (one more scalar load and wait).
static __device__ __attribute__((aligned(16))) float irm_zero_page[4] = {0.f, 0.f, 0.f, 0.f};

// The epilogue activation as a CALL, for the unrolled epilogues of the ring GEMMs whose activation code is a run-time value
// (used only when it is not IRM_ACT_NONE): inlined, the three-way select with erf and exp would be copied once per value.
static __device__ __attribute__((noinline)) float irm_act_noinline(float v, int act) { return irm_act(v, act); }

template <int N>
__device__ __forceinline__ void irm_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int N>
__device__ __forceinline__ void irm_wait_lgkmcnt() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): a loop whose index is a compile-time constant in the body
template <int I> using irm_ic = std::integral_constant<int, I>;
template <class F, int... Is>
__device__ __forceinline__ void irm_for_impl(F&& f, std::integer_sequence<int, Is...>) { (f(irm_ic<Is>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void irm_for(F&& f) { irm_for_impl(f, std::make_integer_sequence<int, N>{}); }

// LDS accesses as (per-lane byte offset in a VGPR) + (compile-time immediate < 64 KiB): the offsets are made opaque
// once, otherwise the compiler materialises one address register per distinct constant beyond the 16-bit DS
// offset field of the 150 KiB layout and spills them.
typedef __attribute__((address_space(3))) char irm_lc;
__device__ __forceinline__ unsigned irm_opaque(unsigned v) { asm volatile("" : "+v"(v)); return v; }
template <typename T>
__device__ __forceinline__ T irm_ld(const irm_lc* base, unsigned voff, int imm) {
    return *reinterpret_cast<const __attribute__((address_space(3))) T*>(base + voff + imm);
}
template <typename T>
__device__ __forceinline__ void irm_st(irm_lc* base, unsigned voff, int imm, T v) {
    *reinterpret_cast<__attribute__((address_space(3))) T*>(base + voff + imm) = v;
}

// Hand-counted LDS reads for the main loop of the fused branch kernels: hipcc (ROCm 7.2) waits lgkmcnt(0) before the
// first use of ANY pending ds_read there, which serialises the prefetch of the next chunk behind the lock-step read
// burst of all 8 waves.  These reads are invisible to its bookkeeping; irm_wait_lgkmcnt<N>() waits until at most N newer
// LDS operations are outstanding and irm_tie(regs...) ties the registers to the wait (consumers cannot be scheduled
// above it).
template <int IMM, typename T>
__device__ __forceinline__ void irm_dsr(T& d, unsigned voff) {
    static_assert(sizeof(T) == 16 && IMM >= 0 && IMM < 65536, "ds_read_b128");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(voff), "n"(IMM) : "memory");
}
template <typename T>
__device__ __forceinline__ void irm_tie1(T& r) { asm volatile("" : "+v"(r)); }
template <typename... T>
__device__ __forceinline__ void irm_tie(T&... r) { (irm_tie1(r), ...); }

// LDS-DMA of NP pieces of 1 KiB by a workgroup of 8 waves, piece i issued by wave i % 8 (LDS destination = wave-uniform
// base + lane * 16)
template <int NP>
__device__ __forceinline__ void irm_dma(const float* src, float* dst, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < (NP + 7) / 8; ++i) {
        const int pc = wave + 8 * i;
        if (pc < NP)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + pc * 256 + lane * 4),
                                             (__attribute__((address_space(3))) void*)(dst + pc * 256), 16, 0, 0);
    }
}

// GELU on a register pair with erf from Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7, i.e. fp32 rounding level): branch
// free, packed fp32 except the two transcendentals per element.
__device__ __forceinline__ irm_v2 irm_gelu2(irm_v2 x) {
    const irm_v2 z = __builtin_elementwise_abs(x) * 0.70710678118654752440f;
    const irm_v2 d = z * 0.3275911f + 1.0f;
    const irm_v2 t = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    irm_v2 p = t * 1.061405429f + -1.453152027f;
    p = p * t + 1.421413741f;
    p = p * t + -0.284496736f;
    p = p * t + 0.254829592f;
    const irm_v2 q = z * z * -1.4426950408889634f;
    const irm_v2 e = p * t * (irm_v2){__builtin_amdgcn_exp2f(q.x), __builtin_amdgcn_exp2f(q.y)};   // 1 - erf(|z|)
    const irm_v2 w = 1.0f - e;
    const irm_v2 sg = {copysignf(w.x, x.x), copysignf(w.y, x.y)};
    const irm_v2 h = x * 0.5f;
    return sg * h + h;
}

// gelu(x) = max(x, 0) - 0.5 |x| erfc(|x| / sqrt 2), erfc by Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7): with
// u = |x| sqrt(log2(e) / 2) the exponential is exp2(-u u), the rational argument 1 + p z = 1 + (p / sqrt(log2 e)) u, and
// the factor 0.5 |x| = u * (0.5 / c_u) is folded into the polynomial's coefficients: 14 instructions (two of them
// transcendental) instead of 18 for the sign-select form 0.5 x (1 + copysign(1 - e, x)); no cancellation beyond a factor
// of two anywhere (x > 0: x - [<= x / 2]).
__device__ __forceinline__ float irm_gelu1(float x) {
    constexpr double CU = 0.84932180028801904272;            // sqrt(log2(e) / 2)
    constexpr double F = 0.5 / CU;
    constexpr float k = (float)(0.3275911 / 1.2011224087864498);
    constexpr float a1 = (float)(0.254829592 * F), a2 = (float)(-0.284496736 * F), a3 = (float)(1.421413741 * F),
                    a4 = (float)(-1.453152027 * F), a5 = (float)(1.061405429 * F);
    const float u = fabsf(x) * (float)CU;
    const float t = __builtin_amdgcn_rcpf(fmaf(u, k, 1.0f));
    float p = fmaf(t, a5, a4);
    p = fmaf(p, t, a3);
    p = fmaf(p, t, a2);
    p = fmaf(p, t, a1);
    const float w = (p * t) * __builtin_amdgcn_exp2f(-u * u);     // 0.5 / c_u * erfc(|x| / sqrt 2)
    return fmaf(-u, w, __builtin_amdgcn_fmed3f(x, 0.0f, 3.0e38f));      // (med3: max(x, 0) without fmaxf's canonicalising v_max)
}

// The fp32-emulated product on the fp16 matrix cores: acc += A B with A = ah + al, B = bh + bl (fp16 hi/lo splits), as
// three v_mfma_f32_16x16x32_f16 in the order lo*hi, hi*lo, hi*hi (the small terms first; lo*lo is dropped).
__device__ __forceinline__ f32x4 irm_mfma3_f16(irm_h8 ah, irm_h8 al, irm_h8 bh, irm_h8 bl, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bl, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bh, acc, 0, 0, 0);
}

// LayerNorm statistics (mean and rstd over the M channels, into st [2][N]) of a finished output tile straight from the
// registers: lane (r, g) holds PT pixel quads t[p][c] of the channels 16 (mt0 + c) + r, c < CT, so a channel reduction
// is CT in-lane adds plus a 16-lane butterfly.  Two passes (mean, then centred squares) in registers; lane r == 0 stores.
// Where a quad lives, and what of it lies inside the image, is the caller's rule:
//   QUAD   pix[p] is the quad's first pixel, or negative for a quad outside the image: two 16-byte stores (dwgemm.hip);
//   else   pix[p] + e is pixel e, written when it is below N: guarded scalars (gemm_pw.hip).
__device__ __forceinline__ float irm_quad_elem(const f32x4& v, int e) { return v[e]; }
__device__ __forceinline__ float irm_quad_elem(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
template <bool QUAD, int PT, int CT, class Tile, class Pix, class Len>
__device__ __forceinline__ void irm_tile_stats(const Tile (&t)[PT][CT], int mt0, int M, Len N, int r, const Pix (&pix)[PT],
                                               float* st, float eps) {
    float sum[PT][4], sq[PT][4];
#pragma unroll
    for (int p = 0; p < PT; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) { sum[p][e] = 0.f; sq[p][e] = 0.f; }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const bool ok = (mt0 + c) * 16 + r < M;
#pragma unroll
        for (int p = 0; p < PT; ++p)
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[p][e] += ok ? irm_quad_elem(t[p][c], e) : 0.f;
    }
    const float inv = 1.0f / (float)M;
#pragma unroll
    for (int p = 0; p < PT; ++p)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) sum[p][e] += __shfl_xor(sum[p][e], o);
            sum[p][e] *= inv;                                   // mean
        }
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const bool ok = (mt0 + c) * 16 + r < M;
#pragma unroll
        for (int p = 0; p < PT; ++p)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = irm_quad_elem(t[p][c], e) - sum[p][e];
                sq[p][e] += ok ? d * d : 0.f;
            }
    }
#pragma unroll
    for (int p = 0; p < PT; ++p) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) sq[p][e] += __shfl_xor(sq[p][e], o);
            sq[p][e] = 1.0f / sqrtf(sq[p][e] * inv + eps);      // rstd
        }
        if constexpr (QUAD) {
            if (r == 0 && pix[p] >= 0) {
                *reinterpret_cast<float4*>(st + pix[p]) = make_float4(sum[p][0], sum[p][1], sum[p][2], sum[p][3]);
                *reinterpret_cast<float4*>(st + N + pix[p]) = make_float4(sq[p][0], sq[p][1], sq[p][2], sq[p][3]);
            }
        } else if (r == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (pix[p] + e < N) {
                    st[pix[p] + e] = sum[p][e];
                    st[N + pix[p] + e] = sq[p][e];
                }
        }
    }
}

// ---- the 8 x 32 pixel tile of the fused GDFN / qkv branch kernels (fused_block.hip, fused_tail.hip)
constexpr int IRM_TH = 8, IRM_TW = 32;
constexpr int IRM_HC = IRM_TW + 2;                 // halo columns
constexpr int IRM_NP = (IRM_TH + 2) * IRM_HC;      // halo pixels (340)
constexpr int IRM_PS = 40;                         // floats per pixel in the LDS image (32 channels + 8 pad)
constexpr int IRM_PLF = (IRM_NP + 16) * IRM_PS;    // floats per LDS image (+ 16 junk pixels: lanes without a pixel store there, no branch)

// The gate of a pair of gate channels, a = dw(h1), m = dw(h2) / 16: gelu(a) * m, saturated, split into packed fp16 hi/lo
// (the k-slots of project_out's MFMA).
__device__ __forceinline__ void irm_gate_split2(float a0, float a1, float m0, float m1, unsigned& hi, unsigned& lo) {
    const float g0 = irm_sat_h(__fmul_rn(irm_gelu1(a0), m0));
    const float g1 = irm_sat_h(__fmul_rn(irm_gelu1(a1), m1));
    irm_split2(g0, g1, hi, lo);
}

// One chunk of the depth-wise stencil of a lane's two vertically adjacent output rows (o[q]: 4 channels each): halo row
// dy (its three pixels P, 4 channels each) feeds tap row dy (kc) of row 0 and tap row dy - 1 (kprev) of row 1; dy == 0
// starts both sums from the bias kb.
__device__ __forceinline__ void irm_stencil_step(int dy, float (&o)[2][4], f32x4 (&kprev)[3], const f32x4 (&P)[3],
                                                 const f32x4 (&kc)[3], const f32x4& kb) {
    // scalar v_fma_f32 (the users are built with -fno-slp-vectorize): as many issue slots as packed FMAs, and
    // they pair with the MFMAs of the interleaved GEMM unit
    if (dy == 0) {
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) o[q][e] = kb[e];
    }
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (dy < 3) o[0][e] = fmaf(kc[dx][e], P[dx][e], o[0][e]);
            if (dy > 0) o[1][e] = fmaf(kprev[dx][e], P[dx][e], o[1][e]);
        }
    }
    if (dy < 3) {
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) kprev[dx] = kc[dx];
    }
    // pin the partial sums here: otherwise the compiler sinks the whole FMA chain to its consumer (the next
    // iteration's project_out) and keeps every LDS read of the stage alive until then
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(o[q][e]));
}
