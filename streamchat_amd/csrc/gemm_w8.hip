// FP8 (OCP e4m3fn) weight-only skinny GEMM (include/streamchat_hip_w8_batched.h): the M <= 32 projections of the batched decode step
// (llm.BatchDecoder: chunk captions, beams) with half the weight bytes.
//   C[m, n] = epi(scale[n] * sum_k e4m3(W[n, k]) * A[m, k] + bias[n]) (+ R[m, n])
// Weight-only: an e4m3 byte becomes the fp16 value it denotes (v_cvt_scalef32_pk_f16_fp8 at scale 1, two bytes per instruction, exact), the fp16
// values are the A operand of v_mfma_f32_16x16x32_f16 against the fp16 activations, products and sums are fp32, the row scale multiplies the
// finished sum once.  Nothing is quantised here and the fp8 MFMA is not used.
//
// ONE summation order, shared by every kernel of this file - so they all give the same bits, and row m's bits depend on row m of A alone:
//   * K is cut into slices of 128; a strip of 16 weight rows is served by 8 waves, wave w owns the contiguous slices [w S / 8, (w + 1) S / 8),
//     S = K / 128 (a wave may own none: its partial tile is +0);
//   * a slice is two blocks of 64; in a block lane (rl, g) holds the 16 bytes W[n0 + rl, kb + 16 g .. + 15] and the 16 halves A[m, the same k]:
//     two MFMA steps, bytes 0-7 first, bytes 8-15 second, blocks and slices ascending into one accumulator per 16 rows of A;
//   * the strip's sum is ((((((p0 + p1) + p2) + p3) + p4) + p5) + p6) + p7 over the waves' partial tiles (read back from LDS by whichever wave
//     stores the strip), then ONE fma: sum * scale + bias.
// A 16-byte load per lane is 16 weights (8 in gemm.hip's k_gemm_skinny), so the register-operand kernel needs half the weight requests per k;
// what it pays per k for the ACTIVATIONS is unchanged, which is why the K = 3584 shapes keep them resident (k_gemm_w8_x).
#include "sc_common.h"
#include "../../include/streamchat_hip_w8_batched.h"
#include <stdlib.h>

namespace {

constexpr int W8_NW = 8;                           // waves per strip: the K split that defines the summation order

// 8 e4m3 bytes -> the 8 fp16 values they denote, in byte order
__device__ __forceinline__ sc_h8 w8_cvt8(unsigned lo, unsigned hi) {
    const sc_h2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(lo, 1.0f, true);
    const sc_h2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(hi, 1.0f, true);
    return sc_h8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// one block of 64 k: the lane's 16 weight bytes against its 16 activation halves of each row group
template <int MG>
__device__ __forceinline__ void w8_block(const sc_u4 w, const sc_h8 (&x)[MG][2], sc_f4 (&acc)[MG]) {
    const sc_h8 w0 = w8_cvt8(w[0], w[1]), w1 = w8_cvt8(w[2], w[3]);
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) acc[mg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0, x[mg][0], acc[mg], 0, 0, 0);
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) acc[mg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1, x[mg][1], acc[mg], 0, 0, 0);
}

// what the epilogue of a strip adds, requested by the strip's reducer wave before the weight stream (lane: output columns n .. n + 3)
struct W8Epi {
    float sc[4];
    sc_h4 bias;
};
__device__ __forceinline__ W8Epi w8_epi_load(const float* __restrict__ scale, const _Float16* __restrict__ bias, int n) {
    W8Epi e;
#pragma unroll
    for (int r = 0; r < 4; ++r) e.sc[r] = scale[n + r];
    e.bias = bias ? *reinterpret_cast<const sc_h4*>(bias + n) : sc_h4{0, 0, 0, 0};
    return e;
}

// The strip's partial tiles through LDS: every wave writes its own, ONE barrier, the strip's reducer wave adds them in wave order (whichever
// wave it is: the order of the sum is p0 .. p7) and stores.  `red`: [W8_NW][MG][4][64] floats - a persistent kernel passes the buffer of the
// strip's parity and rotates the reducer, so that the next strip's barrier is what orders this strip's reads before the buffer's next
// writes, and no wave does every epilogue.  The barrier is bare (no vmcnt(0)): loads in flight for the next strip stay in flight.
template <int EPI, bool OUT_F32, int MG>
__device__ __forceinline__ void w8_reduce_store(float* red, const sc_f4 (&acc)[MG], const W8Epi& e, const _Float16* __restrict__ R, int ldr, void* __restrict__ Cout,
                                                int ldc, int M, int n, int wave, int reducer, int lane) {
    const int rl = lane & 15;
#pragma unroll
    for (int mg = 0; mg < MG; ++mg)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[((wave * MG + mg) * 4 + r) * 64 + lane] = acc[mg][r];
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (wave != reducer) return;
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float t = red[(mg * 4 + r) * 64 + lane];
#pragma unroll
            for (int w = 1; w < W8_NW; ++w) t += red[((w * MG + mg) * 4 + r) * 64 + lane];
            v[r] = __builtin_fmaf(t, e.sc[r], (float)e.bias[r]);
        }
        const int m = mg * 16 + rl;
        if (m >= M) continue;
        if (EPI == SC_EPI_SWIGLU) {
            const float o0 = v[0] / (1.0f + __expf(-v[0])) * v[2], o1 = v[1] / (1.0f + __expf(-v[1])) * v[3];
            *reinterpret_cast<sc_h2*>(reinterpret_cast<_Float16*>(Cout) + (size_t)m * (size_t)ldc + (n >> 1)) = sc_h2{(_Float16)o0, (_Float16)o1};
        } else {
            if (R) {
                const sc_h4 r4 = *reinterpret_cast<const sc_h4*>(R + (size_t)m * (size_t)ldr + n);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += (float)r4[r];
            }
            if (OUT_F32) *reinterpret_cast<sc_f4*>(reinterpret_cast<float*>(Cout) + (size_t)m * (size_t)ldc + n) = sc_f4{v[0], v[1], v[2], v[3]};
            else *reinterpret_cast<sc_h4*>(reinterpret_cast<_Float16*>(Cout) + (size_t)m * (size_t)ldc + n) = sc_h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// The generic kernel: any legal shape, run-time loops, both operands straight from global memory into MFMA operand registers.  One workgroup
// per strip.  Rows of A past M re-read row M - 1 and are never stored.
// ------------------------------------------------------------------------------------------------------------------
template <int EPI, bool OUT_F32, int MG>
__global__ __launch_bounds__(64 * W8_NW) void k_gemm_w8(const _Float16* __restrict__ A, int lda, const uint8_t* __restrict__ W, const float* __restrict__ scale,
                                                        const _Float16* __restrict__ bias, const _Float16* __restrict__ R, int ldr, void* __restrict__ Cout, int ldc,
                                                        int M, int N, int K) {
    __shared__ float red[W8_NW * MG * 4 * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rl = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int S = K >> 7, k_lo = (wave * S / W8_NW) << 7, k_hi = ((wave + 1) * S / W8_NW) << 7;
    W8Epi e = {};
    if (wave == 0) e = w8_epi_load(scale, bias, n0 + g * 4);
    const uint8_t* wp = W + (size_t)(n0 + rl) * (size_t)K + g * 16;
    const _Float16* xp[MG];
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) {
        int m = mg * 16 + rl;
        m = m < M ? m : M - 1;
        xp[mg] = A + (size_t)m * (size_t)lda + g * 16;
    }
    sc_f4 acc[MG];
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) acc[mg] = sc_f4{0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;                          // blocks in flight per wave (a wave's range is whole slices: an even number of blocks)
    int k = k_lo;
    for (; k + U * 64 <= k_hi; k += U * 64) {
        sc_u4 wf[U];
        sc_h8 xf[U][MG][2];
#pragma unroll
        for (int u = 0; u < U; ++u) wf[u] = __builtin_nontemporal_load(reinterpret_cast<const sc_u4*>(wp + k + u * 64));
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int mg = 0; mg < MG; ++mg) {
                xf[u][mg][0] = *reinterpret_cast<const sc_h8*>(xp[mg] + k + u * 64);
                xf[u][mg][1] = *reinterpret_cast<const sc_h8*>(xp[mg] + k + u * 64 + 8);
            }
#pragma unroll
        for (int u = 0; u < U; ++u) w8_block<MG>(wf[u], xf[u], acc);
    }
    for (; k < k_hi; k += 64) {
        const sc_u4 wf = __builtin_nontemporal_load(reinterpret_cast<const sc_u4*>(wp + k));
        sc_h8 xf[MG][2];
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) {
            xf[mg][0] = *reinterpret_cast<const sc_h8*>(xp[mg] + k);
            xf[mg][1] = *reinterpret_cast<const sc_h8*>(xp[mg] + k + 8);
        }
        w8_block<MG>(wf, xf, acc);
    }
    w8_reduce_store<EPI, OUT_F32, MG>(red, acc, e, R, ldr, Cout, ldc, M, n0 + g * 4, wave, 0, lane);
}

// ------------------------------------------------------------------------------------------------------------------
// K = 3584 (Qwen2-7B's hidden width: q|k|v, gate/up, lm_head): 28 slices, a wave owns 3 or 4 (waves 1, 3, 5, 7 four).  The activations are
// fetched ONCE per workgroup into registers - the wave's own k range of every row, at most 4 slices = 128 VGPRs at MG = 2 - and the workgroup
// is persistent over a contiguous range of strips; only weights stream, a strip's 8 blocks per lane requested while the previous strip's are
// consumed.  Same operands in the same order as k_gemm_w8: the same bits.
// ------------------------------------------------------------------------------------------------------------------
template <int EPI, bool OUT_F32, int MG>
__global__ __launch_bounds__(64 * W8_NW) void k_gemm_w8_x(const _Float16* __restrict__ A, int lda, const uint8_t* __restrict__ W, const float* __restrict__ scale,
                                                          const _Float16* __restrict__ bias, const _Float16* __restrict__ R, int ldr, void* __restrict__ Cout, int ldc,
                                                          int M, int N, int strips_q, int strips_r) {
    constexpr int K = 3584, S = K / 128, NB = 8;   // NB: blocks of the longest wave range
    __shared__ float red[2][W8_NW * MG * 4 * 64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rl = lane & 15, g = lane >> 4;
    const int b = blockIdx.x;
    const int s_lo = b * strips_q + min(b, strips_r), s_hi = s_lo + strips_q + (b < strips_r ? 1 : 0);
    if (s_lo >= s_hi) return;
    const int k_lo = (wave * S / W8_NW) << 7, k_hi = ((wave + 1) * S / W8_NW) << 7;
    const int nb = (k_hi - k_lo) >> 6;             // 6 or 8, wave-uniform
    const uint8_t* wp = W + (size_t)(s_lo * 16 + rl) * (size_t)K + k_lo + g * 16;
    sc_u4 wn[NB];
#pragma unroll
    for (int u = 0; u < NB; ++u) wn[u] = u < nb ? __builtin_nontemporal_load(reinterpret_cast<const sc_u4*>(wp + u * 64)) : sc_u4{0, 0, 0, 0};
    sc_h8 xf[NB][MG][2];
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) {
        int m = mg * 16 + rl;
        m = m < M ? m : M - 1;
        const _Float16* xp = A + (size_t)m * (size_t)lda + k_lo + g * 16;
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            xf[u][mg][0] = u < nb ? *reinterpret_cast<const sc_h8*>(xp + u * 64) : sc_h8{0, 0, 0, 0, 0, 0, 0, 0};
            xf[u][mg][1] = u < nb ? *reinterpret_cast<const sc_h8*>(xp + u * 64 + 8) : sc_h8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    for (int strip = s_lo; strip < s_hi; ++strip) {
        const int n = strip * 16 + g * 4;
        W8Epi e = {};
        const int reducer = (strip - s_lo) & (W8_NW - 1);
        if (wave == reducer) e = w8_epi_load(scale, bias, n);  // before the next strip's weights: an in-order wait for these leaves those in flight
        __builtin_amdgcn_sched_barrier(0);
        sc_u4 wc[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) wc[u] = wn[u];
        if (strip + 1 < s_hi) {
            wp += (size_t)16 * K;
#pragma unroll
            for (int u = 0; u < NB; ++u)
                if (u < nb) wn[u] = __builtin_nontemporal_load(reinterpret_cast<const sc_u4*>(wp + u * 64));
        }
        __builtin_amdgcn_sched_barrier(0);
        sc_f4 acc[MG];
#pragma unroll
        for (int mg = 0; mg < MG; ++mg) acc[mg] = sc_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < NB; ++u)
            if (u < nb) w8_block<MG>(wc[u], xf[u], acc);
        w8_reduce_store<EPI, OUT_F32, MG>(red[(strip - s_lo) & 1], acc, e, R, ldr, Cout, ldc, M, n, wave, reducer, lane);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// Long rows with few strips (down: K = 18944, 224 strips; any K >= 2048 that is not 3584): both operands through a per-wave LDS stage.
// What bounds the register-operand kernel here is the CU's address path, as gemm.hip found for k_gemm_skinny: lane (rl, g) reads 16 bytes
// of ROW rl, so every load instruction is 64 separate cache-line lookups - and per 64 k that is one instruction for the weights but 2 MG
// for the activations, which the bytes did not halve.  Here a slice (128 k) is fetched with loads that walk along rows - weights: 2
// instructions of 8 rows x 128 B, activations: 4 MG instructions of 4 rows x 256 B, 8 lines each: 80 line lookups per slice at MG = 2
// against 640 - written to the wave's own stage (10 KiB at MG = 2: rows of 128 B / 256 B, the 16-byte piece index XORed with the row so
// that the fragment reads are conflict-free) and read back as MFMA operands.  A stage is written and read by the same wave: LDS executes a
// wave's accesses in order, no barrier.  Two slices of loads are in flight in registers (SL_PF) while the current one is multiplied.
// Plain loads and LDS accesses - the waits are the compiler's.  Same operands in the same order as k_gemm_w8: the same bits.
// ------------------------------------------------------------------------------------------------------------------
template <int MG>
struct W8Slice {
    sc_u4 w[2], x[4 * MG];
};

template <int EPI, bool OUT_F32, int MG>
__global__ __launch_bounds__(64 * W8_NW) void k_gemm_w8_l(const _Float16* __restrict__ A, int lda, const uint8_t* __restrict__ W, const float* __restrict__ scale,
                                                          const _Float16* __restrict__ bias, const _Float16* __restrict__ R, int ldr, void* __restrict__ Cout, int ldc,
                                                          int M, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) char w8_smem[];
    constexpr int WST = 16 * 128, XST = MG * 16 * 256, STB = WST + XST;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rl = lane & 15, g = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int S = K >> 7, s_lo = wave * S / W8_NW, s_hi = (wave + 1) * S / W8_NW;
    char* stage = w8_smem + wave * STB;
    float* red = reinterpret_cast<float*>(w8_smem + W8_NW * STB);
    W8Epi e = {};
    if (wave == 0) e = w8_epi_load(scale, bias, n0 + g * 4);
    // sources and stage slots of the lane's pieces of a slice (k added per slice)
    const uint8_t* wsrc[2];
    int wdst[2], xdst[4 * MG];
    const _Float16* xsrc[4 * MG];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = j * 8 + (lane >> 3), piece = lane & 7;
        wsrc[j] = W + (size_t)(n0 + row) * (size_t)K + piece * 16;
        wdst[j] = row * 128 + ((piece ^ (row & 7)) << 4);
    }
#pragma unroll
    for (int j = 0; j < 4 * MG; ++j) {
        const int row = j * 4 + (lane >> 4), piece = lane & 15;
        const int m = row < M ? row : M - 1;
        xsrc[j] = A + (size_t)m * (size_t)lda + piece * 8;
        xdst[j] = WST + row * 256 + ((piece ^ (row & 15)) << 4);
    }
    // the lane's fragment slots: weights row rl, piece b * 4 + g of 8; activations row mg * 16 + rl, pieces b * 8 + 2 g and + 1 of 16
    int wfo[2], xfo[2][2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        wfo[b] = rl * 128 + (((b * 4 + g) ^ (rl & 7)) << 4);
#pragma unroll
        for (int h = 0; h < 2; ++h) xfo[b][h] = WST + rl * 256 + (((b * 8 + 2 * g + h) ^ rl) << 4);
    }
    auto load = [&](W8Slice<MG>& r, int s) {
#pragma unroll
        for (int j = 0; j < 2; ++j) r.w[j] = __builtin_nontemporal_load(reinterpret_cast<const sc_u4*>(wsrc[j] + s * 128));
#pragma unroll
        for (int j = 0; j < 4 * MG; ++j) r.x[j] = *reinterpret_cast<const sc_u4*>(xsrc[j] + s * 128);
    };
    sc_f4 acc[MG];
#pragma unroll
    for (int mg = 0; mg < MG; ++mg) acc[mg] = sc_f4{0.f, 0.f, 0.f, 0.f};
    auto consume = [&](const W8Slice<MG>& r) {
#pragma unroll
        for (int j = 0; j < 2; ++j) *reinterpret_cast<sc_u4*>(stage + wdst[j]) = r.w[j];
#pragma unroll
        for (int j = 0; j < 4 * MG; ++j) *reinterpret_cast<sc_u4*>(stage + xdst[j]) = r.x[j];
        sc_u4 wf[2];
        sc_h8 xf[2][MG][2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            wf[b] = *reinterpret_cast<const sc_u4*>(stage + wfo[b]);
#pragma unroll
            for (int mg = 0; mg < MG; ++mg)
#pragma unroll
                for (int h = 0; h < 2; ++h) xf[b][mg][h] = *reinterpret_cast<const sc_h8*>(stage + xfo[b][h] + mg * 4096);
        }
#pragma unroll
        for (int b = 0; b < 2; ++b) w8_block<MG>(wf[b], xf[b], acc);
    };
    constexpr int SL_PF = 2;
    W8Slice<MG> r[SL_PF];
#pragma unroll
    for (int u = 0; u < SL_PF; ++u)
        if (s_lo + u < s_hi) load(r[u], s_lo + u);
    for (int s = s_lo; s < s_hi; s += SL_PF) {
#pragma unroll
        for (int u = 0; u < SL_PF; ++u)
            if (s + u < s_hi) {
                const W8Slice<MG> cur = r[u];
                if (s + u + SL_PF < s_hi) load(r[u], s + u + SL_PF);
                consume(cur);
            }
    }
    w8_reduce_store<EPI, OUT_F32, MG>(red, acc, e, R, ldr, Cout, ldc, M, n0 + g * 4, wave, 0, lane);
}

// SC_SKINNY_W8_GENERIC=1 pins the run-time-loop k_gemm_w8 for every call (the reference path of tests/test_gpu_w8_gemm.py); read once
bool w8_generic() {
    static const bool on = [] { const char* e = getenv("SC_SKINNY_W8_GENERIC"); return e && e[0] == '1'; }();
    return on;
}

// (SwiGLU writes fp16 only: its fp32-output kernels are not instantiated)
template <int EPI>
int launch_w8(const void* A, int lda, const uint8_t* W, const float* scale, const void* bias, const void* R, int ldr, void* C, int ldc, int M, int N, int K,
              int out_f32, hipStream_t s) {
    const dim3 block(64 * W8_NW);
    const _Float16 *a = (const _Float16*)A, *b = (const _Float16*)bias, *r = (const _Float16*)R;
    const int strips = N / 16;
    // K = 3584 with more strips than CUs (q|k|v, gate/up, lm_head): activations resident, persistent over strips.  Up to one strip per CU (o)
    // the staged kernel below is faster: us per launch at M = 26 resident / staged, same box - q|k|v 12.6 / 15.1, o 10.7 / 8.8
    // (profiles/r13_batched_decode_w8.md)
    if (!w8_generic() && K == 3584 && strips > sc_device_cu_count()) {
        const int cus = sc_launch_cu_count(s), gx = strips < cus ? strips : cus;
#define SC_W8X(F32, MGV) hipLaunchKernelGGL((k_gemm_w8_x<EPI, F32, MGV>), dim3((unsigned)gx), block, 0, s, a, lda, W, scale, b, r, ldr, C, ldc, M, N, strips / gx, strips % gx)
        if constexpr (EPI != SC_EPI_SWIGLU) { if (out_f32) { if (M <= 16) SC_W8X(true, 1); else SC_W8X(true, 2); } }
        if (EPI == SC_EPI_SWIGLU || !out_f32) { if (M <= 16) SC_W8X(false, 1); else SC_W8X(false, 2); }
#undef SC_W8X
        SC_CHECK_LAUNCH("sc_gemm_w8_f16");
        return SC_OK;
    }
    const dim3 grid((unsigned)strips);
    // K >= 2048: every wave owns at least two slices (the depth of the staged kernel's register prefetch)
    if (!w8_generic() && K >= 2048) {
#define SC_W8L(F32, MGV) do { constexpr int LDSB = W8_NW * (2048 + MGV * 4096) + W8_NW * MGV * 4 * 64 * 4;                                       \
            sc_set_max_lds<k_gemm_w8_l<EPI, F32, MGV>>(LDSB);                                                                                       \
            hipLaunchKernelGGL((k_gemm_w8_l<EPI, F32, MGV>), grid, block, LDSB, s, a, lda, W, scale, b, r, ldr, C, ldc, M, N, K); } while (0)
        if constexpr (EPI != SC_EPI_SWIGLU) { if (out_f32) { if (M <= 16) SC_W8L(true, 1); else SC_W8L(true, 2); } }
        if (EPI == SC_EPI_SWIGLU || !out_f32) { if (M <= 16) SC_W8L(false, 1); else SC_W8L(false, 2); }
#undef SC_W8L
        SC_CHECK_LAUNCH("sc_gemm_w8_f16");
        return SC_OK;
    }
#define SC_W8G(F32, MGV) hipLaunchKernelGGL((k_gemm_w8<EPI, F32, MGV>), grid, block, 0, s, a, lda, W, scale, b, r, ldr, C, ldc, M, N, K)
    if constexpr (EPI != SC_EPI_SWIGLU) { if (out_f32) { if (M <= 16) SC_W8G(true, 1); else SC_W8G(true, 2); } }
    if (EPI == SC_EPI_SWIGLU || !out_f32) { if (M <= 16) SC_W8G(false, 1); else SC_W8G(false, 2); }
#undef SC_W8G
    SC_CHECK_LAUNCH("sc_gemm_w8_f16");
    return SC_OK;
}

}  // namespace

extern "C" int sc_gemm_w8_f16(const void* A, int lda, const uint8_t* W, const float* scale, const void* bias, const void* R, int ldr, void* C, int ldc, int M, int N,
                              int K, int epilogue, int out_f32, sc_stream_t stream) {
    SC_REQUIRE(A && W && scale && C, "sc_gemm_w8_f16: null pointer argument");
    SC_REQUIRE(M >= 1 && M <= 32, "sc_gemm_w8_f16: M (%d) must be in 1..32 (a caller with more rows launches row blocks)", M);
    SC_REQUIRE(N > 0 && N % 16 == 0, "sc_gemm_w8_f16: N (%d) must be a positive multiple of 16", N);
    SC_REQUIRE(K > 0 && K % 128 == 0, "sc_gemm_w8_f16: K (%d) must be a positive multiple of 128", K);
    if (epilogue != SC_EPI_NONE && epilogue != SC_EPI_SWIGLU) return sc_fail(SC_ERR_UNSUPPORTED, "sc_gemm_w8_f16: epilogue %d is not built (NONE and SWIGLU are)", epilogue);
    const bool sw = epilogue == SC_EPI_SWIGLU;
    SC_REQUIRE(!sw || (!R && !out_f32), "sc_gemm_w8_f16: SwiGLU epilogue takes no residual and writes fp16");
    SC_REQUIRE(lda >= K && lda % 8 == 0 && ldc >= (sw ? N / 2 : N) && ldc % 4 == 0, "sc_gemm_w8_f16: bad leading dimensions (lda %% 8 == 0, ldc %% 4 == 0)");
    SC_REQUIRE(!R || (ldr >= N && ldr % 4 == 0), "sc_gemm_w8_f16: bad residual leading dimension (ldr %% 4 == 0)");
    SC_REQUIRE(((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(W)) & 15) == 0, "sc_gemm_w8_f16: A and W must be 16-byte aligned");
    SC_REQUIRE((reinterpret_cast<uintptr_t>(scale) & 3) == 0 && ((reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(R)) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(C) & (out_f32 ? 15 : sw ? 3 : 7)) == 0,
               "sc_gemm_w8_f16: bias, residual and fp16 C must be 8-byte aligned, fp32 C 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    if (sw) return launch_w8<SC_EPI_SWIGLU>(A, lda, W, scale, bias, R, ldr, C, ldc, M, N, K, 0, s);
    return launch_w8<SC_EPI_NONE>(A, lda, W, scale, bias, R, ldr, C, ldc, M, N, K, out_f32 ? 1 : 0, s);
}
