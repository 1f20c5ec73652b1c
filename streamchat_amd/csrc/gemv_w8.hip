// FP8 (OCP e4m3fn) weight-only decode projections (include/streamchat_hip_w8.h): the kernels of gemv.hip with half the weight bytes.
//   y[n] = scale[n] * sum_k q[n, k] * xh[k]  (+ bias) (+ residual) | SwiGLU,      q: e4m3 bytes, one fp32 scale per output row.
// Batch-1 decode is a pure weight stream (gemv.hip), so the bytes ARE the time: opt-in (llm.Qwen2Model.enable_fp8_decode), because the
// quantisation is an accuracy trade; the kernels themselves are exact up to the summation order - an e4m3 value is a fp16 value
// (v_cvt_scalef32_pk_f16_fp8 with scale 1, two weights per instruction), its product with a fp16 activation is exact in fp32
// (v_dot2_f32_f16), the row scale multiplies the finished fp32 sum once.
// Geometry: a lane loads 16 B = 16 weights, so a K-slice of 512 is HALF a wave: lanes 0-31 stream one set of R rows, lanes 32-63 the
// next R rows.  A wave therefore has the bytes in flight of gemv.hip's wave with the same R and twice the rows; K = 3584 is 7 slices and
// K = 18944 is 37, the straight-line structure of k_gemv_u (all loads of a batch requested, the next batch requested before the
// current one is consumed, no control flow around a load).  The activation vector is always staged in LDS (normalised or copied).
// Every lane adds its slices in ascending order into two partial sums (bytes 0-7 | 8-15 of each load), the half-wave is reduced with
// the xor tree: the result bits depend neither on the workgroup size (SC_GEMV_WPB_*) nor on which of the kernels below ran.
#include "sc_common.h"
#include "gemv_norm.h"
#include "../../include/streamchat_hip_w8.h"
#include <stdlib.h>

namespace {

// 16 e4m3 weights (one 16-byte load) . 16 fp16 activations: bytes 0-7 into `lo`, 8-15 into `hi`
__device__ __forceinline__ void dot16(const sc_u4 w, const sc_h8 x0, const sc_h8 x1, float& lo, float& hi) {
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        lo = __builtin_amdgcn_fdot2(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[d], 1.0f, false), sc_h2{x0[4 * d], x0[4 * d + 1]}, lo, false);
        lo = __builtin_amdgcn_fdot2(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[d], 1.0f, true), sc_h2{x0[4 * d + 2], x0[4 * d + 3]}, lo, false);
        hi = __builtin_amdgcn_fdot2(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[2 + d], 1.0f, false), sc_h2{x1[4 * d], x1[4 * d + 1]}, hi, false);
        hi = __builtin_amdgcn_fdot2(__builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[2 + d], 1.0f, true), sc_h2{x1[4 * d + 2], x1[4 * d + 3]}, hi, false);
    }
}

// the activation vector into LDS, once per workgroup: the fused RMSNorm of gemv.hip (same arithmetic, same order), or a copy
__device__ __forceinline__ void stage_x(const _Float16* __restrict__ x, const _Float16* __restrict__ gamma, int K, float eps, _Float16* xn) {
    if (gamma) {
        block_rmsnorm_to_lds(x, gamma, K, eps, xn, reinterpret_cast<float*>(xn + K));
    } else {
        for (int k = threadIdx.x * 8; k < K; k += (int)blockDim.x * 8) *reinterpret_cast<sc_h8*>(xn + k) = *reinterpret_cast<const sc_h8*>(x + k);
        __syncthreads();
    }
}

// y of a row from its finished sum: ONE fma, shared by the GEMV and the fused q | k | v kernel (which must give the same bits)
__device__ __forceinline__ float row_value(float sum, float scale, float add) { return __builtin_fmaf(sum, scale, add); }

// the weight stream of a half-wave: R rows (wp[r] already offset by 16 * lane-in-half).  NS > 0: K = NS * 512, straight-line code in
// batches of UNR slices with two register buffers (StreamU of gemv.hip); NS == 0: any K % 16 == 0, a loop with a guarded last slice.
template <int R, int NS, int UNR>
struct StreamW8 {
    static constexpr int NBATCH = NS ? (NS + UNR - 1) / UNR : 0;
    sc_u4 buf[2][UNR][R];
    template <int B>
    __device__ __forceinline__ void load(const uint8_t* const (&wp)[R]) {
#pragma unroll
        for (int u = 0; u < UNR; ++u)
            if (B * UNR + u < NS) {
#pragma unroll
                for (int r = 0; r < R; ++r) buf[B & 1][u][r] = __builtin_nontemporal_load(reinterpret_cast<const sc_u4*>(wp[r] + (B * UNR + u) * 512));
            }
    }
    template <int B>
    __device__ __forceinline__ void run(const uint8_t* const (&wp)[R], const _Float16* xn, int hl, float (&lo)[R], float (&hi)[R]) {
        if constexpr (B < NBATCH) {
            if constexpr (B + 1 < NBATCH) load<B + 1>(wp);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < UNR; ++u)
                if (B * UNR + u < NS) {
                    const _Float16* xs = xn + (B * UNR + u) * 512 + hl * 16;
                    const sc_h8 x0 = *reinterpret_cast<const sc_h8*>(xs), x1 = *reinterpret_cast<const sc_h8*>(xs + 8);
#pragma unroll
                    for (int r = 0; r < R; ++r) dot16(buf[B & 1][u][r], x0, x1, lo[r], hi[r]);
                }
            __builtin_amdgcn_sched_barrier(0);
            run<B + 1>(wp, xn, hl, lo, hi);
        }
    }
    __device__ __forceinline__ void run_any(const uint8_t* const (&wp)[R], const _Float16* xn, int hl, int K, float (&lo)[R], float (&hi)[R]) {
#pragma unroll 2
        for (int k = hl * 16; k < K; k += 512) {
            sc_u4 w[R];
#pragma unroll
            for (int r = 0; r < R; ++r) w[r] = __builtin_nontemporal_load(reinterpret_cast<const sc_u4*>(wp[r] + (k - hl * 16)));
            const sc_h8 x0 = *reinterpret_cast<const sc_h8*>(xn + k), x1 = *reinterpret_cast<const sc_h8*>(xn + k + 8);
#pragma unroll
            for (int r = 0; r < R; ++r) dot16(w[r], x0, x1, lo[r], hi[r]);
        }
    }
};

// sum of the two partials, reduced over the 32 lanes of the half-wave (every lane of the half ends with the row's sum)
__device__ __forceinline__ float half_wave_sum(float lo, float hi) {
    float v = lo + hi;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <bool SWIGLU, bool OUT_F32, int R, int NS, int UNR>
__global__ __launch_bounds__(512) void k_gemv_w8(const uint8_t* __restrict__ W, const float* __restrict__ scale, const _Float16* __restrict__ x,
                                                 const _Float16* __restrict__ bias, const _Float16* __restrict__ res, void* __restrict__ y_base, int N, int K_any,
                                                 const int* __restrict__ y_row, int y_ld, const _Float16* __restrict__ gamma, float eps) {
    const int K = NS ? NS * 512 : K_any;
    extern __shared__ __attribute__((aligned(16))) char w8_smem[];
    _Float16* xn = reinterpret_cast<_Float16*>(w8_smem);
    const int lane = threadIdx.x & 63, hl = lane & 31;
    const int row0 = ((blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6)) * 2 + (lane >> 5)) * R;
    const uint8_t* wp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) wp[r] = W + (size_t)(row0 + r < N ? row0 + r : N - 1) * (size_t)K + hl * 16;
    // what the epilogue needs is requested first, with branch-free loads (a null pointer reads x[0], the value is dropped): see k_gemv_u
    float sc[R];
    _Float16 eb_b[R], eb_r[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int n = row0 + r < N ? row0 + r : N - 1;
        sc[r] = scale[n]; eb_b[r] = *(bias ? bias + n : x); eb_r[r] = *(res ? res + n : x);
    }
    // optional dynamic output row (KV-cache append at a device-resident position: keeps a decode step hipGraph-replayable)
    void* y = y_row ? (void*)(reinterpret_cast<_Float16*>(y_base) + (size_t)y_row[0] * (size_t)y_ld) : y_base;
    StreamW8<R, NS, UNR> ws;
    if constexpr (NS > 0) { ws.template load<0>(wp); __builtin_amdgcn_sched_barrier(0); }     // the first batch is under way while x is staged
    stage_x(x, gamma, K, eps, xn);
    // (no early exit for rows past the last one: they stream row N - 1 again and store nothing, see k_gemv_u)
    float lo[R], hi[R];
#pragma unroll
    for (int r = 0; r < R; ++r) lo[r] = hi[r] = 0.f;
    if constexpr (NS > 0) ws.template run<0>(wp, xn, hl, lo, hi);
    else ws.run_any(wp, xn, hl, K, lo, hi);
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        asm volatile("" ::"v"(sc[r]), "v"((unsigned)__builtin_bit_cast(unsigned short, eb_b[r])), "v"((unsigned)__builtin_bit_cast(unsigned short, eb_r[r])));   // (see k_gemv_u)
        acc[r] = half_wave_sum(lo[r], hi[r]);
    }
    if (hl == 0 && row0 < N) {
        if (SWIGLU) {          // rows (g g u u): two outputs per 4 rows (R == 4)
            const float g0 = row_value(acc[0], sc[0], 0.f), g1 = row_value(acc[R > 1 ? 1 : 0], sc[R > 1 ? 1 : 0], 0.f);
            const float u0 = row_value(acc[R > 2 ? 2 : 0], sc[R > 2 ? 2 : 0], 0.f), u1 = row_value(acc[R > 3 ? 3 : 0], sc[R > 3 ? 3 : 0], 0.f);
            _Float16* o = reinterpret_cast<_Float16*>(y) + (row0 >> 1);
            o[0] = (_Float16)(g0 / (1.0f + __expf(-g0)) * u0);
            o[1] = (_Float16)(g1 / (1.0f + __expf(-g1)) * u1);
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int n = row0 + r;
                if (n < N) {
                    const float v = row_value(acc[r], sc[r], (bias ? (float)eb_b[r] : 0.f) + (res ? (float)eb_r[r] : 0.f));
                    if (OUT_F32) reinterpret_cast<float*>(y)[n] = v;
                    else reinterpret_cast<_Float16*>(y)[n] = (_Float16)v;
                }
            }
        }
    }
}

// k_decode_qkv of gemv.hip with e4m3 weights: a wave owns one rotation pair - lanes 0-31 the row (h, j), lanes 32-63 the row (h, j + Dh/2) -
// and lane 0 rotates the two fp32 values (scale * sum + bias, the GEMV's row_value) with the fp32 table and rounds ONCE: the bits of
// k_gemv_w8(out_f32) followed by k_rope_f32in.  V rows ride along unrotated.
template <int NS, int UNR>
__global__ __launch_bounds__(512) void k_decode_qkv_w8(const uint8_t* __restrict__ Wq, const float* __restrict__ sq, const uint8_t* __restrict__ Wkv,
                                                       const float* __restrict__ skv, const _Float16* __restrict__ bq, const _Float16* __restrict__ bkv,
                                                       const _Float16* __restrict__ x, const _Float16* __restrict__ gamma, float eps, _Float16* __restrict__ q_out,
                                                       _Float16* __restrict__ cache, int ld, const int* __restrict__ pos, int Hq, int Hkv, int Dh, int K_any,
                                                       const float* __restrict__ tab_q, const float* __restrict__ tab_k, int tab_rows) {
    const int K = NS ? NS * 512 : K_any;
    const int lane = threadIdx.x & 63, hl = lane & 31;
    const int half = Dh >> 1;
    const int task = blockIdx.x * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);   // (head, j) over q heads, then k heads, then v heads
    const int ntask = (Hq + 2 * Hkv) * half;
    const bool live = task < ntask;                                       // (dead waves stream task 0 again and store nothing)
    const int hh = (live ? task : 0) / half, j = (live ? task : 0) - hh * half;
    int kind, h, n;                                                       // 0 = q, 1 = k, 2 = v; n: this half-wave's weight row
    if (hh < Hq) { kind = 0; h = hh; n = h * Dh + j; }
    else if (hh < Hq + Hkv) { kind = 1; h = hh - Hq; n = h * Dh + j; }
    else { kind = 2; h = hh - Hq - Hkv; n = (Hkv + h) * Dh + j; }
    n += (lane >> 5) * half;
    const uint8_t* wp[1] = {(kind == 0 ? Wq : Wkv) + (size_t)n * (size_t)K + hl * 16};
    const _Float16* bsel = kind == 0 ? bq : bkv;
    const float sc = (kind == 0 ? sq : skv)[n];
    const _Float16 braw = *(bsel ? bsel + n : x);
    extern __shared__ __attribute__((aligned(16))) char w8_qkv_smem[];
    _Float16* xn = reinterpret_cast<_Float16*>(w8_qkv_smem);
    StreamW8<1, NS, UNR> ws;
    if constexpr (NS > 0) { ws.template load<0>(wp); __builtin_amdgcn_sched_barrier(0); }
    const int row = pos[0];
    const int trow = row < 0 ? 0 : (row >= tab_rows ? tab_rows - 1 : row);      // the position lives in device memory: clamp to the table, never read past it
    const float* t = (kind == 0 ? tab_q : tab_k) + (size_t)trow * (size_t)Dh;   // (a V row reads a table row it ignores)
    const float tcs = t[j], tsn = t[half + j];
    __builtin_amdgcn_sched_barrier(0);
    stage_x(x, gamma, K, eps, xn);
    float lo[1] = {0.f}, hi[1] = {0.f};
    if constexpr (NS > 0) ws.template run<0>(wp, xn, hl, lo, hi);
    else ws.run_any(wp, xn, hl, K, lo, hi);
    asm volatile("" ::"v"(sc), "v"((unsigned)__builtin_bit_cast(unsigned short, braw)), "v"(tcs), "v"(tsn));   // (see k_gemv_u)
    const float a32 = row_value(half_wave_sum(lo[0], hi[0]), sc, (bsel ? (float)braw : 0.f) + 0.f);
    const float b32 = __shfl(a32, 32, 64);                                // the pair's second row, from the upper half-wave
    if (lane == 0 && live) {
        _Float16* dst = kind == 0 ? q_out + h * Dh + j : cache + (size_t)row * (size_t)ld + (kind == 1 ? 0 : Hkv * Dh) + h * Dh + j;
        if (kind == 2) { dst[0] = (_Float16)a32; dst[half] = (_Float16)b32; return; }
        // fp32 fma FIRST, then the rounding to fp16 (see k_decode_qkv)
        float ra = __builtin_fmaf(-b32, tsn, a32 * tcs), rb = __builtin_fmaf(a32, tsn, b32 * tcs);
        asm volatile("" : "+v"(ra), "+v"(rb));
        dst[0] = (_Float16)ra;
        dst[half] = (_Float16)rb;
    }
}

// One workgroup per row: amax, then the bytes.  fp32 IEEE division and the hardware's round-to-nearest-even conversion of the clamped
// quotient: the bits of torch's CPU `(W.float() / s).clamp(-448, 448).to(float8_e4m3fn)`.
__global__ __launch_bounds__(256) void k_quantize_rows_e4m3(const _Float16* __restrict__ W, int ldw, int K, uint8_t* __restrict__ q, float* __restrict__ scale) {
    __shared__ float red[4];
    const int t = threadIdx.x;
    const _Float16* row = W + (size_t)blockIdx.x * (size_t)ldw;
    float m = 0.f;
    for (int k = t * 8; k < K; k += 2048) {
        const sc_h8 v = *reinterpret_cast<const sc_h8*>(row + k);
#pragma unroll
        for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)v[e]));
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
    if ((t & 63) == 0) red[t >> 6] = m;
    __syncthreads();
    const float amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float s = amax > 0.f ? __fdiv_rn(amax, 448.f) : 1.f;
    if (t == 0) scale[blockIdx.x] = s;
    for (int k = t * 8; k < K; k += 2048) {
        const sc_h8 v = *reinterpret_cast<const sc_h8*>(row + k);
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = fminf(fmaxf(__fdiv_rn((float)v[e], s), -448.f), 448.f);
        int p0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false), p1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
        p0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], p0, true);
        p1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], p1, true);
        *reinterpret_cast<sc_u2*>(q + (size_t)blockIdx.x * (size_t)K + k) = sc_u2{(unsigned)p0, (unsigned)p1};
    }
}

// Waves per workgroup, per kind of launch as in gemv.hip (0 q/k/v block, 1 short projection, 2 long rows, 3 everything else);
// SC_GEMV_WPB_<kind>=n pins another count.  Unlike gemv.hip the knob only regroups the same waves: the kernel choice and the bits stay.
int pick_wpb_w8(int kind) {
    static int forced[4] = {-1, -1, -1, -1};
    static const int dflt[4] = {4, 4, 7, 4};
    if (forced[kind] < 0) {
        char name[24];
        snprintf(name, sizeof(name), "SC_GEMV_WPB_%d", kind);
        const char* e = getenv(name);
        const int v = e ? atoi(e) : 0;
        forced[kind] = (v >= 1 && v <= 8) ? v : dflt[kind];
    }
    return forced[kind];
}

bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

}  // namespace

extern "C" int sc_quantize_rows_e4m3(const void* W, int ldw, int N, int K, uint8_t* q, float* scale, sc_stream_t stream) {
    SC_REQUIRE(W && q && scale, "sc_quantize_rows_e4m3: null pointer argument");
    SC_REQUIRE(N > 0 && K > 0 && K % 8 == 0 && ldw >= K && ldw % 8 == 0, "sc_quantize_rows_e4m3: K and ldw must be positive multiples of 8, ldw >= K");
    SC_REQUIRE(aligned16(W) && (reinterpret_cast<uintptr_t>(q) & 7) == 0, "sc_quantize_rows_e4m3: W must be 16-byte aligned, q 8-byte aligned");
    hipLaunchKernelGGL(k_quantize_rows_e4m3, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const _Float16*)W, ldw, K, q, scale);
    SC_CHECK_LAUNCH("sc_quantize_rows_e4m3");
    return SC_OK;
}

extern "C" int sc_gemv_w8_f16(const uint8_t* W, const float* scale, const void* x, const void* bias, const void* residual, void* y, int N, int K,
                              int epilogue, int out_f32, const int32_t* y_row, int y_ld, const void* rms_gamma, float rms_eps, sc_stream_t stream) {
    SC_REQUIRE(W && scale && x && y, "sc_gemv_w8_f16: null pointer argument");
    SC_REQUIRE(N > 0 && K > 0 && K % 16 == 0 && K <= 32752, "sc_gemv_w8_f16: K must be a positive multiple of 16, at most 32752");
    SC_REQUIRE(aligned16(W, x, rms_gamma), "sc_gemv_w8_f16: W, x and gamma must be 16-byte aligned");
    SC_REQUIRE(epilogue == SC_EPI_NONE || epilogue == SC_EPI_SWIGLU, "sc_gemv_w8_f16: epilogue must be NONE or SWIGLU");
    SC_REQUIRE(!y_row || (!out_f32 && y_ld > 0), "sc_gemv_w8_f16: a dynamic output row needs fp16 output and y_ld > 0");
    SC_REQUIRE(epilogue != SC_EPI_SWIGLU || (N % 4 == 0 && !bias && !residual && !out_f32), "sc_gemv_w8_f16: SwiGLU needs N % 4 == 0, no bias/residual, fp16 out");
    hipStream_t s = (hipStream_t)stream;
    const _Float16 *xx = (const _Float16*)x, *b = (const _Float16*)bias, *r = (const _Float16*)residual, *gm = (const _Float16*)rms_gamma;
    const size_t lds = (size_t)K * 2 + 16;                           // the staged activation vector + the norm's four wave sums
    // rows per half-wave as gemv.hip picks rows per wave: 4 where there are plenty of rows (x is read once for the four), 1 for the
    // 3584-row projections (enough workgroups in flight); the 7B shapes K = 3584 / 18944 take the straight-line instantiations
    const bool few = N < 16384 && epilogue != SC_EPI_SWIGLU;
    const int rows_per_wave = few ? 2 : 8, wpb = pick_wpb_w8(few ? (K >= 8192 ? 2 : 1) : 3);
    const dim3 grid((unsigned)((N + wpb * rows_per_wave - 1) / (wpb * rows_per_wave))), block(64 * wpb);
#define SC_W8(SW, F32, R, NS, UNR) hipLaunchKernelGGL((k_gemv_w8<SW, F32, R, NS, UNR>), grid, block, lds, s, W, scale, xx, b, r, y, N, K, y_row, y_ld, gm, rms_eps)
#define SC_W8_K(SW, F32, R, UNR7, UNR37)                  \
    do {                                                  \
        if (K == 3584) SC_W8(SW, F32, R, 7, UNR7);        \
        else if (K == 18944) SC_W8(SW, F32, R, 37, UNR37); \
        else SC_W8(SW, F32, R, 0, 1);                     \
    } while (0)
    if (epilogue == SC_EPI_SWIGLU) SC_W8_K(true, false, 4, 2, 2);
    else if (out_f32) { if (few) SC_W8_K(false, true, 1, 7, 12); else SC_W8_K(false, true, 4, 2, 2); }
    else { if (few) SC_W8_K(false, false, 1, 7, 12); else SC_W8_K(false, false, 4, 2, 2); }
#undef SC_W8_K
#undef SC_W8
    SC_CHECK_LAUNCH("sc_gemv_w8_f16");
    return SC_OK;
}

extern "C" int sc_decode_qkv_tab_w8(const uint8_t* Wq, const float* scale_q, const uint8_t* Wkv, const float* scale_kv, const void* bq, const void* bkv,
                                    const void* x, const void* rms_gamma, float rms_eps, void* q_out, void* cache, int cache_ld, const int32_t* pos,
                                    int q_heads, int kv_heads, int Dh, int K, const float* tab_q, const float* tab_k, int tab_rows, sc_stream_t stream) {
    SC_REQUIRE(Wq && scale_q && Wkv && scale_kv && x && q_out && cache && pos && tab_q && tab_k && tab_rows > 0,
               "sc_decode_qkv_tab_w8: null pointer argument / empty rotary table");
    SC_REQUIRE(q_heads > 0 && kv_heads > 0 && Dh > 0 && Dh % 2 == 0 && K > 0 && K % 16 == 0 && K <= 32752, "sc_decode_qkv_tab_w8: bad sizes (K: a multiple of 16, at most 32752)");
    SC_REQUIRE(cache_ld >= 2 * kv_heads * Dh, "sc_decode_qkv_tab_w8: cache row stride too small for K | V");
    SC_REQUIRE(aligned16(Wq, Wkv, x, rms_gamma), "sc_decode_qkv_tab_w8: weights, x and gamma must be 16-byte aligned");
    const int ntask = (q_heads + 2 * kv_heads) * (Dh / 2), wpb = pick_wpb_w8(0);
    const dim3 grid((unsigned)((ntask + wpb - 1) / wpb)), block(64 * wpb);
#define SC_QKV8(NS, UNR)                                                                                                                                     \
    hipLaunchKernelGGL((k_decode_qkv_w8<NS, UNR>), grid, block, (size_t)K * 2 + 16, (hipStream_t)stream, Wq, scale_q, Wkv, scale_kv, (const _Float16*)bq,    \
                       (const _Float16*)bkv, (const _Float16*)x, (const _Float16*)rms_gamma, rms_eps, (_Float16*)q_out, (_Float16*)cache, cache_ld, pos,     \
                       q_heads, kv_heads, Dh, K, tab_q, tab_k, tab_rows)
    if (K == 3584) SC_QKV8(7, 7);
    else SC_QKV8(0, 1);
#undef SC_QKV8
    SC_CHECK_LAUNCH("sc_decode_qkv_tab_w8");
    return SC_OK;
}
