// FP8 (OCP e4m3fn) KV cache for the batch-1 and the batched decode (include/streamchat_hip_kv8.h, streamchat_hip_kv8_batched.h): the row
// quantiser, its inverse, the batched step's rotary + quantised append, and k_attn_decode of attention_decode.hip over e4m3 bytes.  A cache row is [K of all KV heads | V of all KV heads], 128 bytes per head, and every 128-element
// segment has one power-of-two fp32 scale 2^e, e in [-14, 7]: code * 2^e is exact in fp16, so the attention kernel converts each operand to
// exactly the fp16 value k_attn_decode reads from the dequantised cache and feeds it to the same functions (attention_decode_common.h: the
// softmax step, the P.V MFMAs, the merge) in the same order - its results are bit-identical to that kernel's, the loop just streams half the
// bytes.  Default machine scheduler, as attention_decode.hip.
#include "attention_decode_common.h"
#include "../../include/streamchat_hip_kv8_batched.h"

// attention_decode.hip: the split-KV merge, reused unchanged
void sc_attn_combine_launch(int Dh, const float* part, void* out, int ldo, int B, int Sq, int Hq, int nsplit, int o_hs, long o_bs, hipStream_t s);

namespace {

// 8 e4m3 bytes -> 8 fp16 values code * s (s = a power of two as a packed fp16 pair: the product is exact, see the header)
__device__ __forceinline__ sc_h8 cvt8(const sc_u2 w, const sc_h2 s) {
    const sc_h2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[0], 1.0f, false) * s, b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[0], 1.0f, true) * s;
    const sc_h2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[1], 1.0f, false) * s, d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[1], 1.0f, true) * s;
    return sc_h8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// ------------------------------------------------------------------------------------------------------------------
// Quantiser and its inverse: 16 lanes per 128-element segment, 8 elements per lane (one 16-byte load, one 8-byte store).
// ------------------------------------------------------------------------------------------------------------------
// The specification of the header for ONE segment held by 16 consecutive lanes, 8 fp16 values each: the segment's exponent e (every lane gets it)
// and this lane's 8 codes.  The one text of k_kv8_quantize and k_kv8_rope_qkv_rows.
struct Kv8Seg { sc_u2 codes; int e; };
__device__ __forceinline__ Kv8Seg kv8_quantize_seg(const sc_h8 v) {
    float m = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) m = fmaxf(m, fabsf((float)v[e]));
#pragma unroll
    for (int sh = 8; sh >= 1; sh >>= 1) m = fmaxf(m, __shfl_xor(m, sh, 64));
    // frexp(amax / 448) = (mant, e): amax / 448 is a normal fp32 for every non-zero fp16 amax, mant == 0.5 is a zero fraction field
    const unsigned qb = __float_as_uint(__fdiv_rn(m, 448.f));
    int e = (int)(qb >> 23) - 126 - ((qb & 0x7fffffu) == 0 ? 1 : 0);
    e = m > 0.f ? min(max(e, -14), 7) : 0;
    const float inv = __uint_as_float((unsigned)(127 - e) << 23);
    float f[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f[k] = fminf(fmaxf((float)v[k] * inv, -448.f), 448.f);      // x / 2^e is exact
    int p0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], 0, false), p1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], 0, false);
    p0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], p0, true);
    p1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], p1, true);
    return {sc_u2{(unsigned)p0, (unsigned)p1}, e};
}
__device__ __forceinline__ float kv8_scale(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }

__global__ __launch_bounds__(256) void k_kv8_quantize(const _Float16* __restrict__ x, int ld, int n, int nseg, uint8_t* __restrict__ cache, int cache_ld,
                                                      float* __restrict__ scales, int cache_rows, int row0, const int* __restrict__ row0_dev, int x_follows) {
    const int gid = blockIdx.x * 256 + threadIdx.x, seg = gid >> 4, l = gid & 15;
    const int r0 = row0_dev ? row0_dev[0] : row0;
    const int sg = seg < n * nseg ? seg : 0;                  // (lanes past the last segment redo segment 0 and store nothing)
    const int i = sg / nseg, s = sg - i * nseg, row = r0 + i;
    const bool live = seg < n * nseg && row >= 0 && row < cache_rows;
    const int xr = x_follows ? (live ? row : 0) : i;
    const Kv8Seg q = kv8_quantize_seg(*reinterpret_cast<const sc_h8*>(x + (size_t)xr * (size_t)ld + s * 128 + l * 8));
    if (live) {
        *reinterpret_cast<sc_u2*>(cache + (size_t)row * (size_t)cache_ld + s * 128 + l * 8) = q.codes;
        if (l == 0) scales[(size_t)row * (size_t)nseg + s] = kv8_scale(q.e);
    }
}

// sc_kv8_rope_qkv_rows: k_rope_qkv_rows (llm_ops.hip) with the K | V row quantised on the way out.  One 16-lane group per head of the fused
// q | k | v row of one sequence (Hq + 2 Hkv heads of Dh = 128 fp32 sums), 8 elements per lane.  A rotary pair (j, j + 64) lies inside one head:
// lanes l and l + 8 load the same a = x[j0 ..], b = x[64 + j0 ..], cos and sin (j0 = (l & 7) * 8); lane l < 8 keeps the first half's
// fma(-b, sin, a * cos), lane l + 8 the second half's fma(a, sin, b * cos) - k_rope_qkv_rows' fma sequence and ITS rounding to fp16.  q heads are
// stored as they are; K and V (a cast) heads go through kv8_quantize_seg in registers: the second rounding, of the fp16 value.  So bytes and scales
// equal sc_rope_qkv_rows_f16 into an fp16 row followed by sc_kv8_quantize_rows of that row, and no fp16 K | V row exists in memory.
__global__ __launch_bounds__(256) void k_kv8_rope_qkv_rows(const float* __restrict__ x, int ldx, const float* __restrict__ tab_q, const float* __restrict__ tab_k,
                                                           int tab_rows, const int* __restrict__ pos, int B, int Hq, int Hkv, _Float16* __restrict__ q_out, int ldq,
                                                           uint8_t* __restrict__ cache, long cache_bs, int cache_ld, float* __restrict__ scales, int cache_rows) {
    constexpr int DH = 128, HALF = 64;
    const int heads = Hq + 2 * Hkv;
    const int gid = blockIdx.x * 256 + threadIdx.x, unit = gid >> 4, l = gid & 15;
    const bool live = unit < B * heads;
    const int u = live ? unit : 0;                            // (groups past the last head redo head 0 and store nothing: the shuffles need every lane)
    const int b = u / heads, h = u - b * heads;
    const float* xr = x + (size_t)b * (size_t)ldx + h * DH;
    int p = pos[b];
    const int prow = p < 0 ? 0 : (p >= cache_rows ? cache_rows - 1 : p);           // device-side positions are clamped (cache row and table row), as k_rope_qkv_rows
    p = p < 0 ? 0 : (p >= tab_rows ? tab_rows - 1 : p);
    sc_h8 o;
    if (h < Hq + Hkv) {
        const int j0 = (l & 7) * 8;
        const float* t = (h < Hq ? tab_q : tab_k) + (size_t)p * DH;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const sc_f4 a = *reinterpret_cast<const sc_f4*>(xr + j0 + w * 4), bb = *reinterpret_cast<const sc_f4*>(xr + HALF + j0 + w * 4);
            const sc_f4 cs = *reinterpret_cast<const sc_f4*>(t + j0 + w * 4), sn = *reinterpret_cast<const sc_f4*>(t + HALF + j0 + w * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float ra = __builtin_fmaf(-bb[e], sn[e], a[e] * cs[e]), rb = __builtin_fmaf(a[e], sn[e], bb[e] * cs[e]);
                asm volatile("" : "+v"(ra), "+v"(rb));                  // fp32 fma, THEN the fp16 rounding (see k_rope_f32in)
                o[w * 4 + e] = (_Float16)(l < 8 ? ra : rb);
            }
        }
    } else {
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const sc_f4 v = *reinterpret_cast<const sc_f4*>(xr + l * 8 + w * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) o[w * 4 + e] = (_Float16)v[e];
        }
    }
    const Kv8Seg q = kv8_quantize_seg(o);                     // (every lane: q heads take part in the shuffles and drop the result)
    if (!live) return;
    if (h < Hq) {
        _Float16* qo = q_out + (size_t)b * (size_t)ldq + h * DH + l * 8;
        *reinterpret_cast<sc_h4*>(qo) = sc_h4{o[0], o[1], o[2], o[3]};
        *reinterpret_cast<sc_h4*>(qo + 4) = sc_h4{o[4], o[5], o[6], o[7]};
        return;
    }
    const int s = h - Hq;
    *reinterpret_cast<sc_u2*>(cache + (size_t)b * (size_t)cache_bs + (size_t)prow * (size_t)cache_ld + s * DH + l * 8) = q.codes;
    if (l == 0) scales[((size_t)b * (size_t)cache_rows + (size_t)prow) * (size_t)(2 * Hkv) + s] = kv8_scale(q.e);
}

__global__ __launch_bounds__(256) void k_kv8_dequantize(const uint8_t* __restrict__ cache, int cache_ld, const float* __restrict__ scales, int row0, int n, int nseg,
                                                        _Float16* __restrict__ out, int ld) {
    const int gid = blockIdx.x * 256 + threadIdx.x, seg = gid >> 4, l = gid & 15;
    if (seg >= n * nseg) return;
    const int i = seg / nseg, s = seg - i * nseg;
    const sc_u2 w = *reinterpret_cast<const sc_u2*>(cache + (size_t)(row0 + i) * (size_t)cache_ld + s * 128 + l * 8);
    const _Float16 sh = (_Float16)scales[(size_t)(row0 + i) * (size_t)nseg + s];
    *reinterpret_cast<sc_h8*>(out + (size_t)i * (size_t)ld + s * 128 + l * 8) = cvt8(w, sc_h2{sh, sh});
}

// ------------------------------------------------------------------------------------------------------------------
// k_attn_decode (attention_decode.hip: one LDS-DMA ring per wave, hand-counted vmcnt) with e4m3 operands; the 32-row chunks, their even
// partition over splits and waves, the softmax step, P.V and the end-of-block merge are attention_decode_common.h's.  Per wave and ring stage:
//   K bytes  4 KiB: rows of 128 B row-major, the 16-byte slot XORed with (row >> 1) & 7 on the SOURCE side, so the 8-byte A-fragment reads
//            (ds_read_b64: bytes ds * 32 + g * 8 .. + 7 of row kvb * 16 + rl, the elements k_attn_decode's lane holds) of a half-wave
//            cover 256 distinct bytes modulo the bank period;
//   V bytes  4 KiB: rows of 128 B, unswizzled: pass i of the conversion reads 8 bytes per lane at i * 512 + lane * 8 (row i * 4 + lane / 16,
//            piece lane % 16: ONE row, one scale per read);
//   scales   256 B: ONE 4-byte DMA per chunk, lanes 0-31 the K scales of rows 0-31, lanes 32-63 the V scales in the order a lane reads
//            them (slot w * 8 + i = row i * 4 + w);  it rides in front of the K bytes, so a chunk's scales are there with its K.
// The converted V chunk (fp16(code * scale), 8 KiB, ONE per wave) is written in exactly k_attn_decode's V ring layout and read with the same
// ds_read_b64_tr_b16 reads (dec_read_vt); same-wave LDS write -> read needs an lgkmcnt wait and no barrier.  16.25 KiB per wave at DEC8_PD = 1.
// Rows past the wave's range are outside the extent of ALL THREE buffer resources (bytes and scales): zeros, whatever memory holds there
// (0 * 0 = 0 in the MFMA; a NaN scale or a NaN byte behind kv_len is never read).
// vm queue of a wave:  [q x 4]  K(c0) V(c0) ..  then per chunk  K(c + PD)  V(c + PD);  K(c) = 1 scale op + 4 byte ops, V(c) = 4 ops.
// ------------------------------------------------------------------------------------------------------------------
constexpr int DEC8_PD = 1;                                                       // ring stages (2 measured: profiles/r11_decode_kv8_ab.md)
constexpr int KB8 = DCH * 128, SCB = 256, VST = DCH * 256;                       // K or V bytes of a chunk, its scales, the fp16 V stage
constexpr int WAVE_LDS8 = DEC8_PD * (2 * KB8 + SCB) + VST;

__global__ __launch_bounds__(64 * DEC_NW) void k_attn_kv8(const _Float16* __restrict__ Q, int ldq, const uint8_t* __restrict__ cache, int ldc,
                                                           const float* __restrict__ scales, int Sq, int Skv, int Hkv, float scale_log2,
                                                           const int* __restrict__ kv_len, float* __restrict__ part, int nsplit, int q_hs, long q_bs,
                                                           long cache_bs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int DH = 128, DS = 4, DB = 8, VROW = DEC_VROW;
    constexpr int CNT_K = 9 * DEC8_PD - 5, CNT_V = 9 * DEC8_PD - 4;                 // vm ops younger than K(c) / than V(c) at their waits
    static_assert(DEC8_PD >= 1 && CNT_V < 64, "vmcnt is a 6-bit counter");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rl = lane & 15, g = lane >> 4;
    const int split = blockIdx.x, h = blockIdx.y, b = blockIdx.z;                       // grid = (split, KV head, sequence), as k_attn_decode
    const int kv_valid = kv_len ? min(max(kv_len[b], 0), Skv) : Skv;
    const DecRange wr = dec_range<DEC_NW_LOG>(kv_valid, nsplit, split, wave);
    const int c_lo = wr.c_lo, c_hi = wr.c_hi, row_end = wr.row_end;                     // (plain ints: the issue lambdas capture them)
    sc_u4 qf[DS];
    dec_load_q(Q + (size_t)b * (size_t)q_bs + h * q_hs, ldq, Sq, rl, g, qf);
    const int nseg = 2 * Hkv;
    // sequence b's slice goes into the 64-bit BASE of the three buffer resources; offsets and extents below stay 32-bit and per sequence, so the
    // rows behind kv_len[b], the row pad and the next sequence's rows are all outside a wave's extent
    const uint8_t* kbase = cache + (size_t)b * (size_t)cache_bs + h * DH;
    const uint8_t* vbase = kbase + Hkv * DH;
    const float* sbase = scales + (size_t)b * (size_t)Skv * (size_t)nseg + h;
    const bool any = c_lo < c_hi && row_end > 0;
    const int b_ext = any ? (int)((unsigned)(row_end - 1) * (unsigned)ldc + DH) : 0;                       // K and V bytes (from kbase / vbase)
    const int s_ext = any ? (int)(((unsigned)(row_end - 1) * (unsigned)nseg + (unsigned)Hkv + 1u) * 4u) : 0;   // scales (from sbase)
    // per-lane source offsets inside a chunk.  16-byte granule j * 64 + lane lands at LDS byte (j * 64 + lane) * 16 = row j * 8 + (lane >> 3), slot lane & 7
    unsigned k_vo[4], v_vo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = j * 8 + (lane >> 3);
        k_vo[j] = (unsigned)r * (unsigned)ldc + (unsigned)((((lane & 7) ^ ((r >> 1) & 7))) * 16);
        v_vo[j] = (unsigned)r * (unsigned)ldc + (unsigned)((lane & 7) * 16);
    }
    const int sp = lane & 31, srow = lane < 32 ? sp : (sp & 7) * 4 + (sp >> 3);
    const unsigned s_vo = ((unsigned)srow * (unsigned)nseg + (lane < 32 ? 0u : (unsigned)Hkv)) * 4u;
    char* wbase = smem + wave * WAVE_LDS8;
    char* kring = wbase;
    char* vring = wbase + DEC8_PD * KB8;
    char* sring = wbase + DEC8_PD * 2 * KB8;
    const unsigned lds0 = (unsigned)(size_t)((__attribute__((address_space(3))) char*)smem) + (unsigned)(wave * WAVE_LDS8);
    const unsigned k_lds = lds0, v_lds = lds0 + DEC8_PD * KB8, s_lds = lds0 + DEC8_PD * 2 * KB8, st_lds = lds0 + DEC8_PD * (2 * KB8 + SCB);
    unsigned k_off[DS];
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) k_off[ds] = (unsigned)(rl * 128 + (((ds * 2 + (g >> 1)) ^ ((rl >> 1) & 7)) << 4) + (g & 1) * 8);
    // conversion pass i: row i * 4 + g, piece rl -> k_attn_decode's V ring slot piece ^ ((row & 7) << 1)
    unsigned w_off[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { const int r = i * 4 + g; w_off[i] = (unsigned)(r * VROW + ((rl ^ ((r & 7) << 1)) << 4)); }
    unsigned v_off[DB];
    dec_v_offsets(rl, g, v_off);

    auto issue_k = [&](int c) {                                  // 1 + 4 LDS-DMA ops
        const int st = c % DEC8_PD;
        const bool in = c < c_hi;
        lds_load4(sbase, in ? s_ext : 0, sring + st * SCB, (unsigned)c * (unsigned)(DCH * nseg * 4) + s_vo);
        const unsigned ro = (unsigned)c * (unsigned)(DCH * ldc);
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_load16(kbase, in ? b_ext : 0, kring + st * KB8 + j * 1024, ro + k_vo[j]);
    };
    auto issue_v = [&](int c) {                                  // 4 LDS-DMA ops
        const unsigned ro = (unsigned)c * (unsigned)(DCH * ldc);
#pragma unroll
        for (int j = 0; j < 4; ++j) lds_load16(vbase, c < c_hi ? b_ext : 0, vring + (c % DEC8_PD) * KB8 + j * 1024, ro + v_vo[j]);
    };

    sc_f4 o[DB];
#pragma unroll
    for (int i = 0; i < DB; ++i) o[i] = sc_f4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    if (any) {
#pragma unroll
        for (int u = 0; u < DEC8_PD; ++u) { issue_k(c_lo + u); issue_v(c_lo + u); }          // (past c_hi: zero extent -> no traffic)
        for (int c = c_lo; c < c_hi; ++c) {
            const unsigned st = (unsigned)(c % DEC8_PD);
            // ---- S^T = K . Q^T for the 32 rows: K bytes, the chunk's scales ----
            asm volatile("s_waitcnt vmcnt(%4)" : "+v"(qf[0]), "+v"(qf[1]), "+v"(qf[2]), "+v"(qf[3]) : "n"(CNT_K) : "memory");
            sc_u2 kb[2][DS];
            float ksc[2];
            sc_f4 vsa, vsb;
            const unsigned ka = k_lds + st * KB8, sa_ = s_lds + st * SCB;
#pragma unroll
            for (int ds = 0; ds < DS; ++ds) {
                asm volatile("ds_read_b64 %0, %1" : "=v"(kb[0][ds]) : "v"(ka + k_off[ds]));
                asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(kb[1][ds]) : "v"(ka + k_off[ds]), "n"(16 * 128));
            }
            asm volatile("ds_read_b32 %0, %1" : "=v"(ksc[0]) : "v"(sa_ + rl * 4));
            asm volatile("ds_read_b32 %0, %1 offset:64" : "=v"(ksc[1]) : "v"(sa_ + rl * 4));
            asm volatile("ds_read_b128 %0, %1 offset:128" : "=v"(vsa) : "v"(sa_ + g * 32));
            asm volatile("ds_read_b128 %0, %1 offset:144" : "=v"(vsb) : "v"(sa_ + g * 32));
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kb[0][0]), "+v"(kb[0][1]), "+v"(kb[0][2]), "+v"(kb[0][3]), "+v"(kb[1][0]), "+v"(kb[1][1]), "+v"(kb[1][2]),
                                                  "+v"(kb[1][3]), "+v"(ksc[0]), "+v"(ksc[1]), "+v"(vsa), "+v"(vsb) :: "memory");
            issue_k(c + DEC8_PD);                                  // K(c)'s stage and its scales are free: they are in registers
            sc_f4 s[2];
#pragma unroll
            for (int kvb = 0; kvb < 2; ++kvb) {
                const _Float16 kh = (_Float16)ksc[kvb];
                const sc_h2 ks = {kh, kh};
                s[kvb] = sc_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ds = 0; ds < DS; ++ds)
                    s[kvb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cvt8(kb[kvb][ds], ks), __builtin_bit_cast(sc_h8, qf[ds]), s[kvb], 0, 0, 0);
            }
            const sc_h8 pf = dec_softmax_step(s, c * DCH + g * 4, row_end, scale_log2, m_run, l_run, o);
            // ---- V(c) must have landed: bytes -> fp16(code * scale) -> the fp16 stage ----
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CNT_V) : "memory");
            sc_u2 vb[8];
            const unsigned va = v_lds + st * KB8 + (unsigned)lane * 8u;
#pragma unroll
            for (int i = 0; i < 8; ++i) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(vb[i]) : "v"(va), "n"(i * 512));
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vb[0]), "+v"(vb[1]), "+v"(vb[2]), "+v"(vb[3]), "+v"(vb[4]), "+v"(vb[5]), "+v"(vb[6]), "+v"(vb[7]) :: "memory");
            issue_v(c + DEC8_PD);                                  // V(c)'s byte stage is free
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const _Float16 vh = (_Float16)(i < 4 ? vsa[i & 3] : vsb[i & 3]);
                const sc_u4 hv = __builtin_bit_cast(sc_u4, cvt8(vb[i], sc_h2{vh, vh}));
                asm volatile("ds_write_b128 %0, %1" ::"v"(st_lds + w_off[i]), "v"(hv) : "memory");
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // ---- O^T += V^T . P^T ----
            sc_s4 lo[DB], hi[DB];
            dec_read_vt(st_lds, v_off, lo, hi);
            dec_pv(lo, hi, pf, o);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // no LDS-DMA may still be in flight when the merge reuses the rings / the block ends
    dec_merge_waves<DEC_NW, DH>(smem, o, m_run, l_run, tid, wave, rl, g, Sq, part + ((((size_t)b * Hkv + h) * Sq) * nsplit + split) * (DH + 2), nsplit);
}

}  // namespace

#define SC_KV8_DH(name)                                                                                                    \
    do {                                                                                                                   \
        if (Dh != 128) return sc_fail(SC_ERR_UNSUPPORTED, name ": head dim %d unsupported (the fp8 KV cache serves 128 only)", Dh); \
    } while (0)

extern "C" int sc_kv8_quantize_rows(const void* x, int ld, int n, int kv_heads, int Dh, uint8_t* cache, int cache_ld, float* scales, int cache_rows,
                                    int row0, const int32_t* row0_dev, int x_follows_row, sc_stream_t stream) {
    SC_REQUIRE(x && cache && scales, "sc_kv8_quantize_rows: null pointer argument");
    SC_KV8_DH("sc_kv8_quantize_rows");
    SC_REQUIRE(n > 0 && kv_heads > 0 && kv_heads <= 4096 && cache_rows > 0 && n <= cache_rows, "sc_kv8_quantize_rows: bad sizes (n, kv_heads, cache_rows positive, n <= cache_rows)");
    const int w = 2 * kv_heads * Dh;
    SC_REQUIRE(ld >= w && ld % 8 == 0 && cache_ld >= w && cache_ld % 8 == 0, "sc_kv8_quantize_rows: row strides must be multiples of 8, at least 2 * kv_heads * Dh");
    SC_REQUIRE((reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(cache) & 7) == 0, "sc_kv8_quantize_rows: x must be 16-byte aligned, cache 8-byte aligned");
    SC_REQUIRE(row0_dev || (row0 >= 0 && row0 + n <= cache_rows), "sc_kv8_quantize_rows: rows row0 .. row0 + n - 1 exceed the cache");
    const long segs = (long)n * 2 * kv_heads;
    SC_REQUIRE(segs <= (1L << 27), "sc_kv8_quantize_rows: too many segments for one launch");
    hipLaunchKernelGGL(k_kv8_quantize, dim3((unsigned)((segs + 15) / 16)), dim3(256), 0, (hipStream_t)stream, (const _Float16*)x, ld, n, 2 * kv_heads, cache, cache_ld,
                       scales, cache_rows, row0, row0_dev, x_follows_row);
    SC_CHECK_LAUNCH("sc_kv8_quantize_rows");
    return SC_OK;
}

extern "C" int sc_kv8_dequantize_rows(const uint8_t* cache, int cache_ld, const float* scales, int cache_rows, int row0, int n, int kv_heads, int Dh,
                                      void* out, int ld, sc_stream_t stream) {
    SC_REQUIRE(cache && scales && out, "sc_kv8_dequantize_rows: null pointer argument");
    SC_KV8_DH("sc_kv8_dequantize_rows");
    SC_REQUIRE(n > 0 && kv_heads > 0 && kv_heads <= 4096 && cache_rows > 0, "sc_kv8_dequantize_rows: bad sizes (n, kv_heads, cache_rows positive)");
    const int w = 2 * kv_heads * Dh;
    SC_REQUIRE(ld >= w && ld % 8 == 0 && cache_ld >= w && cache_ld % 8 == 0, "sc_kv8_dequantize_rows: row strides must be multiples of 8, at least 2 * kv_heads * Dh");
    SC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(cache) & 7) == 0, "sc_kv8_dequantize_rows: out must be 16-byte aligned, cache 8-byte aligned");
    SC_REQUIRE(row0 >= 0 && n <= cache_rows && row0 <= cache_rows - n, "sc_kv8_dequantize_rows: rows row0 .. row0 + n - 1 exceed the cache");
    const long segs = (long)n * 2 * kv_heads;
    SC_REQUIRE(segs <= (1L << 27), "sc_kv8_dequantize_rows: too many segments for one launch");
    hipLaunchKernelGGL(k_kv8_dequantize, dim3((unsigned)((segs + 15) / 16)), dim3(256), 0, (hipStream_t)stream, cache, cache_ld, scales, row0, n, 2 * kv_heads,
                       (_Float16*)out, ld);
    SC_CHECK_LAUNCH("sc_kv8_dequantize_rows");
    return SC_OK;
}

// the one launcher of k_attn_kv8 + the split-KV merge: sc_attention_kv8 is its B = 1 call
static int kv8_attention(const char* name, const void* q, int ldq, const uint8_t* cache, int cache_ld, int64_t cache_bs, const float* scales, void* out, int ldo,
                         int B, int Sq, int Skv, int kv_heads, int Dh, float scale, int flags, const int32_t* kv_len, int nsplit, void* ws, size_t ws_bytes,
                         int q_head_stride, int o_head_stride, int64_t q_batch_stride, int64_t o_batch_stride, sc_stream_t stream) {
    if (!(q && cache && scales && out)) return sc_fail(SC_ERR_ARG, "%s: null pointer argument", name);
    if (Dh != 128) return sc_fail(SC_ERR_UNSUPPORTED, "%s: head dim %d unsupported (the fp8 KV cache serves 128 only)", name, Dh);
    if ((flags & ~SC_ATTN_Q_PRESCALED) != 0) return sc_fail(SC_ERR_ARG, "%s: flags must be 0 or SC_ATTN_Q_PRESCALED (the kernel is non-causal)", name);
    if (!(B > 0 && B <= 65535 && Sq > 0 && Sq <= 16 && Skv > 0 && kv_heads > 0 && kv_heads <= 65535))
        return sc_fail(SC_ERR_ARG, "%s: bad sizes (1 <= Sq <= 16 query rows per KV head, at most 65535 sequences and KV heads)", name);
    if (!(cache_ld >= 2 * kv_heads * Dh && cache_ld % 16 == 0 && (long)Skv * cache_ld < (1L << 31)))
        return sc_fail(SC_ERR_ARG, "%s: cache row stride must be a multiple of 16, at least 2 * kv_heads * Dh, one sequence's cache below 2 GiB", name);
    if (B > 1 && !(cache_bs % 16 == 0 && cache_bs >= (int64_t)Skv * cache_ld))
        return sc_fail(SC_ERR_ARG, "%s: cache batch stride (bytes) must be a multiple of 16, at least Skv * cache_ld", name);
    if (!(ldq % 8 == 0 && ldo % 4 == 0)) return sc_fail(SC_ERR_ARG, "%s: leading dims must be multiples of 8 (out: 4)", name);
    if (!(((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(cache)) & 15) == 0 && (reinterpret_cast<uintptr_t>(scales) & 3) == 0 &&
          (reinterpret_cast<uintptr_t>(out) & 7) == 0))
        return sc_fail(SC_ERR_ARG, "%s: q and cache must be 16-byte aligned, out 8-byte", name);
    if (!(nsplit >= 1 && nsplit <= 1024)) return sc_fail(SC_ERR_ARG, "%s: nsplit must be in [1, 1024]", name);
    const size_t need = (size_t)B * kv_heads * Sq * nsplit * (Dh + 2) * sizeof(float);
    if (!ws || ws_bytes < need) return sc_fail(SC_ERR_WORKSPACE, "%s: split-KV workspace %zu < required %zu", name, ws_bytes, need);
    const int qhs = q_head_stride > 0 ? q_head_stride : Dh, ohs = o_head_stride > 0 ? o_head_stride : Dh;
    const long qbs = q_batch_stride > 0 ? (long)q_batch_stride : (long)Sq * ldq, obs = o_batch_stride > 0 ? (long)o_batch_stride : (long)Sq * ldo;
    if (!(qhs % 8 == 0 && ohs % 4 == 0 && qbs % 8 == 0 && obs % 4 == 0))
        return sc_fail(SC_ERR_ARG, "%s: head and batch strides must be multiples of 8 (q) / 4 (out)", name);
    hipStream_t s = (hipStream_t)stream;
    const float sl2 = (flags & SC_ATTN_Q_PRESCALED) ? 1.0f : scale * 1.4426950408889634f;
    constexpr int LDS = dec_lds_bytes(DEC_NW * WAVE_LDS8);
    sc_set_max_lds<k_attn_kv8>(LDS);
    hipLaunchKernelGGL(k_attn_kv8, dim3((unsigned)nsplit, (unsigned)kv_heads, (unsigned)B), dim3(64 * DEC_NW), LDS, s, (const _Float16*)q, ldq, cache, cache_ld, scales,
                       Sq, Skv, kv_heads, sl2, kv_len, (float*)ws, nsplit, qhs, qbs, (long)(B > 1 ? cache_bs : 0));
    sc_attn_combine_launch(128, (const float*)ws, out, ldo, B, Sq, kv_heads, nsplit, ohs, obs, s);
    SC_CHECK_LAUNCH(name);
    return SC_OK;
}

extern "C" int sc_attention_kv8(const void* q, int ldq, const uint8_t* cache, int cache_ld, const float* scales, void* out, int ldo, int Sq, int Skv,
                                int kv_heads, int Dh, float scale, int flags, const int32_t* kv_len, int nsplit, void* ws, size_t ws_bytes,
                                int q_head_stride, int o_head_stride, sc_stream_t stream) {
    return kv8_attention("sc_attention_kv8", q, ldq, cache, cache_ld, 0, scales, out, ldo, 1, Sq, Skv, kv_heads, Dh, scale, flags, kv_len, nsplit, ws, ws_bytes,
                         q_head_stride, o_head_stride, 0, 0, stream);
}

extern "C" int sc_attention_kv8_batched(const void* q, int ldq, const uint8_t* cache, int cache_ld, int64_t cache_batch_stride, const float* scales, void* out,
                                        int ldo, int B, int Sq, int Skv, int kv_heads, int Dh, float scale, int flags, const int32_t* kv_len, int nsplit, void* ws,
                                        size_t ws_bytes, int q_head_stride, int o_head_stride, int64_t q_batch_stride, int64_t o_batch_stride, sc_stream_t stream) {
    return kv8_attention("sc_attention_kv8_batched", q, ldq, cache, cache_ld, cache_batch_stride, scales, out, ldo, B, Sq, Skv, kv_heads, Dh, scale, flags, kv_len,
                         nsplit, ws, ws_bytes, q_head_stride, o_head_stride, q_batch_stride, o_batch_stride, stream);
}

extern "C" int sc_kv8_rope_qkv_rows(const float* x, int ldx, const float* tab_q, const float* tab_k, int tab_rows, const int32_t* positions, int B, int q_heads,
                                    int kv_heads, int Dh, void* q_out, int ldq, uint8_t* cache, int64_t cache_batch_stride, int cache_ld, float* scales,
                                    int cache_rows, sc_stream_t stream) {
    SC_REQUIRE(x && tab_q && tab_k && positions && q_out && cache && scales, "sc_kv8_rope_qkv_rows: null pointer argument");
    SC_KV8_DH("sc_kv8_rope_qkv_rows");
    SC_REQUIRE(B > 0 && q_heads > 0 && kv_heads > 0 && tab_rows > 0 && cache_rows > 0, "sc_kv8_rope_qkv_rows: bad sizes");
    SC_REQUIRE(ldx >= (q_heads + 2 * kv_heads) * Dh && ldx % 4 == 0 && ldq >= q_heads * Dh && ldq % 4 == 0 && cache_ld >= 2 * kv_heads * Dh && cache_ld % 8 == 0 &&
               cache_batch_stride % 8 == 0 && (B == 1 || cache_batch_stride >= (int64_t)cache_rows * cache_ld),
               "sc_kv8_rope_qkv_rows: leading dimensions too small or not multiples of 4 (x, q_out) / 8 (cache row and batch stride, in bytes)");
    SC_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(tab_q) | reinterpret_cast<uintptr_t>(tab_k)) & 15) == 0 &&
               ((reinterpret_cast<uintptr_t>(q_out) | reinterpret_cast<uintptr_t>(cache)) & 7) == 0 && (reinterpret_cast<uintptr_t>(scales) & 3) == 0,
               "sc_kv8_rope_qkv_rows: x / tables must be 16-byte aligned, q_out and cache 8-byte, scales 4-byte");
    const long lanes = (long)B * (q_heads + 2 * kv_heads) * 16;
    SC_REQUIRE(lanes <= (1L << 30), "sc_kv8_rope_qkv_rows: too many heads for one launch");
    hipLaunchKernelGGL(k_kv8_rope_qkv_rows, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, tab_q, tab_k, tab_rows, positions, B,
                       q_heads, kv_heads, (_Float16*)q_out, ldq, cache, (long)cache_batch_stride, cache_ld, scales, cache_rows);
    SC_CHECK_LAUNCH("sc_kv8_rope_qkv_rows");
    return SC_OK;
}
