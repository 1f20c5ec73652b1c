// What the two streaming decode attention kernels share: k_attn_decode (attention_decode.hip, fp16 K/V) and k_attn_kv8 (attention_kv8.hip, e4m3
// K/V).  k_attn_kv8's contract is to equal k_attn_decode on the dequantised cache BIT FOR BIT (tests/test_gpu_kv8.py), so everything that decides
// a result bit apart from the operand fetch has its one text here: which chunks a wave takes, the Q fragments, the online-softmax step, the
// transposed V reads and the P.V MFMAs, the merge of a workgroup's waves and the partial it leaves for k_attn_combine.  Each kernel keeps what
// differs: its ring layout and swizzles, issue_k / issue_v, its vmcnt constants, the K-fragment reads and (fp8) the V conversion stage.
// tests/golden/decode_attention_bits.npz pins the bits these functions produce (both kernels call them, so their comparison cannot).
#pragma once
#include "sc_common.h"

typedef short sc_s4 __attribute__((ext_vector_type(4)));

constexpr int DCH = 32;                            // kv rows per chunk
// streaming waves per workgroup.  Measured 2 / 4 / 8 in profiles/r05_run_t_decode_attention_waves_per_workgroup.md
constexpr int DEC_NW = 4, DEC_NW_LOG = 2;
static_assert((1 << DEC_NW_LOG) == DEC_NW, "dec_range shifts by the logarithm");
constexpr int DEC_VROW = 256;                      // bytes of one fp16 V row in LDS (Dh = 128)

// dynamic LDS of a launch: the waves' rings, or dec_merge_waves' [NW][128][16] O^T + [NW][16] m + [NW][16] l where that is larger
constexpr int dec_lds_bytes(int ring_bytes) {
    constexpr int merge = DEC_NW * (128 * 16 + 32) * 4;
    return ring_bytes > merge ? ring_bytes : merge;
}

// LDS-DMA through a raw buffer resource (base, extent in bytes): lane address = base + voff + soff, every lane's 16 (4) bytes land lane-linear
// behind the wave-uniform `lds`; a lane at or past `extent` writes zeros and causes no memory traffic.  Free functions because an opaque
// __amdgpu_buffer_rsrc_t inside a lambda of the kernel silently drops the kernel's host stub.  (attention.hip's tile kernel uses lds_load16 too.)
__device__ __forceinline__ void lds_load16(const void* base, int extent, char* lds, unsigned voff, int soff = 0) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, extent, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds, 16, voff, soff, 0, 0);
}
__device__ __forceinline__ void lds_load4(const void* base, int extent, char* lds, unsigned voff) {
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, extent, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)lds, 4, voff, 0, 0, 0);
}

// The chunks [c_lo, c_hi) and rows [c_lo * 32, row_end) of one wave: the 32-row chunks of the valid keys go to the splits, a split's to its
// 2^NW_LOG waves, in EVEN shares (sizes differ by at most one chunk; a share may be empty).  Round 4 cut ceil(nch / nsplit) chunks per split and
// ceil(that / 4) per wave: at 49 153 keys (1537 chunks, 64 splits) that is 25 chunks for 61 workgroups, 12 for one and none for two, and
// 7 | 7 | 7 | 4 inside a workgroup - the launch lasted 7 chunk times where 6.004 would do.
struct DecRange { int c_lo, c_hi, row_end; };
template <int NW_LOG>
__device__ __forceinline__ DecRange dec_range(int kv_valid, int nsplit, int split, int wave) {
    const int nch = (kv_valid + DCH - 1) / DCH;
    const int cq = nch / nsplit, cr = nch - cq * nsplit;                                // the first cr splits take cq + 1 chunks
    const int s_lo = split * cq + min(split, cr), ns = cq + (split < cr ? 1 : 0);
    const int c_lo = s_lo + ((ns * wave) >> NW_LOG), c_hi = s_lo + ((ns * (wave + 1)) >> NW_LOG);
    return {c_lo, c_hi, min(c_hi * DCH, kv_valid)};
}

// Q fragments of lane (rl, g) from `qh`, the first query row of this head (B operand: column = query row rl, k-slots = 8 head-dim elements;
// rows past Sq repeat the last one).  Inline asm, so that no compiler-tracked vector load is pending when the DMA queue starts (the round-5
// note in attention_decode.hip); they are waited for together with the first K chunk.
template <int DS>
__device__ __forceinline__ void dec_load_q(const _Float16* qh, int ldq, int Sq, int rl, int g, sc_u4 (&qf)[DS]) {
    const int qr = rl < Sq ? rl : Sq - 1;
    const _Float16* qp = qh + (size_t)qr * (size_t)ldq + g * 8;
#pragma unroll
    for (int ds = 0; ds < DS; ++ds) asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(qf[ds]) : "v"(qp), "n"(ds * 64) : "memory");
}

// One exact online-softmax step over the 32 logits s (S^T fragments: lane (rl, g) holds keys kv0 + kvb * 16 + r of query rl, kv0 = c * 32 +
// g * 4): masks the keys at or past row_end, takes the row maximum over the four lane groups, rescales (l_run, o) and returns P as the B operand
// of the P.V MFMAs.  Exact (a rescale per chunk) because the loop is bandwidth-bound: the VALU work is free.
template <int DB>
__device__ __forceinline__ sc_h8 dec_softmax_step(sc_f4 (&s)[2], int kv0, int row_end, float scale_log2, float& m_run, float& l_run, sc_f4 (&o)[DB]) {
    float tmax = -INFINITY;
#pragma unroll
    for (int kvb = 0; kvb < 2; ++kvb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[kvb][r] = (kv0 + kvb * 16 + r < row_end) ? s[kvb][r] : -INFINITY;
            tmax = fmaxf(tmax, s[kvb][r]);
        }
    const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(tmax), __float_as_uint(tmax), false, false);
    tmax = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const auto bsw = __builtin_amdgcn_permlane32_swap(__float_as_uint(tmax), __float_as_uint(tmax), false, false);
    tmax = fmaxf(__uint_as_float(bsw[0]), __uint_as_float(bsw[1])) * scale_log2;
    const float m_new = fmaxf(m_run, tmax);
    const float m_use = (m_new == -INFINITY) ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
    m_run = m_new;
    l_run *= alpha;
#pragma unroll
    for (int db = 0; db < DB; ++db) o[db] *= alpha;
    sc_h8 pf;
    float ps = 0.f;
#pragma unroll
    for (int kvb = 0; kvb < 2; ++kvb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[kvb][r], scale_log2, -m_use));
            ps += p;
            pf[kvb * 4 + r] = (_Float16)p;
        }
    l_run += ps;
    return pf;
}

// The fp16 V chunk in LDS (32 rows of 256 B, the 16-byte piece p of row r in slot p ^ ((r & 7) << 1)) and its transposed reads (P.V needs V^T):
// dec_v_offsets gives lane (rl, g)'s read offsets, dec_read_vt reads the chunk at LDS address `sa` and returns once the data is in registers.
template <int DB>
__device__ __forceinline__ void dec_v_offsets(int rl, int g, unsigned (&v_off)[DB]) {
    const int vrow = 4 * g + (rl >> 2);
#pragma unroll
    for (int db = 0; db < DB; ++db) v_off[db] = (unsigned)(vrow * DEC_VROW + ((db ^ (vrow & 7)) << 5) + (rl & 3) * 8);
}
template <int DB>
__device__ __forceinline__ void dec_read_vt(unsigned sa, const unsigned (&v_off)[DB], sc_s4 (&lo)[DB], sc_s4 (&hi)[DB]) {
#pragma unroll
    for (int db = 0; db < DB; ++db) {
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo[db]) : "v"(sa + v_off[db]) : "memory");
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi[db]) : "v"(sa + v_off[db]), "n"(16 * DEC_VROW) : "memory");
    }
    static_assert(DB == 8, "the lgkmcnt fence below names 16 registers");
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo[0]), "+v"(hi[0]), "+v"(lo[1]), "+v"(hi[1]), "+v"(lo[2]), "+v"(hi[2]), "+v"(lo[3]), "+v"(hi[3]),
                                          "+v"(lo[4]), "+v"(hi[4]), "+v"(lo[5]), "+v"(hi[5]), "+v"(lo[6]), "+v"(hi[6]), "+v"(lo[7]), "+v"(hi[7]) :: "memory");
}

// O^T += V^T . P^T
template <int DB>
__device__ __forceinline__ void dec_pv(const sc_s4 (&lo)[DB], const sc_s4 (&hi)[DB], sc_h8 pf, sc_f4 (&o)[DB]) {
    typedef short sc_s8 __attribute__((ext_vector_type(8)));
#pragma unroll
    for (int db = 0; db < DB; ++db) {
        const sc_s8 v8 = {lo[db][0], lo[db][1], lo[db][2], lo[db][3], hi[db][0], hi[db][1], hi[db][2], hi[db][3]};
        o[db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(sc_h8, v8), pf, o[db], 0, 0, 0);
    }
}

// The NW waves of a workgroup cover consecutive shares of one split; they merge their (O, m, l) through LDS, so a workgroup leaves ONE partial
// per split in the layout k_attn_combine reads: `pp` is partial (query 0, this split) of this head, query q's is nsplit * (DH + 2) floats on.
// The merge buffer starts at smem and ALIASES the waves' rings.  That is safe because the caller has waited for vmcnt(0) - no LDS-DMA of this
// wave is in flight - and the barrier below is passed only once every wave has: all of them are done with their rings.
template <int NW, int DH, int DB>
__device__ __forceinline__ void dec_merge_waves(char* smem, const sc_f4 (&o)[DB], float m_run, float l_run, int tid, int wave, int rl, int g, int Sq,
                                                float* pp, int nsplit) {
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    __syncthreads();
    float* mo = reinterpret_cast<float*>(smem);             // [NW][DH][16] O^T, then [NW][16] m, [NW][16] l
    float* mm = mo + NW * DH * 16;
    float* ml = mm + NW * 16;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) mo[(wave * DH + db * 16 + g * 4 + r) * 16 + rl] = o[db][r];
    if (g == 0) { mm[wave * 16 + rl] = m_run; ml[wave * 16 + rl] = l_run; }
    __syncthreads();
    for (int e = tid; e < Sq * DH; e += 64 * NW) {
        const int q = e / DH, d = e - q * DH;
        float M = mm[q];
#pragma unroll
        for (int w = 1; w < NW; ++w) M = fmaxf(M, mm[w * 16 + q]);
        float acc = 0.f, l = 0.f;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float mw = mm[w * 16 + q];
            const float wt = (mw == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(mw - M);
            acc += mo[(w * DH + d) * 16 + q] * wt;
            l += ml[w * 16 + q] * wt;
        }
        float* pq = pp + (size_t)q * nsplit * (DH + 2);
        pq[d] = acc;
        if (d == 0) { pq[DH] = M; pq[DH + 1] = l; }
    }
}
