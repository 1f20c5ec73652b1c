/* streamchat_hip_kv8.h — extension of streamchat_hip.h: FP8 (OCP e4m3fn) KV cache for batch-1 decode.
 *
 * With FP8 weights (streamchat_hip_w8.h) the untouched fp16 attention is 37 % of a decode step at a 49 k context, and what is left of it is
 * bytes: an e4m3 cache halves them and the cache's footprint.  This is an ACCURACY trade (about 2.65 % relative rms error on
 * N(0, s^2) segments), so nothing in the base header changes and no caller gets it without asking (llm.Qwen2Model(kv_cache="fp8"),
 * SC_KV_CACHE=fp8).
 *
 * Format.  A cache row is [K of all KV heads | V of all KV heads], Dh = 128 bytes per head; every 128-element segment (one head's K or V of one
 * row) has ONE power-of-two fp32 scale, stored in a dense [rows, 2 * kv_heads] array in the same order:
 *   amax = max |x| (fp32);  e = 0 if amax == 0, else the smallest integer with 448 * 2^e >= amax, clamped to [-14, 7];  scale = 2^e;
 *   code = e4m3fn(clamp(x / scale, -448, 448)), round to nearest even, the sign of zero kept.
 * code * 2^e is exactly representable in fp16 for every code and every e in [-14, 7], so sc_attention_kv8 hands the MFMA exactly the operands
 * sc_attention_f16 sees on the dequantised cache: its results are bit-identical to that call.
 *
 * Extension changelog (additive; base ABI 9 - sc_abi_version() and SC_ABI_VERSION of streamchat_hip.h are unchanged, a binding that does
 * not use these symbols is unaffected; one that does looks the three symbols up and fails if the library lacks them):
 *   kv8-1  + sc_kv8_quantize_rows, sc_kv8_dequantize_rows, sc_attention_kv8
 *   kv8-2  + sc_attention_kv8_batched, sc_kv8_rope_qkv_rows: the cache of the BATCHED decode (llm.BatchDecoder(kv_cache="fp8")).  Purely additive:
 *            the three symbols above keep their signatures and their bits (sc_attention_kv8 is now the B = 1 launch of the batched kernel).  The
 *            two are declared in streamchat_hip_kv8_batched.h, which includes this header: the set of symbols THIS file declares is what a kv8-1
 *            binding checks itself against (tests/test_kv8_cpu.py) and stays as it is.
 *
 * Conventions: those of streamchat_hip.h.  Head dim 128 only: anything else is SC_ERR_UNSUPPORTED with a message before any device work.
 */
#ifndef STREAMCHAT_HIP_KV8_H
#define STREAMCHAT_HIP_KV8_H

#include "streamchat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fp16 rows -> bytes and scales of the cache rows r0 .. r0 + n - 1, r0 = row0_dev ? row0_dev[0] : row0 (a device-resident row keeps a decode
 * step hipGraph-replayable, as `pos` of sc_decode_qkv_tab_f16).  x: rows of 2 * kv_heads * Dh halves, ld halves apart (ld % 8 == 0, 16-byte
 * aligned); source row i is x + i * ld, or with x_follows_row != 0 x + (r0 + i) * ld (x is a buffer laid out row for row like the cache).
 * cache: uint8 rows cache_ld bytes apart (cache_ld % 8 == 0, 8-byte aligned), scales: fp32 [cache_rows, 2 * kv_heads] dense.  Writes exactly
 * the 2 * kv_heads * Dh bytes and the 2 * kv_heads scales of those rows - not the row pad, not a neighbouring row; a row outside
 * [0, cache_rows) is skipped.  Bit-identical to the specification above evaluated with torch on the CPU (tests/_kv8.py). */
int sc_kv8_quantize_rows(const void* x, int ld, int n, int kv_heads, int Dh, uint8_t* cache, int cache_ld, float* scales, int cache_rows,
                         int row0, const int32_t* row0_dev, int x_follows_row, sc_stream_t stream);

/* the inverse: out row i (fp16, 2 * kv_heads * Dh halves, ld halves apart, 16-byte aligned) = code * scale of cache row row0 + i, exact.
 * Requires 0 <= row0, row0 + n <= cache_rows. */
int sc_kv8_dequantize_rows(const uint8_t* cache, int cache_ld, const float* scales, int cache_rows, int row0, int n, int kv_heads, int Dh,
                           void* out, int ld, sc_stream_t stream);

/* Split-KV decode attention of sc_attention_f16's streaming kernel over an e4m3 cache: Sq <= 16 query rows per KV head (batch-1 decode packs
 * the G = Hq / Hkv query heads of a KV group as G rows: row stride ldq, head stride q_head_stride, 0 = Dh), non-causal, Skv cache rows of which
 * min(kv_len[0], Skv) are valid (kv_len device-resident, NULL = Skv); rows past that contribute nothing whatever the memory there holds.
 * flags: 0 or SC_ATTN_Q_PRESCALED (q already carries scale * log2 e).  nsplit in [1, 1024] partials go to the caller's workspace
 * (kv_heads * Sq * nsplit * (Dh + 2) floats, else SC_ERR_WORKSPACE) in the layout the split-KV merge of sc_attention_f16 reads; that merge
 * writes out[q * ldo + h * o_head_stride + d] (0 = Dh).  Every operand reaches the fp16 MFMA as fp16(code * scale): bit-identical to
 * sc_attention_f16 with the same nsplit on the dequantised cache. */
int sc_attention_kv8(const void* q, int ldq, const uint8_t* cache, int cache_ld, const float* scales, void* out, int ldo, int Sq, int Skv,
                     int kv_heads, int Dh, float scale, int flags, const int32_t* kv_len, int nsplit, void* ws, size_t ws_bytes,
                     int q_head_stride, int o_head_stride, sc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
