/* streamchat_hip_kv8_batched.h - changelog entry kv8-2 of streamchat_hip_kv8.h: the FP8 (OCP e4m3fn) KV cache for the BATCHED decode step
 * (llm.BatchDecoder: the chunk captions of a product step and every beam search).  K/V is about 70 % of the bytes of that step at the product
 * shape (26 sequences x 22.7 k tokens), against about 27 % in the batch-1 decode.  Format, accuracy trade and conventions: streamchat_hip_kv8.h.
 * One cache is uint8 [B, rows, cache_ld] with scales fp32 [B, rows, 2 * kv_heads] dense; sequence b's slice is an sc_attention_kv8 cache.
 *
 * Additive (base ABI 9, sc_abi_version() and every existing symbol unchanged); a binding looks the two symbols up and fails if the library lacks
 * them.  Head dim 128 only: anything else is SC_ERR_UNSUPPORTED with a message before any device work.  Both calls are hipGraph-capturable:
 * everything that changes from step to step (positions, kv_len) is device data.
 */
#ifndef STREAMCHAT_HIP_KV8_BATCHED_H
#define STREAMCHAT_HIP_KV8_BATCHED_H

#include "streamchat_hip_kv8.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sc_attention_kv8 for B sequences in ONE launch of the same kernel (grid z = sequence).  Sequence b: q rows at q + b * q_batch_stride halves
 * (0 = Sq * ldq), bytes at cache + b * cache_batch_stride (BYTES, 64-bit, a multiple of 16, at least Skv * cache_ld), scales at
 * scales + b * Skv * 2 * kv_heads, min(max(kv_len[b], 0), Skv) valid rows (kv_len device-resident, NULL = Skv; 0 rows give a zero output row),
 * out rows at out + b * o_batch_stride halves (0 = Sq * ldo).  A sequence's base goes into the 64-bit base of the kernel's buffer resources and
 * its extents stay per sequence: rows behind kv_len[b], the row pad and the next sequence's rows are never read.  One sequence's slice stays
 * below 2 GiB (Skv * cache_ld < 2^31); the whole allocation may exceed it.  Workspace: B * kv_heads * Sq * nsplit * (Dh + 2) floats, else
 * SC_ERR_WORKSPACE.  For every b bit-identical to sc_attention_kv8 on slice b with the same nsplit, hence to sc_attention_f16 (batched, same
 * nsplit and kv_len) on the dequantised caches. */
int sc_attention_kv8_batched(const void* q, int ldq, const uint8_t* cache, int cache_ld, int64_t cache_batch_stride, const float* scales, void* out,
                             int ldo, int B, int Sq, int Skv, int kv_heads, int Dh, float scale, int flags, const int32_t* kv_len, int nsplit, void* ws,
                             size_t ws_bytes, int q_head_stride, int o_head_stride, int64_t q_batch_stride, int64_t o_batch_stride, sc_stream_t stream);

/* The e4m3 sibling of sc_rope_qkv_rows_f16: x [B, (q_heads + 2 kv_heads) * Dh] fp32 (fused q | k | v projection + bias of one new token per
 * sequence, ldx floats apart), tab_q / tab_k (sc_rope_table_f32, tab_rows rows), device positions[B], clamped to the table and to
 * [0, cache_rows) exactly as there.  q heads rotated -> q_out [B, q_heads * Dh] fp16, the bits of sc_rope_qkv_rows_f16.  The rotated K heads and
 * the cast V heads of sequence b are rounded to fp16 ONCE, as there, and that fp16 value is quantised by the specification of
 * streamchat_hip_kv8.h in registers: bytes to cache + b * cache_batch_stride + positions[b] * cache_ld (bytes; strides multiples of 8), scales to
 * scales[(b * cache_rows + positions[b]) * 2 * kv_heads ..].  One launch, no fp16 K | V row in memory.  Bytes and scales are bit-identical to
 * sc_rope_qkv_rows_f16 into an fp16 row followed by sc_kv8_quantize_rows of that row.  Writes exactly q_out and those B rows' 2 * kv_heads * Dh
 * bytes and 2 * kv_heads scales. */
int sc_kv8_rope_qkv_rows(const float* x, int ldx, const float* tab_q, const float* tab_k, int tab_rows, const int32_t* positions, int B, int q_heads,
                         int kv_heads, int Dh, void* q_out, int ldq, uint8_t* cache, int64_t cache_batch_stride, int cache_ld, float* scales,
                         int cache_rows, sc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
