/* streamchat_hip_w8.h — extension of streamchat_hip.h: FP8 (OCP e4m3fn) weight-only batch-1 decode projections.
 *
 * Batch-1 decode is a pure weight stream (14.1 of the 16.9 GB a Qwen2-7B token reads at a 49 k context are weights);
 * per-output-row e4m3 weights halve those bytes.  This is an ACCURACY trade (about 2.6 % relative rms error on N(0, 0.02^2) weights), so
 * nothing in the base header changes and no caller gets it without asking (llm.Qwen2Model.enable_fp8_decode, SC_DECODE_WEIGHTS=fp8).
 * The kernels are pinned against the DEQUANTISED weights: e4m3 x fp16 products are exact in fp32, so against those they owe the accuracy
 * of sc_gemv_f16.
 *
 * Extension changelog (additive; base ABI 9 - sc_abi_version() and SC_ABI_VERSION of streamchat_hip.h are unchanged, a binding that does
 * not use these symbols is unaffected; one that does looks the three symbols up and fails if the library lacks them):
 *   w8-1  + sc_quantize_rows_e4m3, sc_gemv_w8_f16, sc_decode_qkv_tab_w8
 *
 * Conventions: those of streamchat_hip.h.  gfx950 speaks OCP e4m3fn (bias 7, no infinities, 0x7F / 0xFF = NaN, max 448), NOT the e4m3fnuz of
 * gfx942: the bytes are torch.float8_e4m3fn's.
 */
#ifndef STREAMCHAT_HIP_W8_H
#define STREAMCHAT_HIP_W8_H

#include "streamchat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-row quantiser (runs once at load; on the device because the library has no host path).  W fp16 [N, K], rows ldw halves apart
 * (K % 8 == 0, ldw % 8 == 0, W 16-byte aligned) -> q uint8 [N, K] dense (8-byte aligned), scale fp32 [N]:
 *   amax = max |W[n, :]| (fp32);  scale[n] = amax > 0 ? amax / 448 : 1;  q[n, k] = e4m3fn(clamp(W[n, k] / scale[n], -448, 448)),
 * fp32 IEEE division, round to nearest even, the sign of zero kept.  Bit-identical to torch on the CPU:
 *   s = where(amax > 0, amax / 448, 1);  (W.float() / s[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn) */
int sc_quantize_rows_e4m3(const void* W, int ldw, int N, int K, uint8_t* q, float* scale, sc_stream_t stream);

/* sc_gemv_f16 with e4m3 weight rows and one fp32 scale per row:
 *   y[n] = scale[n] * sum_k q[n, k] * xh[k]  (+ bias[n]) (+ residual[n]),   or the SC_EPI_SWIGLU epilogue on the (g g u u) row interleave;
 * xh = x, or the fused Qwen2 RMSNorm of x rounded to fp16 once (rms_gamma != NULL: the arithmetic and the reduction order of
 * sc_gemv_f16).  fp32 accumulation, the scale applied once per row after the sum.  Arguments as sc_gemv_f16 (fp16 or fp32 output, `y_row`:
 * a device-resident output row of a [rows, y_ld] fp16 buffer).  Requires K % 16 == 0, K <= 32752, W and x 16-byte aligned (so every weight
 * row is): anything else is SC_ERR_ARG with a message before any device work.  The result bits do not depend on SC_GEMV_WPB_*. */
int sc_gemv_w8_f16(const uint8_t* W, const float* scale, const void* x, const void* bias, const void* residual, void* y, int N, int K,
                   int epilogue, int out_f32, const int32_t* y_row, int y_ld, const void* rms_gamma, float rms_eps, sc_stream_t stream);

/* sc_decode_qkv_tab_f16 with e4m3 weights: fused RMSNorm (rms_gamma may be NULL: x is taken as it is), q | k | v rows from Wq / Wkv with
 * their row scales, + bias, the one-rounding rotary with the fp32 tables at position pos[0] (clamped to the table), q -> q_out, k | v ->
 * cache row pos[0].  Bit-identical to sc_gemv_w8_f16(out_f32 = 1) + sc_rope_f32in_f16.  K % 16 == 0, K <= 32752. */
int sc_decode_qkv_tab_w8(const uint8_t* Wq, const float* scale_q, const uint8_t* Wkv, const float* scale_kv, const void* bq, const void* bkv,
                         const void* x, const void* rms_gamma, float rms_eps, void* q_out, void* cache, int cache_ld, const int32_t* pos,
                         int q_heads, int kv_heads, int Dh, int K, const float* tab_q, const float* tab_k, int tab_rows, sc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
