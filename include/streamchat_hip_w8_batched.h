/* streamchat_hip_w8_batched.h - changelog entry w8-2 of streamchat_hip_w8.h: FP8 (OCP e4m3fn) weights for the BATCHED decode step
 * (llm.BatchDecoder: the chunk captions of a product step and every beam search).  Its projections are GEMMs with M = the number of sequences
 * (at most 32 rows per launch), so the weights - 14.1 GB per step at Qwen2-7B's widths whatever the batch - stream once per step; e4m3 rows
 * halve those bytes.  Format, accuracy trade and conventions: streamchat_hip_w8.h (the tensors are sc_quantize_rows_e4m3's).
 *
 *   w8-2  + sc_gemm_w8_f16
 *
 * Additive (base ABI 9, sc_abi_version() and every existing symbol unchanged); a binding looks the symbol up and fails if the library lacks it.
 * The call allocates nothing and takes no workspace: it is hipGraph-capturable.
 */
#ifndef STREAMCHAT_HIP_W8_BATCHED_H
#define STREAMCHAT_HIP_W8_BATCHED_H

#include "streamchat_hip_w8.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The M <= 32 case of sc_gemm_f16 with e4m3 weight rows and one fp32 scale per row:
 *   C[m, n] = epi(scale[n] * sum_k e4m3fn(W[n, k]) * A[m, k] + bias[n]) (+ R[m, n])
 * A [M, K] fp16 (rows lda halves apart), W dense [N, K] e4m3fn bytes, scale fp32 [N], bias fp16 [N] or NULL, R fp16 (rows ldr apart) or NULL,
 * C fp16 or fp32 (out_f32), rows ldc elements apart.  Weight-only: a byte is converted to the fp16 value it denotes (exact) and multiplied with
 * the fp16 activation in the fp16 MFMA; products are exact in fp32, sums are fp32, the row scale is applied once, to the finished sum, in one
 * fma with the bias.  Epilogues: SC_EPI_NONE, and SC_EPI_SWIGLU on the (g g u u) row interleave (fp16 output of N / 2 columns, no residual);
 * any other epilogue is SC_ERR_UNSUPPORTED.
 * Requires 1 <= M <= 32, N % 16 == 0, K % 128 == 0, lda % 8 == 0, ldc % 4 == 0, ldr % 4 == 0, A and W 16-byte aligned, bias / R / fp16 C 8-byte
 * and fp32 C 16-byte aligned: anything else is SC_ERR_ARG with a message before any device work.
 * Row m of C depends on row m of A alone - not on M, not on the other rows - and every kernel behind the call adds in the same order, so the
 * bits do not depend on which one served it (SC_SKINNY_W8_GENERIC=1, read once per process, pins the run-time-loop kernel).  A caller with
 * more than 32 rows launches row blocks and gets the bits of the rows' own launches.  Persistent kernels size themselves by the stream's CU
 * partition. */
int sc_gemm_w8_f16(const void* A, int lda, const uint8_t* W, const float* scale, const void* bias, const void* R, int ldr, void* C, int ldc,
                   int M, int N, int K, int epilogue, int out_f32, sc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
