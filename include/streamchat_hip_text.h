/* streamchat_hip_text.h — extension of streamchat_hip.h: a whole text-encoder forward from ONE call.
 *
 * The retrieval encoders (BERT-large CLS embedding of the caption tree, reference utiles.py:704-708,725-729; MiniLM-L6 sentence embedding of
 * the dialogue memory, memory_bank/memory_retrieval/local_doc_qa.py:193) are stacks of seven short kernels per layer (6 - 33 us each).  Driven
 * through the base header one entry point at a time, a binding pays its per-call host cost 168 times per BERT-large forward and cannot keep
 * ahead of the GPU.  sc_text_encoder_f16 enqueues the same launches - sc_bert_embed_ln_f16, then per layer sc_gemm_f16 (q|k|v), sc_attention_f16,
 * sc_gemm_f16 (+ residual), sc_layernorm_f16, sc_gemm_f16 (GELU-erf), sc_gemm_f16 (+ residual), sc_layernorm_f16 - with the same operand
 * strides, in the same order, through the same dispatch: the hidden states are bit-identical to that sequence of base-header calls.
 *
 * Extension changelog (additive; base ABI 9 - sc_abi_version() and SC_ABI_VERSION of streamchat_hip.h are unchanged, a binding that does
 * not use these symbols is unaffected; one that does looks the two symbols up and fails if the library lacks them):
 *   text-1  + sc_text_encoder_workspace_bytes, sc_text_encoder_f16
 *
 * Conventions: those of streamchat_hip.h.  No process-wide or static state: scratch is the caller's, the layer table is only read during the
 * call (it may be freed or changed afterwards); re-entrant for distinct streams + workspaces.
 */
#ifndef STREAMCHAT_HIP_TEXT_H
#define STREAMCHAT_HIP_TEXT_H

#include "streamchat_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One post-LN encoder layer (HF BertLayer), all DEVICE pointers to fp16 data in the torch.nn.Linear layout:
 *   wqkv [3H, H] (query, key, value rows), bqkv [3H];  wo [H, H], bo [H];  ln1_g / ln1_b [H] (attention.output.LayerNorm);
 *   w1 [I, H], b1 [I] (intermediate.dense, GELU-erf);  w2 [H, I], b2 [H];  ln2_g / ln2_b [H] (output.LayerNorm).  16-byte aligned. */
typedef struct sc_text_encoder_layer {
    const void *wqkv, *bqkv, *wo, *bo, *ln1_g, *ln1_b, *w1, *b1, *w2, *b2, *ln2_g, *ln2_b;
} sc_text_encoder_layer;

/* scratch of a forward over `rows` = B * L token rows */
size_t sc_text_encoder_workspace_bytes(int rows, int hidden, int intermediate);

/* hidden_out [B * L, hidden] fp16 = last_hidden_state of the stack.
 *   layers      HOST array of n_layers structs
 *   hidden % 128 == 0, intermediate % 128 == 0, hidden / heads in {32, 64, 128}
 *   word [vocab, hidden], pos [>= L, hidden], type0 [hidden], emb_gamma / emb_beta [hidden]: HF BertEmbeddings (fp16)
 *   ids         [B, L] int32, right-padded;  kv_len [B] int32 valid tokens per row (the attention's padding mask) or NULL
 *   ws          sc_text_encoder_workspace_bytes(B * L, hidden, intermediate) bytes, 256-byte aligned; its contents before the call do not matter */
int sc_text_encoder_f16(const sc_text_encoder_layer* layers, int n_layers, int hidden, int heads, int intermediate, float eps,
                        const void* word, const void* pos, const void* type0, const void* emb_gamma, const void* emb_beta, int vocab,
                        const int32_t* ids, const int32_t* kv_len, int B, int L, void* hidden_out, void* ws, size_t ws_bytes,
                        sc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
