// A whole post-LN text-encoder stack (HF BertModel arithmetic: BERT-large "mxbai-colbert", all-MiniLM-L6) from ONE call of the C ABI.
//
// The kernels of these forwards run 6 - 33 us each and there are seven of them per layer; driven one ctypes call at a time the host cannot
// keep ahead of them (profiles/r12_text_encoder_native_ab.md).  sc_text_encoder_f16 enqueues exactly the launches the layer-by-layer body
// (streamchat_amd/text.py, BertEncoder.forward(layerwise=True)) issues, through the same entry points - same dispatch, same operand strides,
// same order - so the hidden states are bit-identical to that body's; only the host side of the launches changes.
// No state: every buffer is carved from the caller's scratch, the layer table is read during the call only.
#include <math.h>

#include "sc_common.h"
#include "../../include/streamchat_hip_text.h"

namespace {

struct Scratch {                        // [M, *] fp16 buffers, each 256-byte aligned
    size_t x, qkv, att, y, x1, f, total;
    Scratch(size_t M, size_t H, size_t I) {
        size_t o = 0;
        auto take = [&](size_t cols) { const size_t at = o; o += sc_align_up(M * cols * 2, 256); return at; };
        x = take(H); qkv = take(3 * H); att = take(H); y = take(H); x1 = take(H); f = take(I);
        total = o;
    }
};

}  // namespace

extern "C" size_t sc_text_encoder_workspace_bytes(int rows, int hidden, int intermediate) {
    if (rows <= 0 || hidden <= 0 || intermediate <= 0) return 0;
    return Scratch((size_t)rows, (size_t)hidden, (size_t)intermediate).total;
}

#define SC_TRY(call)                \
    do {                            \
        const int rc_ = (call);     \
        if (rc_ != SC_OK) return rc_; \
    } while (0)

extern "C" int sc_text_encoder_f16(const sc_text_encoder_layer* layers, int n_layers, int hidden, int heads, int intermediate, float eps,
                                   const void* word, const void* pos, const void* type0, const void* emb_gamma, const void* emb_beta, int vocab,
                                   const int32_t* ids, const int32_t* kv_len, int B, int L, void* hidden_out, void* ws, size_t ws_bytes,
                                   sc_stream_t stream) {
    SC_REQUIRE(layers && word && pos && type0 && emb_gamma && emb_beta && ids && hidden_out && ws, "sc_text_encoder_f16: null pointer argument");
    SC_REQUIRE(n_layers > 0 && B > 0 && L > 0 && vocab > 0, "sc_text_encoder_f16: n_layers, B, L, vocab must be positive");
    SC_REQUIRE(heads > 0 && hidden > 0 && hidden % heads == 0, "sc_text_encoder_f16: hidden (%d) must be a multiple of heads (%d)", hidden, heads);
    const int H = hidden, I = intermediate, Dh = hidden / heads;
    SC_REQUIRE(H % 128 == 0 && I % 128 == 0 && (Dh == 32 || Dh == 64 || Dh == 128),
               "sc_text_encoder_f16: hidden / intermediate must be multiples of 128 and the head width 32, 64 or 128");
    SC_REQUIRE((long long)B * L * (long long)(3 * H > I ? 3 * H : I) < (1ll << 31), "sc_text_encoder_f16: B * L * width exceeds 2^31 elements");
    const int M = B * L;
    const Scratch sc((size_t)M, (size_t)H, (size_t)I);
    if (ws_bytes < sc.total) return sc_fail(SC_ERR_WORKSPACE, "sc_text_encoder_f16: workspace %zu < required %zu bytes", ws_bytes, sc.total);
    SC_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "sc_text_encoder_f16: workspace must be 256-byte aligned");
    for (int l = 0; l < n_layers; ++l) {
        const sc_text_encoder_layer& p = layers[l];
        SC_REQUIRE(p.wqkv && p.bqkv && p.wo && p.bo && p.ln1_g && p.ln1_b && p.w1 && p.b1 && p.w2 && p.b2 && p.ln2_g && p.ln2_b,
                   "sc_text_encoder_f16: layer %d has a null parameter pointer", l);
    }
    char* w8 = static_cast<char*>(ws);
    _Float16* x = reinterpret_cast<_Float16*>(w8 + sc.x);
    _Float16* qkv = reinterpret_cast<_Float16*>(w8 + sc.qkv);
    void *att = w8 + sc.att, *y = w8 + sc.y, *x1 = w8 + sc.x1, *f = w8 + sc.f;
    const float scale = (float)pow((double)Dh, -0.5);
    const int64_t qbs = B > 1 ? (int64_t)L * 3 * H : 0, obs = B > 1 ? (int64_t)L * H : 0;

    SC_TRY(sc_bert_embed_ln_f16(ids, word, pos, type0, emb_gamma, emb_beta, eps, x, B, L, H, vocab, stream));
    for (int l = 0; l < n_layers; ++l) {
        const sc_text_encoder_layer& p = layers[l];
        void* out = l + 1 == n_layers ? hidden_out : (void*)x;
        SC_TRY(sc_gemm_f16(x, H, p.wqkv, p.bqkv, nullptr, 0, qkv, 3 * H, M, 3 * H, H, SC_EPI_NONE, 0, 0, 0, 0, stream));
        SC_TRY(sc_attention_f16(qkv, 3 * H, qkv + H, 3 * H, qkv + 2 * H, 3 * H, att, H, B, L, L, heads, heads, Dh, scale, 0, kv_len, 1, nullptr, 0,
                                0, 0, qbs, obs, stream));
        SC_TRY(sc_gemm_f16(att, H, p.wo, p.bo, x, H, y, H, M, H, H, SC_EPI_NONE, 0, 0, 0, 0, stream));
        SC_TRY(sc_layernorm_f16(y, H, p.ln1_g, p.ln1_b, eps, x1, H, M, H, stream));
        SC_TRY(sc_gemm_f16(x1, H, p.w1, p.b1, nullptr, 0, f, I, M, I, H, SC_EPI_GELU_ERF, 0, 0, 0, 0, stream));
        SC_TRY(sc_gemm_f16(f, I, p.w2, p.b2, x1, H, y, H, M, H, I, SC_EPI_NONE, 0, 0, 0, 0, stream));
        SC_TRY(sc_layernorm_f16(y, H, p.ln2_g, p.ln2_b, eps, out, H, M, H, stream));
    }
    return SC_OK;
}
