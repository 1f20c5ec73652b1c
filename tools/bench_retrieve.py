#!/usr/bin/env python3
"""The retrieve stage of the bench step on its own: MiniLM dialogue search + BERT-large caption-tree search with a fresh caption cache, on
what bench.Pipeline builds for it (random-init encoders, hash tokenizer, 32 dialogue documents, a 26-node tree: one merged node with 10
children and 16 depth-0 nodes, synthetic captions, the bench's question).  Reports, per call: wall time (synchronised at both ends),
GPU-busy time (KernelTimer sum) and launches; and the host time of one `ops` call with and without an active KernelTimer.
`--layerwise` pins the layer-by-layer encoder body (where the package has the one-call encoder); SC_GEMM_MID=0 pins the old GEMM dispatch."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from streamchat_amd import ops, synthetic, text as T, utiles as U
from streamchat_amd.memory_bank.memory_retrieval import local_doc_qa as Q

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--layerwise", action="store_true")
a = ap.parse_args()
dev = "cuda"
bl, ml = T.BertConfigLite(**T.BERT_LARGE), T.BertConfigLite(**T.MINILM_L6)
colbert = T.BertEncoder(T.random_bert_state_dict(bl, seed=2, device=dev), bl, device=dev)
minilm = T.BertEncoder(T.random_bert_state_dict(ml, seed=3, device=dev), ml, device=dev)
native = hasattr(ops, "text_encoder")
if a.layerwise and native:
    for enc in (colbert, minilm):
        fwd = enc.forward
        enc.forward = lambda ids, lengths=None, _f=fwd: _f(ids, lengths, layerwise=True)
tok = T.HashTokenizer()
sent = Q.HipSentenceEmbeddings(T.SentenceEmbedder(minilm), tok)
docs = [Q.Document(f"Conversation content on 2024-05-{1 + i // 8:02d}:[|User|]: {synthetic.caption(100 + i, words=8)}; "
                   f"[|AI|]: {synthetic.caption(200 + i, words=10)}", {"source": f"2024-05-{1 + i // 8:02d}"}) for i in range(32)]
question = "where did I leave the red cup and what was on the kitchen table"
feat = torch.zeros((1, 8, 64), dtype=torch.float16, device=dev)
merged = U.MultimodalTreeNode(feat, synthetic.caption(999), depth=1)
merged.children = [U.MultimodalTreeNode(feat, synthetic.caption(i)) for i in range(10)]
tree = [merged] + [U.MultimodalTreeNode(feat, synthetic.caption(10 + i)) for i in range(16)]


def retrieve():
    lm = Q.LocalMemoryRetrieval()
    lm.init_cfg("minilm-l6", top_k=1, language="en", embedder=sent)
    store = Q.FlatL2VectorStore(docs, lm._embed_docs(docs), sent.embed_query)
    lm.search_memory(question, store)
    return U.fast_search_tree_multi_modal_with_embedding(tree, question, feat, colbert, tok, cache=U.CaptionEmbeddingCache())


def wall(n):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        retrieve()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


for _ in range(a.warmup):
    text = retrieve()[1]
plain = wall(a.iters)
with ops.KernelTimer() as kt:
    timed = wall(a.iters)
    s = kt.summary()
busy = sum(v[1] for v in s.values()) / a.iters
launches = sum(v[0] for v in s.values()) / a.iters

# host cost of one ops call: a 16 x 128 x 1024 GEMM, enqueued back to back (the queue never drains: host time per call)
x, w = torch.randn(16, 1024, device=dev).half(), torch.randn(128, 1024, device=dev).half()
def host_us(n=2000):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n):
        ops.gemm(x, w)
    t1 = time.perf_counter(); torch.cuda.synchronize()
    return 1e6 * (t1 - t0) / n
host_us(200)
h_plain = host_us()
with ops.KernelTimer() as kt2:
    h_timed = host_us()
    kt2.records.clear()
print(json.dumps(dict(native_encoder=bool(native and not a.layerwise), gemm_mid=os.environ.get("SC_GEMM_MID", "1") != "0", iters=a.iters,
                      wall_ms=round(plain, 3), wall_ms_with_timer=round(timed, 3), gpu_busy_ms=round(busy, 3), launches=launches,
                      host_us_per_ops_call=round(h_plain, 2), host_us_per_ops_call_with_timer=round(h_timed, 2),
                      kernels={k: dict(n=v[0] / a.iters, ms=round(v[1] / a.iters, 3)) for k, v in sorted(s.items())}, path_text_crc=__import__("zlib").crc32("|".join(text).encode()))))
