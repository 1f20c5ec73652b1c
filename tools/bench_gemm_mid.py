#!/usr/bin/env python3
"""Per-launch time of sc_gemm_f16 at the shapes k_gemm_mid takes over (and the MiniLM ones it leaves alone): the BERT-large layer GEMMs at the
bench's caption batches (M = 280, 448), MiniLM-L6's at its 32 documents, one ViT frame (M = 577), a short text-only Qwen2-7B prefill (M = 200).
Weights rotate through enough copies to exceed the 256 MB MALL, as the 604 MB of BERT-large do in the real forward; the launches are
replayed from one captured graph, so the figure is GPU time.  One process measures ONE
dispatch (SC_GEMM_MID is read once per process): run it with SC_GEMM_MID=0 and without, interleaved, and compare the JSON lines."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from streamchat_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
a = ap.parse_args()
SHAPES = [(f"bert-large M{M} {n}", M, N, K, epi, res) for M in (280, 448) for n, N, K, epi, res in
          (("qkv", 3072, 1024, "none", False), ("wo", 1024, 1024, "none", True), ("w1", 4096, 1024, "gelu", False), ("w2", 1024, 4096, "none", True))]
SHAPES += [(f"minilm M960 {n}", 960, N, K, epi, res) for n, N, K, epi, res in
           (("qkv", 1152, 384, "none", False), ("wo", 384, 384, "none", True), ("w1", 1536, 384, "gelu", False), ("w2", 384, 1536, "none", True))]
SHAPES += [("vit 1 frame wo", 577, 1024, 1024, "none", True), ("vit 1 frame fc1", 577, 4096, 1024, "quick_gelu", False), ("vit 1 frame fc2", 577, 1024, 4096, "none", True),
           ("qwen2-7b M200 o", 200, 3584, 3584, "none", True), ("qwen2-7b M200 down", 200, 3584, 18944, "none", True)]
g = torch.Generator(device="cuda").manual_seed(0)
rn = lambda *s, std=1.0: (torch.randn(*s, device="cuda", generator=g) * std).half()
out = {}
for name, M, N, K, epi, res in SHAPES:
    copies = max(2, -(-(512 << 20) // (N * K * 2)))
    ws = [rn(N, K, std=0.03) for _ in range(copies)]
    x, b, r, y = rn(M, K), rn(N, std=0.1), (rn(M, N) if res else None), torch.empty(M, N, dtype=torch.float16, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for i in range(3):
            ops.gemm(x, ws[i % copies], b, r, epi, out=y)
        s.synchronize()
        graph = torch.cuda.CUDAGraph()                 # one linear chain of launches: GPU time per launch without the host in the way
        with torch.cuda.graph(graph, stream=s):
            for i in range(a.iters):
                ops.gemm(x, ws[i % copies], b, r, epi, out=y)
        graph.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        s.synchronize()
    out[name] = round(1e3 * e0.elapsed_time(e1) / a.iters, 2)
    del graph
    del ws
print(json.dumps(dict(gemm_mid=os.environ.get("SC_GEMM_MID", "1") != "0", iters=a.iters, us_per_launch=out)))
