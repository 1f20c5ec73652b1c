#!/usr/bin/env python3
"""The batched caption decode step alone (B chunk captions decoded together, llm.BatchDecoder) at the product's shape:
B sequences x ctx cached tokens, Qwen2-7B random-init.  The caches are filled with random K/V instead of 26 real prefills (8 s), so
that a rocprofv3 trace of this command holds the decode step's kernels only.  ms per step and the HBM roofline fraction.
--kv_cache fp16 fp8: one decoder per cache format in ONE process, their timed legs interleaved (fp16, fp8, fp16, fp8: the yardstick of the
e4m3 cache is the fp16 leg of the same process); the e4m3 caches hold random valid codes and power-of-two scales, bytes counted per format.
--decode_weights fp16 fp8: per cache format ONE decoder whose weight mode alternates from leg to leg (each generate() captures its own graph),
so the yardstick of the e4m3 weights is the fp16-weight leg of the same process on the same caches; GB_per_step counts each leg's real weight bytes.
--launches: instead of the step, us per launch of the step's five projections at M = --chunks, walking the 28 layers' tensors in turn (so that no
weight is served from a cache), captured as one graph: ops.gemm, ops.gemm_w8 as dispatched, and - in a child process, the switch is read once - ops.gemm_w8 pinned to
the generic kernel (SC_SKINNY_W8_GENERIC=1)."""
import argparse, json, os, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from streamchat_amd import llm as LM

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=26)
ap.add_argument("--ctx", type=int, default=22740)
ap.add_argument("--new", type=int, default=48)
ap.add_argument("--eager", action="store_true")
ap.add_argument("--nsplit", type=int, nargs="*", default=[0])
ap.add_argument("--kv_cache", type=str, nargs="+", choices=list(LM.KV_CACHE), default=["fp16"])
ap.add_argument("--legs", type=int, default=0, help="timed legs per cache format and split factor (default: 1, or 2 with several formats)")
ap.add_argument("--decode_weights", type=str, nargs="+", choices=list(LM.DECODE_WEIGHTS), default=["fp16"])
ap.add_argument("--launches", action="store_true")
a = ap.parse_args()
cfg = LM.Qwen2ConfigLite(**LM.QWEN2_7B)
lm = LM.Qwen2Model(LM.random_qwen2_state_dict(cfg, seed=0), cfg, max_seq=4096, consume=True)
g = torch.Generator(device="cuda").manual_seed(1)
wmodes = list(dict.fromkeys(a.decode_weights))
w8 = lm._w8_tensors() if "fp8" in wmodes or a.launches else None
if a.launches:
    from streamchat_amd import ops
    M, pinned = a.chunks, os.environ.get("SC_SKINNY_W8_GENERIC") == "1"
    x = {k: (torch.randn(M, k, device="cuda", generator=g) * 0.05).half() for k in (cfg.hidden, cfg.heads * cfg.head_dim, cfg.intermediate)}
    res = torch.zeros(M, cfg.hidden, dtype=torch.float16, device="cuda")
    shapes = [("qkv", "wqkv", "sqkv", dict(out_f32=True)), ("o", "wo", "so", dict(residual=res)), ("gate_up", "wgu", "sgu", dict(epilogue="swiglu")),
              ("down", "wd", "sd", dict(residual=res))]

    def timed(fn, n, reps=8):
        """us per launch: n launches captured as ONE hipGraph (the step runs from a graph: no host time between kernels), replayed reps times"""
        for i in range(2):
            fn(i)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for i in range(n):
                fn(i)
        graph.replay(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            graph.replay()
        e1.record(); torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / (n * reps)
    for name, wk, sk, kw in shapes:
        K = lm.L[0][wk].shape[1]
        bias = lm.L[0]["bqkv"] if name == "qkv" else None
        r = dict(proj=name, M=M, N=lm.L[0][wk].shape[0], K=K, generic_pinned=pinned,
                 w8_us=round(timed(lambda i: ops.gemm_w8(x[K], w8["L"][i % cfg.layers][wk], w8["L"][i % cfg.layers][sk], bias, **kw), 4 * cfg.layers), 2))
        if not pinned:
            r["fp16_us"] = round(timed(lambda i: ops.gemm(x[K], lm.L[i % cfg.layers][wk], bias, **kw), 4 * cfg.layers), 2)
        print(json.dumps(r), flush=True)
    r = dict(proj="lm_head", M=M, N=lm.lm_head.shape[0], K=cfg.hidden, generic_pinned=pinned,
             w8_us=round(timed(lambda i: ops.gemm_w8(x[cfg.hidden], w8["lm_head"], w8["slm_head"], None, out_f32=True), 10), 2))
    if not pinned:
        r["fp16_us"] = round(timed(lambda i: ops.gemm(x[cfg.hidden], lm.lm_head, None, out_f32=True), 10), 2)
    print(json.dumps(r), flush=True)
    if not pinned:
        sys.stdout.flush()
        subprocess.run([sys.executable, os.path.abspath(__file__), "--launches", "--chunks", str(M)], env=dict(os.environ, SC_SKINNY_W8_GENERIC="1"), check=True, timeout=600)
    sys.exit(0)
prompts = [(torch.randn(16, cfg.hidden, device="cuda", generator=g) * 0.02).half() for _ in range(a.chunks)]
decs = {}
for mode in dict.fromkeys(a.kv_cache):
    dec = decs[mode] = LM.BatchDecoder(lm, prompts, a.ctx + a.new, kv_cache=mode)          # cap = 16 + ctx + new rows per sequence
    if mode == "fp8":
        for kb, ks in dec.kv8:
            kb.random_(0, 254, generator=g)                    # the 254 finite codes: 0x7F and 0xFF (NaN) are skipped
            kb.add_(kb >= 127)
            ks.copy_(torch.exp2(torch.randint(-14, 8, ks.shape, device="cuda", generator=g).float()))
    else:
        for c in dec.cache:
            c.normal_(0, 0.5)
torch.cuda.synchronize()
w = 2 * cfg.kv_heads * cfg.head_dim
row_bytes = {"fp16": 2 * w, "fp8": w + 2 * cfg.kv_heads * 4}        # K | V of one cached token and layer: halves, or bytes + one fp32 scale per segment
n_w = sum(t.numel() for L in lm.L for t in (L["wq"], L["wkv"], L["wo"], L["wgu"], L["wd"])) + lm.lm_head.numel()
n_rows = sum(t.shape[0] for L in lm.L for t in (L["wq"], L["wkv"], L["wo"], L["wgu"], L["wd"])) + lm.lm_head.shape[0]
w_bytes_of = {"fp16": n_w * 2, "fp8": n_w + n_rows * 4}              # halves, or bytes + one fp32 scale per output row
legs = a.legs or (2 if len(decs) > 1 or len(wmodes) > 1 else 1)


for ns in a.nsplit:
    for dec in decs.values():
        dec.nsplit_override = ns or None
        for wm in wmodes:
            dec.set_decode_weights(wm)
            dec.len.fill_(a.ctx)
            dec.generate(8, use_graph=not a.eager)                 # warm-up (captures a graph of its own)
    for leg in range(legs):
        for mode, wm in ((m, w) for m in decs for w in wmodes):
            dec, w_bytes = decs[mode], w_bytes_of[wm]
            dec.set_decode_weights(wm)
            dec.len.fill_(a.ctx)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            dec.generate(a.new, use_graph=not a.eager)
            torch.cuda.synchronize(); dt = time.perf_counter() - t0
            steps = a.new - 1
            kv_bytes = a.chunks * (a.ctx + a.new / 2) * row_bytes[mode] * cfg.layers
            print(json.dumps(dict(kv_cache=mode, decode_weights=wm, leg=leg, chunks=a.chunks, ctx=a.ctx, steps=steps, ms_per_step=round(1e3 * dt / steps, 3),
                                  tok_per_s=round(a.chunks * steps / dt, 1), GB_per_step=round((w_bytes + kv_bytes) / 1e9, 2),
                                  TBps=round((w_bytes + kv_bytes) / (dt / steps) / 1e12, 3), frac_of_8TBps=round((w_bytes + kv_bytes) / (dt / steps) / 8e12, 3),
                                  nsplit=dec.nsplit)), flush=True)
