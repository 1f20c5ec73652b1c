#!/usr/bin/env python3
"""A/B of the batch-1 answer decode from fp16 and from FP8 (e4m3) weights (llm.Qwen2Model.enable_fp8_decode), in ONE process.

Random-init Qwen2-7B, a 49 k-token context in the KV cache (filled with N(0, 0.5^2) rows as tools/bench_decode.py does: the decode kernels' time
does not depend on the values), 512 tokens per leg through DecodeGraph, the fp16 and fp8 legs interleaved for --rounds rounds.  Prints one JSON
line: tok/s per leg (every round + median), the fp16 legs' own spread, weight / total bytes per token and the fraction of 8 TB/s they amount to,
and - `--launches` - the time of every decode projection launch in both formats (a captured graph of one launch per layer, so the weights of 28
layers cycle through and nothing is served from the cache), and - `--agreement` - the fp8-vs-fp16 logit distance and top-1 agreement over
the tokens of the fp16 answer (teacher-forced: both models are fed the fp16 model's tokens).

    python tools/decode_w8_ab.py [--ctx 49152] [--tokens 512] [--rounds 3] [--launches] [--agreement]
    rocprofv3 --kernel-trace --stats -- python tools/decode_w8_ab.py --rounds 1        (the per-kernel table)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from streamchat_amd import llm as LM, ops  # noqa: E402

HBM_PEAK = 8e12


def weight_bytes(cfg, fp8):
    H, I, dq, dkv = cfg.hidden, cfg.intermediate, cfg.heads * cfg.head_dim, cfg.kv_heads * cfg.head_dim
    rows = cfg.layers * (dq + 2 * dkv + H + 2 * I + H) + cfg.vocab
    elems = cfg.layers * ((dq + 2 * dkv) * H + H * dq + 2 * I * H + H * I) + cfg.vocab * H
    return elems * (1 if fp8 else 2) + (rows * 4 if fp8 else 0)


def leg(lm, ctx, n):
    lm.cache_len = ctx
    g = lm._ab_graph
    g.start(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.run(n)
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def launch_times(lm16, lm8, reps=20):
    """us per launch of each decode projection, fp16 and fp8: one launch per layer captured as a graph, replayed `reps` times"""
    c = lm16.cfg
    dev = lm16.device
    h = torch.randn(c.hidden, device=dev).half()
    m = torch.randn(c.intermediate, device=dev).half()
    shapes = {
        "q (3584 x 3584, norm, f32)": (lambda L, Q: ops.gemv(L["wq"], h, L["bq"], out_f32=True, rms_gamma=L["ln1"], rms_eps=c.eps),
                                       lambda L, Q: ops.gemv_w8(Q["wq"], Q["sq"], h, L["bq"], out_f32=True, rms_gamma=L["ln1"], rms_eps=c.eps)),
        "o (3584 x 3584, res)": (lambda L, Q: ops.gemv(L["wo"], h, None, residual=h), lambda L, Q: ops.gemv_w8(Q["wo"], Q["so"], h, None, residual=h)),
        "gate/up (37888 x 3584, norm, swiglu)": (lambda L, Q: ops.gemv(L["wgu"], h, None, epilogue="swiglu", rms_gamma=L["ln2"], rms_eps=c.eps),
                                                 lambda L, Q: ops.gemv_w8(Q["wgu"], Q["sgu"], h, None, epilogue="swiglu", rms_gamma=L["ln2"], rms_eps=c.eps)),
        "down (3584 x 18944, res)": (lambda L, Q: ops.gemv(L["wd"], m, None, residual=h), lambda L, Q: ops.gemv_w8(Q["wd"], Q["sd"], m, None, residual=h)),
    }
    out = {}
    for name, fns in shapes.items():
        us = []
        for fn in fns:
            body = lambda: [fn(L, Q) for L, Q in zip(lm16.L, lm8.w8["L"])]
            s = torch.cuda.Stream(device=dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                body()
            torch.cuda.current_stream(dev).wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                keep = body()
            g.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / (reps * len(lm16.L)))
            del keep, g
        out[name] = dict(fp16_us=round(us[0], 2), fp8_us=round(us[1], 2), ratio=round(us[0] / us[1], 3))
    return out


def agreement(lm16, lm8, ctx, n):
    """teacher-forced on the fp16 model's greedy tokens: relative rms distance of the logits and top-1 agreement over n tokens"""
    toks, agree, num, den = [1], 0, 0.0, 0.0
    for lm in (lm16, lm8):
        lm.cache_len = ctx
        lm._ab_graph.start(1)
    for i in range(n):
        for lm in (lm16, lm8):
            lm._ab_graph.tok.fill_(toks[-1])
            lm._ab_graph.graph.replay()
        a, b = lm16._ab_graph.logits, lm8._ab_graph.logits
        num += float((a - b).pow(2).sum()); den += float(a.pow(2).sum())
        agree += int(a.argmax()) == int(b.argmax())
        toks.append(int(a.argmax()))
    return dict(tokens=n, logit_rel_rms=round((num / den) ** 0.5, 5), top1_agreement=round(agree / n, 4))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ctx", type=int, default=49152)
    p.add_argument("--tokens", type=int, default=512)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--launches", action="store_true")
    p.add_argument("--agreement", action="store_true")
    a = p.parse_args()
    cfg = LM.Qwen2ConfigLite(**LM.QWEN2_7B)
    lm16 = LM.Qwen2Model(LM.random_qwen2_state_dict(cfg, seed=0), cfg, max_seq=a.ctx + a.tokens + 64, consume=True, decode_weights="fp16")
    lm8 = lm16.shared_view().enable_fp8_decode()
    for lm in (lm16, lm8):
        lm.reset_cache()
        for l in range(cfg.layers):                             # the SAME context for both models (the agreement figures compare their logits)
            lm.cache[l][:a.ctx].normal_(0, 0.5) if lm is lm16 else lm.cache[l][:a.ctx].copy_(lm16.cache[l][:a.ctx])
        lm.cache_len = a.ctx
        lm._ab_graph = LM.DecodeGraph(lm, max_new_tokens=a.tokens + 16)
        lm._ab_graph.start(1)
        lm._ab_graph.capture()
        leg(lm, a.ctx, 16)                                      # warm-up
    rates = {"fp16": [], "fp8": []}
    for _ in range(a.rounds):
        rates["fp16"].append(leg(lm16, a.ctx, a.tokens))
        rates["fp8"].append(leg(lm8, a.ctx, a.tokens))
    kv = cfg.layers * (a.ctx + a.tokens / 2) * 2 * cfg.kv_heads * cfg.head_dim * 2
    out = dict(context=a.ctx, tokens=a.tokens, rounds=a.rounds, build=ops.build_info())
    for k, fp8 in (("fp16", False), ("fp8", True)):
        med = statistics.median(rates[k])
        byt = weight_bytes(cfg, fp8) + kv
        out[k] = dict(tok_per_s=[round(r, 1) for r in rates[k]], median=round(med, 1), weight_gb_per_token=round(weight_bytes(cfg, fp8) / 1e9, 2),
                      gb_per_token=round(byt / 1e9, 2), fraction_of_8tbs=round(med * byt / HBM_PEAK, 3))
    out["fp16_spread"] = round((max(rates["fp16"]) - min(rates["fp16"])) / out["fp16"]["median"], 4)
    out["ratio"] = round(out["fp8"]["median"] / out["fp16"]["median"], 3)
    if a.launches:
        out["launches"] = launch_times(lm16, lm8)
    if a.agreement:
        out["agreement"] = agreement(lm16, lm8, a.ctx, a.tokens)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
