#!/usr/bin/env python3
"""A/B of the batch-1 answer decode from fp16 and from FP8 (e4m3) weights (llm.Qwen2Model.enable_fp8_decode), in ONE process.

Random-init Qwen2-7B, a 49 k-token context in the KV cache (filled with N(0, 0.5^2) rows as tools/bench_decode.py does: the decode kernels' time
does not depend on the values), 512 tokens per leg through DecodeGraph, the fp16 and fp8 legs interleaved for --rounds rounds.  Prints one JSON
line: tok/s per leg (every round + median), the fp16 legs' own spread, weight / total bytes per token and the fraction of 8 TB/s they amount to,
and - `--launches` - the time of every decode projection launch in both formats (a captured graph of one launch per layer, so the weights of 28
layers cycle through and nothing is served from the cache), and - `--agreement` - the fp8-vs-fp16 logit distance and top-1 agreement over
the tokens of the fp16 answer (teacher-forced: both models are fed the fp16 model's tokens).

`--kv_cache` adds the FP8 (e4m3) KV-cache legs (llm.Qwen2Model(kv_cache="fp8")): fp16/fp8-kv and fp8-w/fp8-kv run interleaved with the two fp16-kv legs in
the same rounds (their caches hold the quantised form of the same context), bytes per token count the cache's bytes and scales, `--launches`
adds the attention + combine and the quantise launches of both cache formats (the split-KV kernel and the merge are ONE library call: the
kernel trace below splits them), `--agreement` compares every leg with the fp16 / fp16 one.  `--kv_pads 0,64,256` and `--nsplits 32,128` add
fp8-w / fp8-kv legs whose byte rows carry that pad (bytes) or whose graph takes that split-KV factor, interleaved with the others.

    python tools/decode_w8_ab.py [--ctx 49152] [--tokens 512] [--rounds 3] [--launches] [--agreement] [--kv_cache [--kv_pads B,..] [--nsplits N,..]]
    rocprofv3 --kernel-trace --stats -- python tools/decode_w8_ab.py --rounds 1        (the per-kernel table: k_attn_kv8, k_attn_combine, ...)"""
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


def kv_launch_times(lm16, lmk, ctx, variants, reps=20):
    """us per launch and layer: the decode attention (split-KV kernel + merge) over the fp16 and over the fp8 cache, and the fp8 cache's row
    quantiser; `variants` {name: (model, nsplit)}: the same fp8 pair over caches of another row pad or with another split-KV factor"""
    c, dev = lm16.cfg, lm16.device
    q = torch.randn(1, c.heads * c.head_dim, device=dev).half()
    nsplit = LM.decode_nsplit(c.head_dim, ctx)
    nmax = max([nsplit] + [n for _, n in variants.values()])
    klen = torch.tensor([ctx + 1], dtype=torch.int32, device=dev)
    row = torch.tensor([ctx], dtype=torch.int32, device=dev)
    ws = torch.empty(max(ops.attention_workspace_bytes(1, c.kv_heads, c.heads // c.kv_heads, nmax, c.head_dim), 256), dtype=torch.uint8, device=dev)
    G, Dh = c.heads // c.kv_heads, c.head_dim
    kv8 = lambda m, ns: [ops.attention_kv8(q.as_strided((1, G, Dh), (c.heads * Dh, Dh, 1)), *m.kv8[l], c.kv_heads, Dh, Dh ** -0.5, kv_len=klen, nsplit=ns,
                                           q_head_stride=G * Dh, o_head_stride=G * Dh, out_ld=Dh, ws=ws, q_prescaled=True) for l in range(c.layers)]
    bodies = {
        "attention + combine, fp16 cache": lambda: [lm16._decode_attention(q, lm16.cache[l], nsplit, kv_len=klen, ws=ws) for l in range(c.layers)],
        "attention + combine, fp8 cache": lambda: kv8(lmk, nsplit),
        "quantise one row, fp8 cache": lambda: [ops.kv8_quantize_rows(lmk._kv_stage, *lmk.kv8[l], row, c.kv_heads, Dh, x_follows_row=True) for l in range(c.layers)],
    }
    for name, (m, ns) in variants.items():
        bodies["attention + combine, " + name] = lambda m=m, ns=ns: kv8(m, ns)
    out = {}
    for name, body in bodies.items():
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
        out[name] = round(e0.elapsed_time(e1) * 1e3 / (reps * c.layers), 2)
        del keep, g
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
    p.add_argument("--kv_cache", action="store_true", help="add the fp8 KV-cache legs (fp16 and fp8 weights)")
    p.add_argument("--kv_pads", default="", help="with --kv_cache: more fp8-w / fp8-kv legs, their byte rows padded by these many bytes (comma list)")
    p.add_argument("--nsplits", default="", help="with --kv_cache: more fp8-w / fp8-kv legs with these split-KV factors (comma list)")
    a = p.parse_args()
    cfg = LM.Qwen2ConfigLite(**LM.QWEN2_7B)
    lm16 = LM.Qwen2Model(LM.random_qwen2_state_dict(cfg, seed=0), cfg, max_seq=a.ctx + a.tokens + 64, consume=True, decode_weights="fp16")
    lm8 = lm16.shared_view().enable_fp8_decode()
    legs = {"fp16": lm16, "fp8": lm8}
    if a.kv_cache:
        legs["fp16_kv8"] = lm16.shared_view().set_kv_cache("fp8")
        legs["fp8_kv8"] = lm8.shared_view().set_kv_cache("fp8")
    pads, splits = {}, {}
    if a.kv_cache:
        for b in filter(None, a.kv_pads.split(",")):
            pads["fp8_kv8_pad%d" % int(b)] = int(b)
        for n in filter(None, a.nsplits.split(",")):
            splits["fp8_kv8_nsplit%d" % int(n)] = int(n)
        for k in list(pads) + list(splits):
            legs[k] = lm8.shared_view().set_kv_cache("fp8")
    pad0 = LM.KV_ROW_PAD
    for k, lm in legs.items():
        LM.KV_ROW_PAD = pads[k] // 2 if k in pads else pad0       # (reset_cache reads it: halves of the fp16 rows, twice that in bytes for the fp8 rows)
        lm.reset_cache()
        LM.KV_ROW_PAD = pad0
        for l in range(cfg.layers):                             # the SAME context for every model (the agreement figures compare their logits)
            if lm is lm16:
                lm.cache[l][:a.ctx].normal_(0, 0.5)
            elif lm.kv_cache == "fp8":                          # ... in its quantised form
                ops.kv8_quantize_rows(lm16.cache[l][:a.ctx], *lm.kv8[l], 0, cfg.kv_heads, cfg.head_dim)
            else:
                lm.cache[l][:a.ctx].copy_(lm16.cache[l][:a.ctx])
        lm.cache_len = a.ctx
        lm._ab_graph = LM.DecodeGraph(lm, max_new_tokens=a.tokens + 16, nsplit=splits.get(k))
        lm._ab_graph.start(1)
        lm._ab_graph.capture()
        leg(lm, a.ctx, 16)                                      # warm-up
    rates = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, lm in legs.items():
            rates[k].append(leg(lm, a.ctx, a.tokens))
    seg = 2 * cfg.kv_heads                                       # fp8 cache: one byte per element + one fp32 scale per 128-element segment
    kv_row = {False: seg * cfg.head_dim * 2, True: seg * cfg.head_dim + seg * 4}
    out = dict(context=a.ctx, tokens=a.tokens, rounds=a.rounds, build=ops.build_info())
    for k, lm in legs.items():
        fp8 = lm.w8 is not None
        med = statistics.median(rates[k])
        byt = weight_bytes(cfg, fp8) + cfg.layers * (a.ctx + a.tokens / 2) * kv_row[lm.kv_cache == "fp8"]
        out[k] = dict(tok_per_s=[round(r, 1) for r in rates[k]], median=round(med, 1), weight_gb_per_token=round(weight_bytes(cfg, fp8) / 1e9, 2),
                      gb_per_token=round(byt / 1e9, 2), fraction_of_8tbs=round(med * byt / HBM_PEAK, 3))
    out["fp16_spread"] = round((max(rates["fp16"]) - min(rates["fp16"])) / out["fp16"]["median"], 4)
    out["ratio"] = round(out["fp8"]["median"] / out["fp16"]["median"], 3)
    for k in ("fp16_kv8", "fp8_kv8"):
        if k in legs:
            out[k]["ratio_to_fp16_cache"] = round(out[k]["median"] / out[k[:-4]]["median"], 3)
    for k in list(pads) + list(splits):
        out[k].update(row_stride_bytes=legs[k].kv8[0][0].stride(0), nsplit=legs[k]._ab_graph.nsplit, ratio_to_fp8_kv8=round(out[k]["median"] / out["fp8_kv8"]["median"], 4))
    if a.launches:
        out["launches"] = launch_times(lm16, lm8)
        if a.kv_cache:
            out["kv_launches_us"] = kv_launch_times(lm16, legs["fp16_kv8"], a.ctx, {k: (legs[k], legs[k]._ab_graph.nsplit) for k in list(pads) + list(splits)})
    if a.agreement:
        out["agreement"] = agreement(lm16, lm8, a.ctx, a.tokens)
        for k in ("fp16_kv8", "fp8_kv8"):
            if k in legs:
                out["agreement_" + k] = agreement(lm16, legs[k], a.ctx, a.tokens)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
