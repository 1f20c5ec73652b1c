#!/usr/bin/env python3
"""The caption prefill phase of the product step alone (what bench.py's `product.caption_prefill_s_per_step` times inside
llm.LlavaQwenForCausalLM.generate_batch_with_image_embedding): llm.BatchDecoder prefills `--chunks` prompts of `--ctx` tokens, one after the
other, into the slices of one per-layer KV cache.  Qwen2-7B random-init.  Runs the phase with the last-layer trim (the default) and with
trim_last_layer=False, interleaved in ONE process on the same weights, and prints one JSON line: seconds per phase of each repetition, the means,
the difference per phase and per prefill, and whether the first logits of the two sides are bit-identical."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from streamchat_amd import llm as LM

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=26)
ap.add_argument("--ctx", type=int, default=22740)
ap.add_argument("--new", type=int, default=128)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
cfg = LM.Qwen2ConfigLite(**LM.QWEN2_7B)
lm = LM.Qwen2Model(LM.random_qwen2_state_dict(cfg, seed=0), cfg, max_seq=4096, consume=True)
g = torch.Generator(device="cuda").manual_seed(1)
prompts = [(torch.randn(a.ctx, cfg.hidden, device="cuda", generator=g) * 0.02).half() for _ in range(a.chunks)]


def phase(trim):
    lm.trim_last_layer = trim
    torch.cuda.synchronize(); t0 = time.perf_counter()
    dec = LM.BatchDecoder(lm, prompts, a.new)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, dec.logits


phase(True); phase(False)                                   # warm-up: activation buffers, rotary tables, cache allocation
times, same = {True: [], False: []}, True
for _ in range(a.reps):
    dt_f, lf = phase(False)
    dt_t, lt = phase(True)
    times[False].append(dt_f); times[True].append(dt_t)
    same = same and torch.equal(lt.view(torch.int32), lf.view(torch.int32))
    del lf, lt
    torch.cuda.empty_cache()
mean = lambda v: sum(v) / len(v)
d = mean(times[False]) - mean(times[True])
print(json.dumps(dict(chunks=a.chunks, ctx=a.ctx, reps=a.reps, every_row_s=[round(t, 4) for t in times[False]], trimmed_s=[round(t, 4) for t in times[True]],
                      every_row_mean_s=round(mean(times[False]), 4), trimmed_mean_s=round(mean(times[True]), 4),
                      every_row_spread_s=round(max(times[False]) - min(times[False]), 4), gain_s_per_phase=round(d, 4),
                      gain_ms_per_prefill=round(1e3 * d / a.chunks, 3), gain_frac=round(d / mean(times[False]), 4), first_logits_bit_identical=same)))
