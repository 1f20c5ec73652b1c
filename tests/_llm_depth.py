"""Shared by tests/test_llm_depth_power.py (CPU) and tests/test_gpu_llm_depth.py: the narrow Qwen2 shape, the references with per-layer taps,
and the contract of tests/test_gpu_heavy_tail.py applied to logits and, layer by layer, to what a KV cache holds.

    rms(candidate - ref) <= 1.5 * rms(hf_fp16_emulation - ref) + 1e-3 * rms(ref)

`ref`: oracle/torch_ref.qwen2_logits in fp64 (narrow shape) or fp32 (full width) on the fp16 weights upcast; `hf_fp16_emulation`: the same
function in fp32 under `storage(torch.float16)`.  (The fp64 pass keeps HF's fp32 inside RMSNorm and the fp32 rotary tables: 1e-7 of a value,
four orders below the bound.)"""
import torch

from oracle import torch_ref as R
from streamchat_amd import llm as LM

# the smallest shape that still takes the production kernels (head dim 128, 128-multiple widths): tests/test_gpu_prefill_trim.py's widths
NARROW = dict(hidden=1024, heads=8, kv_heads=2, head_dim=128, intermediate=2816, vocab=512)
PROMPT, DECODE = 320, 8            # 320 >= 256 rows: rotary GEMM epilogue + last-layer trim; 2.5 q-blocks of 128: the trimmed block starts at row 256
SEED = 7


def narrow_cfg(layers):
    return LM.Qwen2ConfigLite(layers=layers, **NARROW)


def kw_of(cfg, layers=None):
    return dict(heads=cfg.heads, kv_heads=cfg.kv_heads, layers=cfg.layers if layers is None else layers, head_dim=cfg.head_dim,
                theta=cfg.rope_theta, eps=cfg.eps)


class Upcast:
    """a state dict that converts each tensor on lookup: the fp32 / fp64 copy of one weight is alive at a time, never of the whole model"""

    def __init__(self, sd, dtype):
        self.sd, self.dtype = sd, dtype

    def __getitem__(self, k):
        return self.sd[k].to(self.dtype)

    def __contains__(self, k):
        return k in self.sd


class LayersFrom:
    """state-dict view whose layer j is layer first + j of `sd`: qwen2_logits(LayersFrom(sd, l), x, layers=n) runs layers l .. l+n-1 on the
    stream x (every row present, so positions are unchanged), then the final norm and the head"""

    def __init__(self, sd, first):
        self.sd, self.first = sd, first

    def _k(self, k):
        if k.startswith("model.layers."):
            i, rest = k[len("model.layers."):].split(".", 1)
            return f"model.layers.{int(i) + self.first}.{rest}"
        return k

    def __getitem__(self, k):
        return self.sd[self._k(k)]

    def __contains__(self, k):
        return self._k(k) in self.sd


def reference(sd, emb, cfg, dtype):
    """(logits, taps) of the truth in `dtype` and of the fp16-storage emulation in fp32, on the device of `sd`"""
    with torch.no_grad():
        t_ref, t_emu = [], []
        ref = R.qwen2_logits(Upcast(sd, dtype), emb.to(dtype), taps=t_ref, **kw_of(cfg))
        with R.storage(torch.float16):
            emu = R.qwen2_logits(Upcast(sd, torch.float32), emb.float(), taps=t_emu, **kw_of(cfg))
    return (ref, t_ref), (emu, t_emu)


def _rms_rows(t):
    return t.pow(2).mean(-1).sqrt()


def contract(cand, ref, emu, per_row=False):
    """(error, bound), both relative to rms(ref); finite error <= bound passes.  per_row: one figure per row ([rows] tensors), else over all rows."""
    cand, ref, emu = cand.double(), ref.double().to(cand.device), emu.double().to(cand.device)
    if per_row:
        r = _rms_rows(ref)
        return _rms_rows(cand - ref) / r, 1.5 * _rms_rows(emu - ref) / r + 1e-3
    r = ref.pow(2).mean().sqrt()
    return ((cand - ref).pow(2).mean().sqrt() / r).item(), (1.5 * (emu - ref).pow(2).mean().sqrt() / r + 1e-3).item()


def passes(err, bound):
    return bool(err == err and err != float("inf") and err <= bound)


def kv_of(tap):
    """(K | V) rows of one layer's tap: the layout of Qwen2Model.cache[l]"""
    return torch.cat([tap[0], tap[1]], dim=-1)


def stream_of(tap):
    return tap[2]


def layer_curve(cand, taps_ref, taps_emu, pick=kv_of):
    """per layer (error, bound, emulation's error) of what a candidate holds for that layer - `cand`: one tensor per layer, [rows, 2*dkv] K | V
    rows with pick=kv_of, [rows, H] residual streams with pick=stream_of; a layer the candidate has nothing for fails (error inf)"""
    out = []
    for l, (tr, te) in enumerate(zip(taps_ref, taps_emu)):
        ref, emu = pick(tr), pick(te)
        e_emu, b = contract(emu, ref, emu)
        e = contract(cand[l].to(ref.device), ref, emu)[0] if l < len(cand) and cand[l] is not None else float("inf")
        out.append((e, b, e_emu))
    return out


def first_failing(curve):
    return next((l for l, (e, b, _) in enumerate(curve) if not passes(e, b)), None)


def format_curve(curve, name="candidate"):
    return "\n".join([f"layer  {name:>10}  emulation      bound"] + [f"{l:5d}  {e:10.3e}  {h:9.3e}  {b:9.3e}" for l, (e, b, h) in enumerate(curve)])
