"""CPU: the contract tests/test_gpu_llm_depth.py applies at the narrow shape can tell a wrong 28-layer stack from a right one.

The candidate is the reference alone: oracle/torch_ref.qwen2_logits under `storage(torch.float16)` (HF's fp16 storage points) against the same
function in fp64, 320 tokens, seed 7, tests/_llm_depth.py's shape.  Unchanged it has to PASS

    rms(candidate - ref) <= 1.5 * rms(emulation - ref) + 1e-3 * rms(ref)

on the logits and on every layer's K | V.  A MUTANT is that emulation with one change of the kind a per-layer loop can get wrong; with L layers
it sits at layer m = L // 2 (14 of 28; at 2 layers that is layer 1, which is also the last):

  norm from the layer before   layer m uses layer m-1's post_attention_layernorm.weight
  last layer skipped           the stack stops after L-1 layers
  K/V projections swapped      layers m-1 and m swap k_proj / v_proj (a cache row written to the neighbouring layer)
  MLP residual = block input   in layer m the MLP adds to the block's input, not to the post-attention stream (an h / h2 mix-up)
  layers >= 2 project K/V as layer 1   every layer from the third on uses layer 1's k_proj / v_proj (a per-layer index that stops at 1): it has
                                       no 2-layer form, like every fault that needs a layer that is neither the first nor the last

Each mutant must FAIL the logits contract, and the per-layer check must point at it: the first layer whose residual stream fails is the mutated
one, and the first layer whose K | V fails - the only per-layer state a GPU test can read, Qwen2Model.cache - is the mutated layer for a fault
on the K / V side and the NEXT layer for a fault in the MLP half (a layer's K / V are projected before its MLP runs; behind the last layer
only the logits see it).  A mutant below the bound is listed as such in the table, never dropped.

`python -m tests.test_llm_depth_power` prints the table and rewrites tests/LLM_DEPTH_POWER.md with it."""
import os
import time

import pytest
import torch

from oracle import torch_ref as R
from streamchat_amd import llm as LM
from tests import _llm_depth as D

_PRE = "model.layers.{}."
_KV = ["self_attn.k_proj.weight", "self_attn.k_proj.bias", "self_attn.v_proj.weight", "self_attn.v_proj.bias"]


def _resume(sd, cfg, x, first, n):
    """layers first .. first+n-1, final norm and head on the stream x, at the emulation's storage points -> (logits, taps)"""
    taps = []
    with torch.no_grad(), R.storage(torch.float16):
        return R.qwen2_logits(D.LayersFrom(D.Upcast(sd, torch.float32), first), x, taps=taps, **D.kw_of(cfg, n)), taps


def _norm_from_the_layer_before(S, m):
    sd = dict(S.sd)
    sd[_PRE.format(m) + "post_attention_layernorm.weight"] = S.sd[_PRE.format(m - 1) + "post_attention_layernorm.weight"]
    logits, taps = _resume(sd, S.cfg, S.stream(m), m, S.layers - m)
    return logits, S.t_emu[:m] + taps


def _last_layer_skipped(S, m):
    logits, _ = _resume(S.sd, S.cfg, S.stream(S.layers - 1), S.layers - 1, 0)
    return logits, S.t_emu[:S.layers - 1]


def _kv_projections_swapped(S, m):
    sd = dict(S.sd)
    for n in _KV:
        sd[_PRE.format(m - 1) + n], sd[_PRE.format(m) + n] = S.sd[_PRE.format(m) + n], S.sd[_PRE.format(m - 1) + n]
    logits, taps = _resume(sd, S.cfg, S.stream(m - 1), m - 1, S.layers - m + 1)
    return logits, S.t_emu[:m - 1] + taps


def _mlp_residual_is_block_input(S, m):
    x_in = S.stream(m)
    k, v, x_out = S.t_emu[m]
    sd = dict(S.sd)
    sd[_PRE.format(m) + "mlp.down_proj.weight"] = torch.zeros_like(S.sd[_PRE.format(m) + "mlp.down_proj.weight"])
    x_mid = _resume(sd, S.cfg, x_in, m, 1)[1][0][2]                    # no MLP output: the post-attention stream
    x_bad = (x_in + (x_out - x_mid)).half().float()                    # the MLP's output added to the block input
    logits, taps = _resume(S.sd, S.cfg, x_bad, m + 1, S.layers - m - 1)
    return logits, S.t_emu[:m] + [(k, v, x_bad)] + taps


def _later_layers_project_kv_as_layer_1(S, m):
    sd = dict(S.sd)
    for l in range(2, S.layers):
        for n in _KV:
            sd[_PRE.format(l) + n] = S.sd[_PRE.format(1) + n]
    logits, taps = _resume(sd, S.cfg, S.stream(2), 2, S.layers - 2)
    return logits, S.t_emu[:2] + taps


# name -> (build, mutated layer, first layer whose K | V can differ (None: none does), expressible with L layers)
MUTANTS = {
    "norm from the layer before": (_norm_from_the_layer_before, lambda L, m: m, lambda L, m: m + 1 if m + 1 < L else None, lambda L: L >= 2),
    "last layer skipped": (_last_layer_skipped, lambda L, m: L - 1, lambda L, m: L - 1, lambda L: L >= 2),
    "K/V projections swapped": (_kv_projections_swapped, lambda L, m: m - 1, lambda L, m: m - 1, lambda L: L >= 2),
    "MLP residual = block input": (_mlp_residual_is_block_input, lambda L, m: m, lambda L, m: m + 1 if m + 1 < L else None, lambda L: L >= 2),
    "layers >= 2 project K/V as layer 1": (_later_layers_project_kv_as_layer_1, lambda L, m: 2, lambda L, m: 2, lambda L: L >= 3),
}
LAYERS = (28, 2)


class _Stack:
    def __init__(self, layers):
        self.layers, self.cfg = layers, D.narrow_cfg(layers)
        self.sd = LM.random_qwen2_state_dict(self.cfg, seed=D.SEED, device="cpu")
        ids = torch.randint(0, self.cfg.vocab, (D.PROMPT,), generator=torch.Generator().manual_seed(D.SEED))
        self.emb = self.sd["model.embed_tokens.weight"][ids]
        (self.ref, self.t_ref), (self.emu, self.t_emu) = D.reference(self.sd, self.emb, self.cfg, torch.float64)

    def stream(self, l):
        """the emulation's residual stream in front of layer l"""
        return self.emb.float() if l == 0 else self.t_emu[l - 1][2]


_STACKS, _TABLE = {}, {}


def _stack(layers):
    if layers not in _STACKS:
        _STACKS[layers] = _Stack(layers)
    return _STACKS[layers]


def _judge(S, logits, taps):
    """-> (logits error / bound, first layer whose K | V fails, first layer whose residual stream fails)"""
    e, b = D.contract(logits, S.ref, S.emu)
    kv = D.first_failing(D.layer_curve([D.kv_of(t) for t in taps], S.t_ref, S.t_emu))
    st = D.first_failing(D.layer_curve([D.stream_of(t) for t in taps], S.t_ref, S.t_emu, D.stream_of))
    return e / b, kv, st


def _measure(layers, name):
    S = _stack(layers)
    build, where, where_kv, expressible = MUTANTS[name]
    if not expressible(layers):
        return None
    m = layers // 2
    ratio, kv, st = _judge(S, *build(S, m))
    return dict(ratio=ratio, kv=kv, stream=st, want_kv=where_kv(layers, m), want_stream=where(layers, m))


@pytest.mark.parametrize("layers", LAYERS)
def test_the_emulation_itself_passes(layers):
    S = _stack(layers)
    e, b = D.contract(S.emu, S.ref, S.emu)
    ratio, kv, st = _judge(S, S.emu, S.t_emu)
    _TABLE[(layers, "emulation")] = dict(ratio=ratio, kv=kv, stream=st, err=e)
    print(f"\n[depth power] {layers} layers: emulation's own error {e:.3e} of rms(ref), bound {b:.3e}")
    er, br = D.contract(S.emu, S.ref, S.emu, per_row=True)
    assert ratio < 1 and kv is None and st is None and bool((er <= br).all())
    assert torch.isfinite(S.ref).all() and 1e-4 < e < 1e-2                # fp16 storage really costs something, and not the format


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_is_caught_at_28_layers_and_located(name):
    r = _measure(28, name)
    _TABLE[(28, name)] = r
    print(f"\n[depth power] 28 layers, {name}: logits error / bound {r['ratio']:.3g}, first failing layer K|V {r['kv']}, stream {r['stream']}")
    assert r["ratio"] > 1, f"'{name}' passes the logits contract at 28 layers ({r['ratio']:.3g} of the bound)"
    assert r["stream"] == r["want_stream"] and r["kv"] == r["want_kv"], r


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_at_2_layers_is_recorded(name):
    """what a 2-layer suite sees of the same faults: measured and written to the table; a mutant with no 2-layer form is recorded as such"""
    r = _measure(2, name)
    _TABLE[(2, name)] = r
    if r is None:
        assert name == "layers >= 2 project K/V as layer 1"
        return
    print(f"\n[depth power] 2 layers, {name}: logits error / bound {r['ratio']:.3g}, first failing layer K|V {r['kv']}, stream {r['stream']}")
    assert r["stream"] == r["want_stream"] and r["kv"] == r["want_kv"], r


def _cell(r, mutant=True):
    if r is None:
        return "- | - | -"
    f = lambda v: "none" if v is None else str(v)
    return f"{r['ratio']:.3g}" + ("" if r["ratio"] > 1 or not mutant else " below the bound") + f" | {f(r['kv'])} | {f(r['stream'])}"


def _markdown():
    lines = ["# What the depth contract can tell apart", "",
             "Written by `python -m tests.test_llm_depth_power`; do not edit.  Narrow Qwen2 shape of `tests/_llm_depth.py`, 320 tokens, seed 7, CPU.  Candidate:",
             "`oracle/torch_ref.qwen2_logits` under `storage(torch.float16)` with one change; reference: the same function in fp64.  *error / bound*:",
             "`rms(candidate - ref) / (1.5 rms(emulation - ref) + 1e-3 rms(ref))` over all 320 logit rows - a value above 1 fails the check.  *first K|V* /",
             "*first stream*: the first layer whose K | V (what `Qwen2Model.cache` holds) / whose residual stream fails the same contract, `none`: no layer does.",
             "With L layers a mutant sits at layer L // 2 (14 of 28; at 2 layers that is layer 1, also the last one); `-`: the mutant has no form with that many",
             "layers.  A fault in a layer's MLP half shows in the NEXT layer's K | V (a layer's K / V are projected before its MLP runs) - at 2 layers there is no",
             "next layer, so only the logits see it.", "",
             "| candidate | 28 layers: error / bound | first K\\|V | first stream | 2 layers: error / bound | first K\\|V | first stream |", "|---|---|---|---|---|---|---|"]
    for name in ["emulation"] + list(MUTANTS):
        lines.append(f"| {name} | {_cell(_TABLE[(28, name)], name != 'emulation')} | {_cell(_TABLE[(2, name)], name != 'emulation')} |")
    lines += ["", "The emulation's own error, relative to rms(ref): " + ", ".join(f"{_TABLE[(L, 'emulation')]['err']:.3e} at {L} layers" for L in LAYERS) + "."]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    t0 = time.time()
    for L in LAYERS:
        S = _stack(L)
        e, _ = D.contract(S.emu, S.ref, S.emu)
        ratio, kv, st = _judge(S, S.emu, S.t_emu)
        _TABLE[(L, "emulation")] = dict(ratio=ratio, kv=kv, stream=st, err=e)
        for name in MUTANTS:
            _TABLE[(L, name)] = _measure(L, name)
    text = _markdown()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "LLM_DEPTH_POWER.md"), "w") as f:
        f.write(text)
    print(text)
    print(f"{time.time() - t0:.1f} s")
