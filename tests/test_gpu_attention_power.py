"""GPU: ops.attention at the production call signatures against the fp64 probe-row reference of tests/_attn_cases.py, every input family that
applies, with the per-row check (4e-3 of max|ref_row| and a row cosine of 0.9999: tests/_tol.py's constants per probe row and head).
tests/test_attention_case_power.py shows on the CPU what these cases can tell apart; tests/ATTENTION_POWER.md holds its table.
Shapes, strides and split factors come from the production code (llm.decode_nsplit, Qwen2Model.forward's and BatchDecoder.prepare_steps' own
formulas, llm.KV_ROW_PAD): see _attn_cases.cases()."""
import pytest
import torch

from streamchat_amd import llm as LM
from streamchat_amd import ops
from tests import _attn_cases as A

pytestmark = pytest.mark.gpu

_CASES = A.cases()


def _cache_of(k, v, pad):
    """one cache tensor per layer as Qwen2Model.reset_cache lays it out: rows of [K of all KV heads | V of all KV heads] + `pad` halves"""
    S, w = k.shape[1], k.shape[2]
    cache = torch.empty((S, 2 * w + pad), dtype=torch.float16, device=k.device)[:, :2 * w]
    cache[:, :w], cache[:, w:] = k[0], v[0]
    return cache


def _call(c, inp):
    """the production call of this case's layout -> [B, Sq, Hq, Dh] output"""
    Hq, Hkv, Dh, G, dq, dkv = c.Hq, c.Hkv, c.Dh, c.G, c.Hq * c.Dh, c.Hkv * c.Dh
    dev = inp.k.device
    kl = None if c.kv_len is None else torch.tensor(c.kv_len, dtype=torch.int32, device=dev)
    if c.layout in ("dense", "cache"):                     # Qwen2Model.forward: q rows of a buffer, K / V column windows of ONE padded cache tensor
        ck = _cache_of(inp.k, inp.v, LM.KV_ROW_PAD)
        assert c.causal                                     # (a causal call runs k_attn, split-KV included, whatever sc_attention_variant says for Sq = 1)
        out = ops.attention(inp.q[0].unsqueeze(0), ck[:, :dkv].unsqueeze(0), ck[:, dkv:].unsqueeze(0), Hq, Hkv, Dh, Dh ** -0.5, causal=True,
                            nsplit=c.nsplit, q_prescaled=True)
    elif c.layout == "packed":                             # DecodeGraph: G query heads of a KV group as G query rows, kv_len on the device, capacity beyond it
        ck = _cache_of(inp.k, inp.v, LM.KV_ROW_PAD)
        q = inp.q.reshape(1, dq)
        ws = torch.empty(max(ops.attention_workspace_bytes(1, Hkv, G, c.nsplit, Dh), 256), dtype=torch.uint8, device=dev)
        out = ops.attention(q.as_strided((1, G, Dh), (dq, Dh, 1)), ck[:, :dkv].unsqueeze(0), ck[:, dkv:].unsqueeze(0), Hkv, Hkv, Dh, Dh ** -0.5, causal=False,
                            kv_len=kl, nsplit=c.nsplit, q_head_stride=G * Dh, o_head_stride=G * Dh, out_ld=Dh, ws=ws, q_prescaled=True)
    elif c.layout == "packed_batched":                     # BatchDecoder.step: one dense cache [B, cap, K | V], q / out batch strides
        ck = torch.cat([inp.k, inp.v], dim=2)
        q = inp.q.reshape(c.B, dq)
        ws = torch.empty(max(ops.attention_workspace_bytes(c.B, Hkv, G, c.nsplit, Dh), 256), dtype=torch.uint8, device=dev)
        out = ops.attention(q.as_strided((c.B, G, Dh), (dq, Dh, 1)), ck[:, :, :dkv], ck[:, :, dkv:], Hkv, Hkv, Dh, Dh ** -0.5, causal=False,
                            kv_len=kl, nsplit=c.nsplit, q_head_stride=G * Dh, o_head_stride=G * Dh, out_ld=Dh, ws=ws, q_prescaled=True)
    else:                                                  # vision.py / text.py: q | k | v thirds of one fused projection output
        qkv = torch.cat([inp.q, inp.k, inp.v], dim=2)
        D = dq
        out = ops.attention(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], Hq, Hkv, Dh, Dh ** -0.5, causal=c.causal, kv_len=kl, q_prescaled=c.prescaled)
    torch.cuda.synchronize()
    return out.reshape(c.B, c.Sq, Hq, Dh)


@pytest.mark.parametrize("case", _CASES, ids=[c.name.replace(" ", "_") for c in _CASES])
def test_attention_production_call(case):
    c = case
    if c.variant is not None:
        packed = c.layout.startswith("packed")
        assert ops.attention_variant(c.Dh, c.G if packed else c.Sq, c.nsplit) == c.variant
    base = A.Base(c, "cuda")
    worst, failed = {}, []
    try:
        for fam in c.families:
            inp = base.make(fam, full_q=True)
            out = _call(c, inp)
            got = torch.stack([out[b, i] for b, i in c.rows])
            ratio, cos = A.check(got, A.REFERENCE(inp))
            worst[fam] = float(ratio.max())
            msg = A.describe_worst(inp, ratio, cos)
            print(f"\n[attn] {msg}")
            if bool(A.failures(ratio, cos).any()):
                failed.append(msg)
            base.restore()
            del inp, out, got
    finally:
        del base
        torch.cuda.empty_cache()
    print(f"\n[attn] {c.name}: worst ratio per family " + ", ".join(f"{f} {r:.3g}" for f, r in worst.items()))
    assert not failed, "\n".join(failed)
