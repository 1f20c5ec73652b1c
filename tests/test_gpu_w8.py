"""GPU: FP8 (OCP e4m3fn) weight-only decode (include/streamchat_hip_w8.h, gemv_w8.hip, llm.Qwen2Model.enable_fp8_decode).

The quantiser is pinned bit for bit to its torch CPU specification.  The GEMV is pinned against fp64 on the DEQUANTISED weights with
assert_close_fp16 at its defaults - the fp16 GEMV's own contract: e4m3 x fp16 products are exact in fp32, only the summation order differs,
so the fp8 kernel is owed no slack (tests/test_w8_power.py: the same check on the same inputs rejects fnuz decoding and a neighbour's scale).
The model tests use fp8-EXACT weights (tests/_w8.fp8_exact_matrix), for which the fp8 model is mathematically the fp16 model."""
import json
import os
import subprocess
import sys

import pytest
import torch

from oracle import torch_ref as R
from streamchat_amd import llm as LM, ops
from tests import _w8
from tests._tol import assert_close_fp16

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cuda(c):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


# ---- quantiser -----------------------------------------------------------------------------------------------------------------------------
def _quant_inputs():
    g = _w8.gen(11)
    gauss = (torch.randn(37, 1040, generator=g) * 0.02).half()
    zero_row = gauss[:6, :64].clone(); zero_row[2] = 0; zero_row[4, 5] = -0.0
    extreme = (torch.randn(9, 256, generator=g)).half()
    extreme[0, 3], extreme[1, 7], extreme[2, 0], extreme[2, 1] = 65504, -65504, 65504, -65504
    extreme[3] = (torch.randint(-1023, 1024, (256,), generator=g).float() * 2.0 ** -24).half()          # a row of fp16 subnormals only
    extreme[4, :16] = torch.tensor([2.0 ** -24, -2.0 ** -24] * 8).half()                                # subnormals beside ordinary values
    exact, codes, e = _w8.fp8_exact_matrix(12, 320, seed=5)
    return dict(gauss=gauss, zero_row=zero_row, extreme=extreme, exact=exact), codes, e


def test_quantiser_is_bit_identical_to_the_torch_cpu_expression():
    mats, codes, e = _quant_inputs()
    for name, w in mats.items():
        q, s = ops.quantize_rows_e4m3(w.cuda())
        qr, sr = _w8.quantize_ref(w)
        assert torch.equal(_bits(s).cpu(), _bits(sr)), name
        assert torch.equal(q.cpu(), qr), (name, int((q.cpu() != qr).sum()))
    q, s = ops.quantize_rows_e4m3(mats["exact"].cuda())
    assert torch.equal(q.cpu(), codes) and torch.equal(s.cpu(), torch.exp2(e.float()))      # scales exactly 2^e_n, the codes unchanged
    assert int(ops.quantize_rows_e4m3(mats["zero_row"].cuda())[0][4, 5]) == 0x80            # the sign of zero is kept
    wide = torch.full((37, 1040 + 40), float("nan"), dtype=torch.float16)
    wide[:, 8:1048] = mats["gauss"]
    q, s = ops.quantize_rows_e4m3(wide.cuda()[:, 8:1048])                                   # a row-strided view
    qr, sr = _w8.quantize_ref(mats["gauss"])
    assert torch.equal(q.cpu(), qr) and torch.equal(_bits(s).cpu(), _bits(sr))


# ---- GEMV ----------------------------------------------------------------------------------------------------------------------------------
GEMV_CASES = [                                                    # the smallest shapes that reach each code path of sc_gemv_w8_f16
    dict(N=5, K=16),                                              # a single slice, one lane of each half-wave
    dict(N=1, K=48, bias=True),
    dict(N=37, K=1040, bias=True, res=True),                      # two full slices + a tail of 16
    dict(N=37, K=1040, norm=True, bias=True),
    dict(N=50, K=3584, res=True),                                 # the 7B straight-line paths (7 and 37 slices), one row per half-wave
    dict(N=50, K=3584, norm=True, bias=True),
    dict(N=50, K=18944, res=True),
    dict(N=50, K=18944, norm=True),
    dict(N=16500, K=48, bias=True),                               # the many-rows dispatch (four rows per half-wave): loop kernel
    dict(N=16500, K=3584, norm=True),                             # ... and straight-line (the lm_head call)
    dict(N=4, K=1040, swiglu=True),
    dict(N=36, K=1040, swiglu=True, norm=True),
    dict(N=36, K=3584, swiglu=True, norm=True),                   # the gate / up call
]


@pytest.mark.parametrize("kw", GEMV_CASES, ids=lambda k: "-".join(f"{a}{b}" if a in "NK" else a for a, b in k.items()))
def test_gemv_w8_against_fp64_on_the_dequantised_weights(kw):
    c = _cuda(_w8.gemv_case(**kw))
    epi = "swiglu" if kw.get("swiglu") else "none"
    for f32 in ((False,) if kw.get("swiglu") else (False, True)):
        y = ops.gemv_w8(c["q"], c["scale"], c["x"], c["bias"], c["res"], epilogue=epi, out_f32=f32, rms_gamma=c["gamma"], rms_eps=1e-6)
        assert y.dtype == (torch.float32 if f32 else torch.float16)
        assert_close_fp16(y, c["ref"], what=f"gemv_w8 {kw} f32={f32}")
    if not kw.get("swiglu") and kw["N"] <= 50:                       # a dynamic output row of a padded cache view
        N = kw["N"]
        cache = torch.full((6, N + 64), 7.0, dtype=torch.float16, device="cuda")[:, :N]
        ops.gemv_w8(c["q"], c["scale"], c["x"], c["bias"], c["res"], out=cache, out_row=torch.tensor([4], dtype=torch.int32, device="cuda"),
                    rms_gamma=c["gamma"], rms_eps=1e-6)
        assert_close_fp16(cache[4], c["ref"], what=f"gemv_w8 {kw} dynamic row")
        assert bool((cache[:4] == 7.0).all()) and bool((cache[5] == 7.0).all())


def test_result_bits_do_not_depend_on_waves_per_workgroup():
    """two child processes with different SC_GEMV_WPB_* values: identical output bytes (GEMV shapes of every dispatch + the fused q|k|v)"""
    out = []
    for knobs in ({}, {"SC_GEMV_WPB_0": "3", "SC_GEMV_WPB_1": "2", "SC_GEMV_WPB_2": "5", "SC_GEMV_WPB_3": "8"}):
        env = {k: v for k, v in os.environ.items() if not k.startswith("SC_GEMV_")}
        env.update(knobs)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_w8_child.py"), "wpb"], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out.append([l for l in r.stdout.splitlines() if l.startswith("W8SHA")][0])
    assert out[0] == out[1]


@pytest.mark.parametrize("Hq,Hkv,Dh,K", [(4, 2, 64, 256), (28, 4, 128, 3584)])
def test_decode_qkv_tab_w8_is_bitwise_gemv_w8_plus_rope(Hq, Hkv, Dh, K):
    pos, dq, dkv = 9, Hq * Dh, Hkv * Dh
    c = _cuda(_w8.gemv_case(dq + 2 * dkv, K, seed=7, norm=True, bias=True))
    wq, sq, wkv, skv, bq, bkv = c["q"][:dq], c["scale"][:dq], c["q"][dq:], c["scale"][dq:], c["bias"][:dq].contiguous(), c["bias"][dq:].contiguous()
    tq, tk = ops.rope_table(64, Dh, 1e6, Dh ** -0.5 * ops.LOG2E, "cuda:0"), ops.rope_table(64, Dh, 1e6, 1.0, "cuda:0")
    row = torch.tensor([pos], device="cuda", dtype=torch.int32)
    q_out = torch.zeros(dq, dtype=torch.float16, device="cuda")
    cache = torch.zeros((16, 2 * dkv + LM.KV_ROW_PAD), dtype=torch.float16, device="cuda")[:, :2 * dkv]
    ops.decode_qkv_tab_w8(wq, sq, wkv, skv, bq, bkv, c["x"], c["gamma"], 1e-6, q_out, cache, row, Hq, Hkv, Dh, tq, tk)
    q32 = ops.gemv_w8(wq, sq, c["x"], bq, out_f32=True, rms_gamma=c["gamma"], rms_eps=1e-6).view(1, -1)
    kv32 = ops.gemv_w8(wkv, skv, c["x"], bkv, out_f32=True, rms_gamma=c["gamma"], rms_eps=1e-6).view(1, -1)
    assert_close_fp16(torch.cat([q32, kv32], 1)[0], c["ref"], what="q | k | v sums")
    q_b = ops.rope_f32in(q32, tq, Hq, Dh, torch.empty((1, dq), dtype=torch.float16, device="cuda"), 0, pos)
    want = torch.zeros((16, 2 * dkv), dtype=torch.float16, device="cuda")
    ops.rope_f32in(kv32, tk, Hkv, Dh, want[pos:pos + 1], dkv, pos)
    assert torch.equal(_bits(q_out), _bits(q_b.view(-1))) and torch.equal(_bits(cache), _bits(want))
    assert bool(q_out.float().abs().sum() > 0) and bool(cache[pos].float().abs().sum() > 0)


# ---- model ---------------------------------------------------------------------------------------------------------------------------------
TINY = dict(hidden=256, layers=2, heads=4, kv_heads=2, intermediate=512, vocab=32768)


def _exact_state_dict(cfg, seed=0):
    """random_qwen2_state_dict with every projection and lm_head replaced by an fp8-exact matrix (norms, biases, embeddings stay fp16 random)"""
    sd = LM.random_qwen2_state_dict(cfg, seed=seed)
    for i, k in enumerate(sorted(sd)):
        if k.endswith("_proj.weight") or k == "lm_head.weight":
            sd[k] = _w8.fp8_exact_matrix(sd[k].shape[0], sd[k].shape[1], seed=100 + i)[0].cuda()
    return sd


@pytest.fixture(scope="module")
def exact_model():
    cfg = LM.Qwen2ConfigLite(**TINY)
    sd = _exact_state_dict(cfg)
    emb = (torch.randn(40, 256, generator=_w8.gen(2)) * 0.5).half().cuda()
    return cfg, sd, emb


def _decode(lm, emb, steps=8, graph=False):
    """40-token prefill + `steps` greedy decode steps: ([steps, vocab] decode logits, tokens)"""
    lm.reset_cache()
    logits = lm.forward(emb)
    first = int(logits.argmax())
    rows, toks = [], [first]
    if graph:
        dg = LM.DecodeGraph(lm, max_new_tokens=steps + 1)
        dg.start(first)
        dg.capture()
        for _ in range(steps):
            dg.graph.replay()
            rows.append(dg.logits.clone())
        toks += dg.out[:steps].cpu().tolist()
        lm.cache_len += steps
    else:
        for _ in range(steps):
            rows.append(lm.forward(lm.embed_tokens(torch.tensor([toks[-1]], device="cuda"))).clone())
            toks.append(int(rows[-1].argmax()))
    return torch.stack(rows), toks


def test_fp8_model_with_fp8_exact_weights_matches_the_fp32_reference_and_the_graph(exact_model):
    cfg, sd, emb = exact_model
    lm = LM.Qwen2Model(sd, cfg, max_seq=64, decode_weights="fp8")
    assert lm.w8 is not None and lm.w8["L"][0]["wq"].data_ptr() == lm.w8["L"][0]["wqkv"].data_ptr() and lm.w8["lm_head"].dtype == torch.uint8
    for k in ("wqkv", "wo", "wgu", "wd"):                           # the weights are fp8-exact: dequantising returns them
        deq = _w8.e4m3_values(lm.w8["L"][1][k].cpu()) * lm.w8["L"][1]["s" + k[1:]].cpu().double()[:, None]
        assert torch.equal(deq, lm.L[1][k].cpu().double()), k
    seen = []
    orig = ops.gemv_w8
    ops.gemv_w8 = lambda *a, **k: (seen.append(1), orig(*a, **k))[1]
    try:
        eager, toks = _decode(lm, emb)
    finally:
        ops.gemv_w8 = orig
    assert len(seen) == 8 * (cfg.layers * 5 + 1)                   # every decode projection went through the w8 kernel
    seq = torch.cat([emb, lm.embed_tokens(torch.tensor(toks[:-1], device="cuda"))])
    ref = R.qwen2_logits({k: v.float() for k, v in sd.items()}, seq.float(), heads=4, kv_heads=2, layers=2, head_dim=64)
    assert_close_fp16(eager, ref[40:48], what="fp8 decode logits (fp8-exact weights) vs fp32 torch_ref")
    g_logits, g_toks = _decode(lm, emb, graph=True)
    assert g_toks == toks and torch.equal(_bits(g_logits), _bits(eager))          # DecodeGraph == the eager loop, bitwise


def test_default_model_is_untouched_by_an_fp8_sibling_and_views_share(exact_model):
    cfg, sd, emb = exact_model
    lm = LM.Qwen2Model(sd, cfg, max_seq=64)
    assert lm.w8 is None
    before, toks = _decode(lm, emb)
    view = lm.shared_view().enable_fp8_decode()
    assert lm.w8 is None and view.w8 is not None
    after, toks2 = _decode(lm, emb)
    assert toks2 == toks and torch.equal(_bits(after), _bits(before))
    v_logits, v_toks = _decode(view, emb)
    lm8 = LM.Qwen2Model(sd, cfg, max_seq=64, decode_weights="fp8")
    p_logits, p_toks = _decode(lm8, emb)
    assert v_toks == p_toks and torch.equal(_bits(v_logits), _bits(p_logits))
    child = lm8.shared_view()
    assert child.w8 is lm8.w8 and _decode(child, emb)[1] == p_toks                # a view of an fp8 model decodes from the same fp8 tensors
    with pytest.raises(ValueError):
        LM.Qwen2Model(sd, cfg, max_seq=64, decode_weights="int4")


def test_fp8_path_on_ordinary_weights_is_exact_against_its_dequantised_weights():
    """ordinary N(0, 0.02^2) weights: EVERY projection of every decode step (q, k|v, o, gate/up, down, lm_head: 8 x 11 launches) against an fp64
    recomputation from the dequantised weights and the inputs that launch was given - the kernel contract inside the model.  The distance to the
    fp16 path is a property of the format, not of this code: printed, not gated."""
    cfg = LM.Qwen2ConfigLite(**TINY)
    sd = LM.random_qwen2_state_dict(cfg, seed=3)
    emb = (torch.randn(40, 256, generator=_w8.gen(4)) * 0.5).half().cuda()
    lm16, lm8 = LM.Qwen2Model(sd, cfg, max_seq=64), LM.Qwen2Model(sd, cfg, max_seq=64, decode_weights="fp8")
    calls, deq = [], {}
    orig = ops.gemv_w8

    def spy(q, s, x, bias=None, residual=None, epilogue="none", rms_gamma=None, rms_eps=1e-6, **k):
        y = orig(q, s, x, bias, residual, epilogue=epilogue, rms_gamma=rms_gamma, rms_eps=rms_eps, **k)
        cpu = lambda t: None if t is None else t.detach().reshape(-1).cpu().clone()
        calls.append((q, cpu(s), cpu(x), cpu(bias), cpu(residual), epilogue, cpu(rms_gamma), rms_eps, cpu(y)))
        return y
    ops.gemv_w8 = spy
    try:
        l8, t8 = _decode(lm8, emb)
    finally:
        ops.gemv_w8 = orig
    assert len(calls) == 8 * 11
    for i, (q, s, x, b, r, epi, g, eps, y) in enumerate(calls):
        if q.data_ptr() not in deq:
            deq[q.data_ptr()] = _w8.e4m3_values(q.cpu())
        xh = x.double() if g is None else _w8.rmsnorm_fp16(x, g, eps)
        c = dict(q=q.cpu(), scale=s, xh=xh, bias=b, res=r, swiglu=epi == "swiglu")
        assert_close_fp16(y, _w8.reference(c, values=lambda _: deq[q.data_ptr()]), what=f"decode launch {i} ({tuple(q.shape)}, {epi})")
    l16, t16 = _decode(lm16, emb)
    d = (l8 - l16).float()
    print(f"\n[w8] fp8 vs fp16 decode logits, tiny model, 8 steps: rms rel {(d.pow(2).mean().sqrt() / l16.pow(2).mean().sqrt()).item():.3e}, "
          f"top-1 agreement {sum(a == b for a, b in zip(t8, t16))}/{len(t16)}")


# ---- entry point ---------------------------------------------------------------------------------------------------------------------------
def test_entry_point_runs_with_the_flag(tmp_path):
    import inference_streaming_longva_v2 as E
    args = E.parse_args(["--video_dir", "none", "--model_name", "none", "--memory_basic_dir", str(tmp_path / "mem"), "--save_file",
                         str(tmp_path / "out.json"), "--annotations", "none", "--language", "en", "--conv-mode", "qwen_1_5", "--synthetic", "1",
                         "--tiny", "--chunk_size", "4", "--num_clusters", "2", "--interval", "3", "--short_window", "6", "--remember_window", "3",
                         "--max_new_tokens", "4", "--multi_modal_memory", "--decode_weights", "fp8"])
    seen = []
    orig = ops.gemv_w8
    ops.gemv_w8 = lambda *a, **k: (seen.append(1), orig(*a, **k))[1]
    try:
        E.run_inference(args)
    finally:
        ops.gemv_w8 = orig
    out = json.load(open(tmp_path / "out.json"))
    assert len(out) == 2 and all(isinstance(r["predict"], str) for r in out) and seen


def test_entry_point_runs_with_the_environment_setting(tmp_path):
    env = dict(os.environ, SC_DECODE_WEIGHTS="fp8")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_w8_child.py"), "entry", str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    calls = [l for l in r.stdout.splitlines() if l.startswith("W8CALLS")]
    assert calls and int(calls[0].split()[1]) > 0
    assert len(json.load(open(tmp_path / "out.json"))) == 2
