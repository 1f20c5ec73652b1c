"""GPU: FP8 (e4m3) weights for the BATCHED decode (llm.BatchDecoder(decode_weights="fp8"), ops.gemm_w8, include/streamchat_hip_w8_batched.h).
With fp8-EXACT weights (tests/_w8.fp8_exact_matrix) the fp8 decoder is mathematically the fp16 model: every projection of a step goes through
gemm_w8, the logits match the fp32 reference, a captured step replays the eager bits.  With ordinary weights every launch is exact against its
dequantised weights; a sequence's bits do not depend on what it is batched with; the weight mode and the cache mode are independent; an fp16
decoder is untouched by an fp8 sibling; the defaults hold; beams and the entry point reach the kernel."""
import json

import pytest
import torch

from oracle import torch_ref as R
from streamchat_amd import llm as LM, ops
from tests import _w8, _w8_gemm as G
from tests._tol import assert_close_fp16
from tests.test_gpu_w8 import TINY, _exact_state_dict

pytestmark = pytest.mark.gpu
N_NEW = 9                                       # 8 decode steps
LENS = (24, 17, 33)


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).cpu()


def _prompts(cfg, seed=5):
    return [(torch.randn(n, cfg.hidden, generator=_w8.gen(seed + i)) * 0.5).half().cuda() for i, n in enumerate(LENS)]


@pytest.fixture(scope="module")
def exact():
    cfg = LM.Qwen2ConfigLite(**TINY)
    sd = _exact_state_dict(cfg)
    return cfg, sd, LM.Qwen2Model(sd, cfg, max_seq=64), _prompts(cfg)


@pytest.fixture(scope="module")
def ordinary():
    cfg = LM.Qwen2ConfigLite(**{**TINY, "head_dim": 128})
    return cfg, LM.Qwen2Model(LM.random_qwen2_state_dict(cfg, seed=3), cfg, max_seq=64), _prompts(cfg, 15)


class _Spy:
    """counts (and optionally records) the calls of ops.gemm and ops.gemm_w8 while active"""

    def __init__(self, monkeypatch, record=False):
        self.gemm, self.w8, self.rec = 0, 0, []
        real, real8 = ops.gemm, ops.gemm_w8

        def gemm(*a, **k):
            self.gemm += 1
            return real(*a, **k)

        def gemm_w8(a, q, scale, bias=None, residual=None, epilogue="none", out=None, out_f32=False):
            self.w8 += 1
            y = real8(a, q, scale, bias, residual, epilogue=epilogue, out=out, out_f32=out_f32)
            if record:
                cpu = lambda t: None if t is None else t.detach().cpu().clone()
                self.rec.append((q, cpu(scale), cpu(a), cpu(bias), cpu(residual), epilogue, cpu(y)))
            return y
        monkeypatch.setattr(ops, "gemm", gemm)
        monkeypatch.setattr(ops, "gemm_w8", gemm_w8)


def _greedy(dec, steps, tokens=None):
    """`steps` eager decode steps, greedy (or fed `tokens` [steps][B]): ([steps, B, vocab] logits, the tokens fed)"""
    dec.prepare_steps(steps + 1)
    rows, fed = [], []
    tok = dec.logits.argmax(dim=1).to(torch.int32)
    for t in range(steps):
        if tokens is not None:
            tok = torch.tensor(tokens[t], dtype=torch.int32, device="cuda")
        fed.append(tok.cpu().tolist())
        rows.append(dec.step(tok).clone())
        tok = rows[-1].argmax(dim=1).to(torch.int32)
    return torch.stack(rows), fed


def test_fp8_exact_weights_every_projection_through_gemm_w8_reference_and_graph(exact, monkeypatch):
    cfg, sd, lm, prompts = exact
    dec = LM.BatchDecoder(lm, prompts, N_NEW, decode_weights="fp8")
    assert dec.decode_weights == "fp8" and lm.w8 is None and dec._w8 is lm._w8_shared["w8"]
    with monkeypatch.context() as mp:
        spy = _Spy(mp)
        eager, fed = _greedy(dec, N_NEW - 1)
    assert spy.w8 == (N_NEW - 1) * (cfg.layers * 4 + 1) and spy.gemm == 0
    for b, p in enumerate(prompts):
        seq = torch.cat([p, lm.embed_tokens(torch.tensor([f[b] for f in fed], device="cuda"))])
        ref = R.qwen2_logits({k: v.float() for k, v in sd.items()}, seq.float(), heads=4, kv_heads=2, layers=2, head_dim=64)
        n = p.shape[0]
        assert_close_fp16(eager[:, b], ref[n:n + N_NEW - 1], what=f"fp8-weight batched decode logits (fp8-exact weights), sequence {b}, vs fp32 torch_ref")
    # the step replayed from a captured graph, fed the same tokens: the eager bits
    dec = LM.BatchDecoder(lm, prompts, N_NEW, decode_weights="fp8")
    dec.prepare_steps(N_NEW)
    tok = torch.zeros(len(prompts), dtype=torch.int32, device="cuda")
    graph, out = LM._capture_graph(lm.device, lambda: dec.step(tok), (dec.len,))
    for t in range(N_NEW - 1):
        tok.copy_(torch.tensor(fed[t], dtype=torch.int32))
        graph.replay()
        assert torch.equal(_bits(out), _bits(eager[t])), f"replayed step {t}"
    # generate() captures the fp8-weight step as it captures the fp16 one
    a = LM.BatchDecoder(lm, prompts, N_NEW, decode_weights="fp8").generate(N_NEW)
    b = LM.BatchDecoder(lm, prompts, N_NEW, decode_weights="fp8").generate(N_NEW, use_graph=False)
    assert a == b and all(len(t) == N_NEW for t in a)


def test_ordinary_weights_every_launch_against_its_dequantised_weights(ordinary, monkeypatch):
    """every gemm_w8 launch of 8 steps against fp64 from the dequantised weights and THAT launch's inputs: the kernel contract inside the model.
    The distance to the fp16-weight run is the format's (about 2.6 % relative rms per projection), not this code's: printed, not gated."""
    cfg, lm, prompts = ordinary
    dec = LM.BatchDecoder(lm, prompts, N_NEW, decode_weights="fp8")
    with monkeypatch.context() as mp:
        spy = _Spy(mp, record=True)
        l8, fed = _greedy(dec, N_NEW - 1)
    assert len(spy.rec) == (N_NEW - 1) * (cfg.layers * 4 + 1) and spy.gemm == 0
    for i, (q, s, a, b, r, epi, y) in enumerate(spy.rec):
        c = dict(q=q.cpu(), scale=s, a=a, bias=b, res=r, swiglu=epi == "swiglu")
        assert_close_fp16(y, G.reference(c)[1], what=f"batched decode launch {i} ({tuple(q.shape)}, {epi})")
    l16, _ = _greedy(LM.BatchDecoder(lm, prompts, N_NEW, decode_weights="fp16"), N_NEW - 1, tokens=fed)
    d = (l8 - l16).float()
    print(f"\n[w8 batched] fp8- vs fp16-weight logits, tiny model, 8 steps, same tokens: rms rel {(d.pow(2).mean().sqrt() / l16.pow(2).mean().sqrt()).item():.3e}, "
          f"top-1 agreement {(l8.argmax(-1) == l16.argmax(-1)).float().mean().item():.3f}  (the format's cost, r09: 2.6 % relative rms per projection)")


def test_a_sequence_does_not_depend_on_what_it_is_batched_with(ordinary):
    cfg, lm, prompts = ordinary
    all3, fed = _greedy(LM.BatchDecoder(lm, prompts, N_NEW, decode_weights="fp8"), N_NEW - 1)
    for b in (0, 2):
        dec = LM.BatchDecoder(lm, [prompts[b]], N_NEW, decode_weights="fp8")
        dec.nsplit_override = LM.batched_decode_nsplit(3, cfg.kv_heads, max(LENS) + N_NEW)      # (the attention's split is sized by the batch: pin it)
        one, _ = _greedy(dec, N_NEW - 1, tokens=[[f[b]] for f in fed])
        assert torch.equal(_bits(one[:, 0]), _bits(all3[:, b])), f"sequence {b}: alone it gives other logits bits than in the batch of 3"


def _restated_projections(mp):
    """inside the context every projection of `BatchDecoder.step` is a torch restatement in fp64 on the device - ops.gemm from the fp16 weights,
    ops.gemm_w8 from the DEQUANTISED ones: epi(scale * (a @ value(q)^T) + bias) (+ residual), rounded once to the output type - so a decoder run
    under it is the same model at the same contract with none of this code's GEMM kernels in it.  Returns the call counts [gemm, gemm_w8]."""
    deq, calls = {}, [0, 0]

    def finish(z, bias, residual, epilogue, out, out_f32):
        if bias is not None:
            z = z + bias.double()
        z = G.swiglu64(z) if epilogue == "swiglu" else z
        assert epilogue in ("none", "swiglu")
        if residual is not None:
            z = z + residual.double()
        y = z.to(torch.float32 if out_f32 or (out is not None and out.dtype == torch.float32) else torch.float16)
        return y if out is None else out.copy_(y)

    def gemm(a, w, bias=None, residual=None, epilogue="none", out=None, out_f32=False):
        calls[0] += 1
        return finish(a.double() @ w.double().t(), bias, residual, epilogue, out, out_f32)

    def gemm_w8(a, q, scale, bias=None, residual=None, epilogue="none", out=None, out_f32=False):
        calls[1] += 1
        if q.data_ptr() not in deq:
            deq[q.data_ptr()] = _w8.e4m3_values(q.cpu()).cuda()
        return finish((a.double() @ deq[q.data_ptr()].t()) * scale.double(), bias, residual, epilogue, out, out_f32)
    mp.setattr(ops, "gemm", gemm)
    mp.setattr(ops, "gemm_w8", gemm_w8)
    return calls


def test_all_four_combinations_run_and_agree_with_a_restated_run(ordinary, monkeypatch):
    """weights x cache, ordinary weights.  Each combination is decoded twice from the same prompts and the same fed tokens: by the kernels, and by
    the SAME decoder with its five projections restated in torch fp64 (`_restated_projections`: the fp16 weights, or the dequantised e4m3 ones).
    The two runs' logits agree at assert_close_fp16, the contract of every other model test here; the combination routes through the GEMM its
    weight mode names and through the cache its cache mode names."""
    cfg, lm, prompts = ordinary
    steps, n = 4, 4 * (cfg.layers * 4 + 1)
    fed = [[5, 6, 7], [9, 2, 11], [3, 3, 8], [100, 200, 300]]
    for wmode in ("fp16", "fp8"):
        for cmode in ("fp16", "fp8"):
            dec = LM.BatchDecoder(lm, prompts, N_NEW, kv_cache=cmode, decode_weights=wmode)
            assert dec.decode_weights == wmode and dec.kv_cache == cmode and (dec.kv8 is not None) == (cmode == "fp8") and (dec._w8 is not None) == (wmode == "fp8")
            with monkeypatch.context() as mp:
                spy = _Spy(mp)
                got, _ = _greedy(dec, steps, tokens=fed)
            assert (spy.gemm, spy.w8) == ((0, n) if wmode == "fp8" else (n, 0))
            ref_dec = LM.BatchDecoder(lm, prompts, N_NEW, kv_cache=cmode, decode_weights=wmode)        # (the prefill runs before the restatement: it is this code's, as in `dec`)
            assert torch.equal(_bits(ref_dec.logits), _bits(dec.logits))
            with monkeypatch.context() as mp:
                calls = _restated_projections(mp)
                want, _ = _greedy(ref_dec, steps, tokens=fed)
            assert calls == ([0, n] if wmode == "fp8" else [n, 0])
            assert bool(torch.isfinite(got).all())
            for t in range(steps):
                assert_close_fp16(got[t], want[t], what=f"weights {wmode} / cache {cmode}, step {t}: kernels vs the restated projections")
    assert lm.w8 is None and lm.kv_cache == "fp16"


def test_an_fp16_decoder_is_untouched_by_an_fp8_sibling(monkeypatch):
    cfg = LM.Qwen2ConfigLite(**TINY)
    lm = LM.Qwen2Model(LM.random_qwen2_state_dict(cfg, seed=3), cfg, max_seq=64)
    prompts = _prompts(cfg, 25)
    before, fed = _greedy(LM.BatchDecoder(lm, prompts, N_NEW), N_NEW - 1)
    assert "w8" not in lm._w8_shared
    sib = LM.BatchDecoder(lm, prompts, N_NEW, decode_weights="fp8")
    _greedy(sib, 2)
    assert lm.w8 is None and "w8" in lm._w8_shared and lm.batch_decode_weights == "fp16"
    with monkeypatch.context() as mp:
        spy = _Spy(mp)
        after, fed2 = _greedy(LM.BatchDecoder(lm, prompts, N_NEW), N_NEW - 1)
    assert spy.w8 == 0 and fed2 == fed and torch.equal(_bits(after), _bits(before))
    # the model's own batch-1 decode still runs from fp16
    seen = []
    monkeypatch.setattr(ops, "gemv_w8", lambda *a, **k: seen.append(1))
    lm.reset_cache(); lm.forward(prompts[0]); lm.forward(lm.embed_tokens(torch.tensor([3], device="cuda")))
    assert not seen
    # and an fp8 batch-1 model's decoder stays fp16 unless asked
    lm8 = lm.shared_view().enable_fp8_decode()
    assert lm8.w8 is sib._w8 and LM.BatchDecoder(lm8, prompts, N_NEW).decode_weights == "fp16"


def test_defaults_hold(monkeypatch):
    cfg = LM.Qwen2ConfigLite(**TINY)
    sd = LM.random_qwen2_state_dict(cfg, seed=3)
    lm = LM.Qwen2Model(sd, cfg, max_seq=64)
    prompts = _prompts(cfg, 35)[:2]
    assert LM.DEFAULT_BATCH_DECODE_WEIGHTS == "fp16" and lm.batch_decode_weights == "fp16" and LM.BatchDecoder(lm, prompts, 4).decode_weights == "fp16"
    mb = lm.shared_view().set_batch_decode_weights("fp8")               # asked on the model; a view inherits it; the argument still wins
    assert mb.w8 is None and mb.shared_view().batch_decode_weights == "fp8" and lm.batch_decode_weights == "fp16"
    assert LM.BatchDecoder(mb, prompts, 4).decode_weights == "fp8" and LM.BatchDecoder(mb, prompts, 4, decode_weights="fp16")._w8 is None
    mc = LM.Qwen2Model(sd, cfg, max_seq=64, batch_decode_weights="fp8")
    assert mc.batch_decode_weights == "fp8" and mc.w8 is None and LM.BatchDecoder(mc, prompts, 4)._w8 is not None
    for bad in (lambda: LM.BatchDecoder(lm, prompts, 4, decode_weights="int4"), lambda: lm.set_batch_decode_weights("fp4"),
                lambda: LM.Qwen2Model(sd, cfg, batch_decode_weights="e5m2"), lambda: LM.check_batch_decode_weights("")):
        with pytest.raises(ValueError, match="batch_decode_weights must be one of"):
            bad()
    import inference_streaming_longva_v2 as E
    base = ["--video_dir", "none", "--model_name", "none", "--memory_basic_dir", "m", "--save_file", "o", "--annotations", "none", "--language", "en",
            "--conv-mode", "qwen_1_5"]
    assert E.parse_args(base).batch_decode_weights == "fp16" and E.parse_args(base + ["--batch_decode_weights", "fp8"]).batch_decode_weights == "fp8"
    with pytest.raises(SystemExit):
        E.parse_args(base + ["--batch_decode_weights", "int4"])
    # the environment setting is read once at import: a child interpreter
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from streamchat_amd import llm; print('MODE', llm.DEFAULT_BATCH_DECODE_WEIGHTS, llm.DEFAULT_DECODE_WEIGHTS)"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=root, SC_BATCH_DECODE_WEIGHTS="fp8"), capture_output=True, text=True, cwd=root, timeout=300)
    assert r.returncode == 0 and "MODE fp8 fp16" in r.stdout, r.stderr[-2000:]
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=root, SC_BATCH_DECODE_WEIGHTS="int4"), capture_output=True, text=True, cwd=root, timeout=300)
    assert r.returncode != 0 and "decode_weights must be one of" in r.stderr


def test_beams_run_through_gemm_w8(monkeypatch):
    cfg = LM.Qwen2ConfigLite(**TINY)
    lm = LM.Qwen2Model(LM.random_qwen2_state_dict(cfg, seed=3), cfg, max_seq=64, batch_decode_weights="fp8")
    model = LM.LlavaQwenForCausalLM(lm)
    spy = _Spy(monkeypatch)
    ids = torch.tensor([[5, 9, 11, 200, 7, 3]], device="cuda")
    out = model.generate_with_image_embedding(ids, [], num_beams=3, max_new_tokens=5, do_sample=False, temperature=0)
    assert out.shape[0] == 1 and 1 <= out.shape[1] <= 5 and spy.w8 > 0 and spy.w8 % (cfg.layers * 4 + 1) == 0 and lm.w8 is None


def test_entry_point_captions_with_fp8_batch_weights(tmp_path, monkeypatch):
    import inference_streaming_longva_v2 as E
    spy = _Spy(monkeypatch)
    args = E.parse_args(["--video_dir", "none", "--model_name", "none", "--memory_basic_dir", str(tmp_path / "mem"), "--save_file",
                         str(tmp_path / "out.json"), "--annotations", "none", "--language", "en", "--conv-mode", "qwen_1_5", "--synthetic", "1",
                         "--tiny", "--chunk_size", "4", "--num_clusters", "2", "--interval", "3", "--short_window", "6", "--remember_window", "3",
                         "--max_new_tokens", "4", "--multi_modal_memory", "--batch_captions", "1", "--batch_decode_weights", "fp8"])
    assert args.batch_decode_weights == "fp8" and args.decode_weights == "fp16" and args.batch_kv_cache == "fp16"
    E.run_inference(args)
    out = json.load(open(tmp_path / "out.json"))
    assert len(out) >= 1 and all("predict" in r for r in out) and spy.w8 > 0
