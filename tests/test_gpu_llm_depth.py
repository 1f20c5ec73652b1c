"""The Qwen2 stack at depth: 1, 3 and 28 layers at the narrow shape of tests/_llm_depth.py, and the real 28 layers at the 7B widths once.

Every other numerical test builds 2 layers, where a layer is only ever the first or the last.  streamchat_amd/llm.py has four bodies that loop
over the layers (Qwen2Model.forward with its trimmed last layer, _decode_one, DecodeGraph, BatchDecoder), each with per-layer state: the cache
of layer l, the h / h2 ping-pong, the graph's nodes, the batched caches.  Here a middle layer exists (3, 28), the trimmed last layer is also
the first (1) or sits behind 27 full ones (28), and the fp16 residual stream runs through the 28 blocks bench.py reports.

Yardstick (tests/test_gpu_heavy_tail.py's contract; what it can tell apart: tests/test_llm_depth_power.py, tests/LLM_DEPTH_POWER.md):

    rms(hip - ref) <= 1.5 * rms(hf_fp16_emulation - ref) + 1e-3 * rms(ref)

over all rows together and for every row alone, on the logits and on the K | V rows of EVERY layer's cache against the reference's per-layer
taps (oracle/torch_ref.qwen2_logits(taps=...)); a failure names the first layer that breaks it.  ref: fp64 on the fp16 weights (narrow shape),
fp32 (full width); both run on the GPU through torch."""
import time

import pytest
import torch

from streamchat_amd import llm as LM, ops
from tests import _llm_depth as D

pytestmark = pytest.mark.gpu

DEPTHS = [1, 3, 28]
N, ND = D.PROMPT, D.DECODE


class _Stack:
    """weights, 320 + 8 token ids, both references with taps (328 rows: causal, so rows :n are the n-row run), the default model and one that
    runs every row of the last layer"""

    def __init__(self, cfg, n_rows, two_models=True, ref_dtype=torch.float64):
        self.cfg = cfg
        sd = LM.random_qwen2_state_dict(cfg, seed=D.SEED)
        self.ids = torch.randint(0, cfg.vocab, (n_rows,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(D.SEED))
        (self.ref, self.t_ref), (self.emu, self.t_emu) = D.reference(sd, sd["model.embed_tokens.weight"][self.ids], cfg, ref_dtype)
        assert torch.isfinite(self.ref).all() and torch.isfinite(self.emu).all()
        self.full = LM.Qwen2Model(sd, cfg, max_seq=512, trim_last_layer=False) if two_models else None
        self.lm = LM.Qwen2Model(sd, cfg, max_seq=512, consume=True)            # (the reference is done: the weights are not held twice)
        assert self.lm.trim_last_layer is True
        self.emb = self.lm.embed_tokens(self.ids)

    def taps(self, n):
        return [[tuple(t[:n] for t in tap) for tap in taps] for taps in (self.t_ref, self.t_emu)]


_STACKS = {}


def _stack(layers):
    if layers not in _STACKS:
        _STACKS[layers] = _Stack(D.narrow_cfg(layers), N + ND)
    return _STACKS[layers]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _STACKS.clear()
    torch.cuda.empty_cache()


def _check_logits(name, got, ref, emu):
    """the contract over all rows together and for every row alone; the decisions wherever the truth has a clear winner (heavy-tail's margin rule)"""
    assert got.shape == ref.shape and torch.isfinite(got).all(), name
    e, b = D.contract(got, ref, emu)
    e_emu = D.contract(emu, ref, emu)[0]
    er, br = D.contract(got, ref, emu, per_row=True)
    worst = int((er / br).argmax())
    print(f"\n[depth] {name}: rms error of rms(ref)   HIP {e:.3e}   HF-fp16 storage emulation {e_emu:.3e}   bound {b:.3e}"
          f"   worst row {worst}: {er[worst]:.3e} of {br[worst]:.3e}")
    assert D.passes(e, b), f"{name}: all rows {e:.3e} > bound {b:.3e} (emulation {e_emu:.3e})"
    assert bool((er <= br).all()), f"{name}: {int((~(er <= br)).sum())} rows miss the contract, worst row {worst}: {er[worst]:.3e} > {br[worst]:.3e}"
    g, r = got.double(), ref.double()
    top2 = r.topk(2, dim=-1).values
    clear = (top2[:, 0] - top2[:, 1]) > 8 * (g - r).abs().max()
    assert clear.sum() > 0 and torch.equal(g.argmax(-1)[clear], r.argmax(-1)[clear]), f"{name}: arg-max differs where the reference has a clear winner"
    return e, e_emu


def _check_caches(name, lm, S, n, show=False):
    """rows :n of every layer's cache against that layer's taps; a failure names the first layer that breaks the contract"""
    t_ref, t_emu = S.taps(n)
    curve = D.layer_curve([c[:n] for c in lm.cache], t_ref, t_emu)
    text = D.format_curve(curve, "HIP")
    if show:
        print(f"\n[depth] {name}: K | V rows :{n} of every layer's cache, rms error of rms(ref)\n{text}")
    bad = D.first_failing(curve)
    assert bad is None, f"{name}: the cache of layer {bad} is the first that misses the contract\n{text}"
    return curve


class _AttnLog:
    """records the query row count of every ops.attention call"""

    def __init__(self, monkeypatch):
        self.sq, real = [], ops.attention

        def spy(q, *a, **kw):
            self.sq.append(int(q.shape[1]))
            return real(q, *a, **kw)
        monkeypatch.setattr(ops, "attention", spy)


# ------------------------------------------------------------------------------------------------------------------------------------
# narrow shape, 1 / 3 / 28 layers
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", DEPTHS)
def test_prefill_every_row_and_every_layers_cache(layers):
    S = _stack(layers)
    S.lm.reset_cache()
    out = S.lm.forward(S.emb[:N], last_only=False)
    assert S.lm.cache_len == N
    _check_caches(f"{layers} layers, {N}-token prefill", S.lm, S, N, show=True)
    _check_logits(f"{layers} layers, {N}-token prefill, all rows", out, S.ref[:N], S.emu[:N])


@pytest.mark.parametrize("layers", DEPTHS)
def test_trimmed_last_layer_is_bit_identical(layers, monkeypatch):
    """tests/test_gpu_prefill_trim.py's assertion where the trimmed layer is layer 0 (it reads the copied embeddings) and behind 27 full layers"""
    S = _stack(layers)
    log = _AttnLog(monkeypatch)
    S.lm.reset_cache(); S.full.reset_cache()
    lt = S.lm.forward(S.emb[:N], last_only=True)
    sq_t, log.sq[:] = list(log.sq), []
    lf = S.full.forward(S.emb[:N], last_only=True)
    assert LM.last_q_block(N, S.cfg.head_dim)[0] == 256
    assert sq_t == [N] * (layers - 1) + [N - 256] and log.sq == [N] * layers            # the trim ran, in the last layer only; the other model ran every row
    assert torch.isfinite(lf).all() and torch.equal(lt, lf)
    assert S.lm.cache_len == S.full.cache_len == N
    for l, (ct, cf) in enumerate(zip(S.lm.cache, S.full.cache)):
        assert torch.equal(ct[:N], cf[:N]), f"cache of layer {l}"


@pytest.mark.parametrize("layers", DEPTHS)
def test_chunked_prefill(layers, monkeypatch):
    """200 + 120 rows: both chunks are below 256 rows, the second sits behind the first one's keys - the fp32-projection route, untrimmed"""
    S = _stack(layers)
    log = _AttnLog(monkeypatch)
    S.lm.reset_cache()
    S.lm.forward(S.emb[:200])
    lg = S.lm.forward(S.emb[200:N])
    assert log.sq == [200] * layers + [N - 200] * layers
    assert S.lm.cache_len == N
    _check_caches(f"{layers} layers, prefill 200 + 120", S.lm, S, N)
    _check_logits(f"{layers} layers, prefill 200 + 120, last row", lg.view(1, -1), S.ref[N - 1:N], S.emu[N - 1:N])


@pytest.mark.parametrize("layers", DEPTHS)
def test_teacher_forced_decode_behind_the_prefill(layers):
    S = _stack(layers)
    S.lm.reset_cache()
    S.lm.forward(S.emb[:N])
    out = torch.stack([S.lm.forward(S.emb[N + i:N + i + 1]).view(-1) for i in range(ND)])
    assert S.lm.cache_len == N + ND
    _check_caches(f"{layers} layers, {ND} decode steps behind {N}", S.lm, S, N + ND)
    _check_logits(f"{layers} layers, {ND} decode steps behind {N}", out, S.ref[N:], S.emu[N:])


def test_decode_graph_replays_the_eager_loop_at_28_layers():
    """one capture, 8 replays (the device-side token / position advance between them): the eager loop's tokens and its logits, bit for bit"""
    S = _stack(28)
    lm = S.lm
    lm.reset_cache()
    first = int(lm.forward(S.emb[:N]).argmax())
    g = LM.DecodeGraph(lm, max_new_tokens=16)
    assert g.nsplit == lm._nsplit_prompt
    g.start(first)
    graph_logits = []
    for _ in range(8):
        g.run(1)
        graph_logits.append(g.logits.clone().view(-1))
    graph = g.out[:8].tolist()
    assert lm.cache_len == N + 8
    lm.cache_len = N                                               # rewind: the eager loop rewrites the same cache rows
    tok, eager = first, []
    for i in range(8):
        lg = lm.forward(lm.embed_tokens(torch.tensor([tok], device="cuda"))).view(-1)
        assert torch.equal(lg.view(torch.int32), graph_logits[i].view(torch.int32)), f"logits of token {i + 1}"
        tok = int(lg.argmax())
        eager.append(tok)
    assert graph == eager


def test_batched_decode_equals_one_by_one_at_28_layers():
    """three prompts of different lengths (tests/test_gpu_heavy_tail.py's 1 + 40 / 23 / 31): the same greedy ids decoded together and alone"""
    S = _stack(28)
    lm = S.lm
    g = torch.Generator(device="cuda").manual_seed(5)
    prompts = [lm.embed_tokens(torch.randint(0, S.cfg.vocab, (1 + n,), device="cuda", generator=g)) for n in (40, 23, 31)]
    single = []
    for e in prompts:
        lm.reset_cache()
        logits, toks = lm.forward(e), []
        for _ in range(6):
            toks.append(int(logits.argmax()))
            logits = lm.forward(lm.embed_tokens(torch.tensor([toks[-1]], device="cuda")))
        single.append(toks)
    dec = LM.BatchDecoder(lm, prompts, max_new_tokens=6)
    assert dec.len.tolist() == [41, 24, 32]
    assert dec.generate(6) == single


# ------------------------------------------------------------------------------------------------------------------------------------
# the benchmarked stack: 28 layers at 3584 / 18944 / 28:4 heads, once
# ------------------------------------------------------------------------------------------------------------------------------------
FULL_PROMPT, FULL_DECODE = 300, 4


def test_full_width_28_layers_prefill_and_decode():
    """Qwen2-7B's own 28 layers (vocabulary cut to 1024): a 300-token prefill, every row, and 4 teacher-forced decode steps against torch fp32 on
    the GPU (each fp16 weight upcast on lookup) and the fp16-storage emulation.  Measured on an MI355X, rms error of rms(ref), HIP / emulation:
    see DESIGN.md section 2."""
    t0 = time.time()
    cfg = LM.Qwen2ConfigLite(**dict(LM.QWEN2_7B, vocab=1024))
    S = _Stack(cfg, FULL_PROMPT + FULL_DECODE, two_models=False, ref_dtype=torch.float32)
    torch.cuda.synchronize(); t1 = time.time()
    lm, n = S.lm, FULL_PROMPT
    lm.reset_cache()
    out = lm.forward(S.emb[:n], last_only=False)
    dec = torch.stack([lm.forward(S.emb[n + i:n + i + 1]).view(-1) for i in range(FULL_DECODE)])
    torch.cuda.synchronize(); t2 = time.time()
    print(f"\n[depth] full width: weights + two reference passes + model {t1 - t0:.1f} s, HIP prefill + {FULL_DECODE} decode steps {t2 - t1:.2f} s")
    try:
        _check_caches(f"7B widths, 28 layers, {n} + {FULL_DECODE} tokens", lm, S, n + FULL_DECODE, show=True)
        _check_logits(f"7B widths, 28 layers, {n}-token prefill, all rows", out, S.ref[:n], S.emu[:n])
        _check_logits(f"7B widths, 28 layers, {FULL_DECODE} decode steps behind it", dec, S.ref[n:], S.emu[n:])
    finally:
        del S, lm
        torch.cuda.empty_cache()
