"""The last-layer trim of a last-row-only prefill is BIT-identical to running every row (llm.Qwen2Model.forward, trim_last_layer).

In the last decoder layer of a `last_only` prefill nothing reads the query side of any row but the final one.  The default forward runs it for
the rows of the attention q-block that holds the final row - through the same kernels, chosen as for the full launch (ops.gemm dispatch_rows,
ops.attention long_prefill) - and must leave exactly what `trim_last_layer=False` leaves: logits, every layer's cache rows, cache_len, the
split-KV factor, and the tokens decoded afterwards.  All comparisons are on bit patterns; there is no tolerance anywhere in this file.

The block sizes the expectations use (192 query rows per k_attn workgroup from 2048 queries on, 128 below) are written here from the contract in
include/streamchat_hip.h (sc_attention_variant / sc_attention_q_block_rows), not read back from the library.

Host part (runs without a GPU): the row-range arithmetic and the argument checks of the two dispatch hints."""
from ctypes import c_float, c_void_p

import pytest
import torch

from streamchat_amd import llm as LM
from streamchat_amd import ops

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------------------
# host: row ranges, argument checks
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, rows, b0", [(1, 192, 0), (191, 192, 0), (192, 192, 0), (193, 192, 192), (384, 192, 192), (385, 192, 384), (575, 192, 384),
                                         (4097, 192, 4032), (48994, 192, 48960), (22700, 192, 22656), (256, 128, 128), (257, 128, 256), (1024, 128, 896)])
def test_last_block_start(n, rows, b0):
    got = LM.last_block_start(n, rows)
    assert got == b0
    assert got % rows == 0 and got <= n - 1 < got + rows            # the block that holds the last row, counted from row 0


def test_last_block_start_rejects_nonsense():
    for n, rows in ((0, 192), (-3, 192), (10, 0)):
        with pytest.raises(ValueError):
            LM.last_block_start(n, rows)


def test_q_block_rows_follow_the_variant(hip_lib):
    for Dh, Sq, nsplit, rows in ((128, 2048, 1, 192), (128, 48994, 1, 192), (128, 2047, 1, 128), (128, 256, 1, 128), (64, 4096, 1, 128), (32, 577, 1, 128),
                                 (128, 4096, 2, 128), (128, 7, 16, 0)):
        assert hip_lib.sc_attention_q_block_rows(Dh, Sq, nsplit) == rows, (Dh, Sq, nsplit)
        assert (hip_lib.sc_attention_variant(Dh, Sq, nsplit) == 1) == (rows == 192)


def test_dispatch_hints_are_checked_before_any_device_work(hip_lib):
    """argument checks run before any launch: callable without a GPU, the pointers are never touched"""
    p = c_void_p(4096)
    rc = hip_lib.sc_gemm_f16(p, 256, p, None, None, 0, p, 256, 64, 256, 256, 0, 32 << 1, 0, 0, 0, None)          # dispatch as 32 rows, compute 64
    assert rc == -1 and b"SC_GEMM_DISPATCH_ROWS" in hip_lib.sc_last_error()
    rc = hip_lib.sc_gemm_f16(p, 256, p, None, None, 0, p, 256, 64, 256, 256, 0, -2, 0, 0, 0, None)
    assert rc == -1
    att = lambda Dh, nsplit, flags: hip_lib.sc_attention_f16(p, 128, p, 128, p, 128, p, 128, 1, 16, 16, 1, 1, Dh, c_float(1.0), flags, None, nsplit,
                                                             p, 1 << 20, 0, 0, 0, 0, None)
    assert att(64, 1, 4 | 1) == -1 and b"SC_ATTN_LONG_PREFILL" in hip_lib.sc_last_error()                        # long-prefill kernel: head dim 128 only
    assert att(128, 2, 4 | 1) == -1 and b"SC_ATTN_LONG_PREFILL" in hip_lib.sc_last_error()                       # ... and no split-KV
    assert att(128, 1, 8) == -1 and b"flags" in hip_lib.sc_last_error()


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: the model
# ------------------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), f"{what}: {int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements differ"


def _expected_q_rows(n):
    rows = 192 if n >= 2048 else 128
    return n - rows * ((n - 1) // rows)


@pytest.fixture(scope="module")
def models():
    """Qwen2-7B widths, 2 layers, heavy-tailed weights (tests/test_gpu_heavy_tail.py): one model built with the DEFAULT arguments, one that runs every row"""
    from tests.test_gpu_heavy_tail import heavy_qwen2
    cfg, sd = heavy_qwen2(layers=2, seed=41)
    trimmed = LM.Qwen2Model(sd, cfg, max_seq=512)
    assert trimmed.trim_last_layer is True                         # the default
    full = LM.Qwen2Model(sd, cfg, max_seq=512, trim_last_layer=False)
    ids = torch.randint(1, cfg.vocab, (9000,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(7))
    ids[0] = 0                                                     # the sink token first
    return cfg, trimmed, full, trimmed.embed_tokens(ids)


class _AttnLog:
    """records the query row count of every ops.attention call"""

    def __init__(self, monkeypatch):
        self.sq, real = [], ops.attention

        def spy(q, *a, **kw):
            self.sq.append(int(q.shape[1]))
            return real(q, *a, **kw)
        monkeypatch.setattr(ops, "attention", spy)


def _prefill(lm, chunks, last_only=True):
    lm.reset_cache(max_seq=sum(int(c.shape[0]) for c in chunks) + 64)
    for c in chunks:
        logits = lm.forward(c, last_only=last_only)
    return logits


def _decode_both_ways(lm, logits, steps=16):
    """`steps` greedy tokens after the prefill that left `logits`: a replayed DecodeGraph, then - from the same cache state - the eager loop"""
    S, first = lm.cache_len, int(logits.argmax())
    g = LM.DecodeGraph(lm, max_new_tokens=steps)
    g.start(first)
    graph = [first] + g.run(steps - 1)
    lm.cache_len = S                                               # rewind: the eager loop rewrites the same cache rows
    eager, lg = [], logits
    for i in range(steps):
        eager.append(int(lg.argmax()))
        if i + 1 < steps:
            lg = lm.forward(lm.embed_tokens(torch.tensor([eager[-1]], device="cuda")))
    return graph, eager


def _compare(models, monkeypatch, chunk_lens, decode=True):
    cfg, trimmed, full, emb = models
    log = _AttnLog(monkeypatch)
    o, chunks = 0, []
    for n in chunk_lens:
        chunks.append(emb[o:o + n]); o += n
    S, n_last = o, chunk_lens[-1]
    lt = _prefill(trimmed, chunks)
    sq_t, log.sq[:] = list(log.sq), []
    lf = _prefill(full, chunks)
    sq_f = list(log.sq)
    # the trim really ran (and only in the last layer of every chunk), the other model really ran every row
    per_chunk = lambda last: [x for n in chunk_lens for x in [n] * (cfg.layers - 1) + [last(n)]]
    assert sq_f == per_chunk(lambda n: n), sq_f
    assert sq_t == per_chunk(_expected_q_rows), (sq_t, per_chunk(_expected_q_rows))
    assert torch.isfinite(lf).all()
    _same(lt, lf, f"logits, chunks {chunk_lens}")
    assert trimmed.cache_len == full.cache_len == S
    assert trimmed._nsplit_prompt == full._nsplit_prompt == LM.decode_nsplit(cfg.head_dim, S)
    for l, (ct, cf) in enumerate(zip(trimmed.cache, full.cache)):
        _same(ct[:S], cf[:S], f"cache of layer {l}, chunks {chunk_lens}")
    if decode:
        gt, et = _decode_both_ways(trimmed, lt)
        gf, ef = _decode_both_ways(full, lf)
        assert gt == et == gf == ef, (gt, et, gf, ef)
        assert trimmed.cache_len == full.cache_len == S + 15
        for l, (ct, cf) in enumerate(zip(trimmed.cache, full.cache)):
            _same(ct[:S + 15], cf[:S + 15], f"cache of layer {l} after 16 tokens, chunks {chunk_lens}")


# 256 / 1024: 128-row q-blocks, k_gemm128 below 1024 rows, k_gemm_fat from 1024 on; 1153 = 9 * 128 + 1: ONE trimmed row under 2048;
# 2304 = 12 * 192 (a full last block), 2305 (one row), 2495 = 12 * 192 + 191; 4097: persistent GEMM walks in the full launch; 8200 >= 8192
@gpu
@pytest.mark.parametrize("n", [256, 1024, 1153, 2304, 2305, 2495, 4097, 8200])
def test_trimmed_prefill_is_bit_identical(models, monkeypatch, n):
    _compare(models, monkeypatch, [n])


@gpu
@pytest.mark.parametrize("chunks", [[1000, 2500], [2304, 300], [4097, 2049]])
def test_trimmed_second_chunk_is_bit_identical(models, monkeypatch, chunks):
    """pos0 > 0: the second chunk's queries sit behind the first chunk's keys (rotary positions and the causal offset move with pos0)"""
    _compare(models, monkeypatch, chunks)


@gpu
def test_all_rows_forward_is_untouched(models, monkeypatch):
    """last_only=False returns every row's logits: nothing may be trimmed, whatever the switch says"""
    cfg, trimmed, full, emb = models
    log = _AttnLog(monkeypatch)
    lt = _prefill(trimmed, [emb[:2305]], last_only=False)
    assert log.sq == [2305] * cfg.layers
    lf = _prefill(full, [emb[:2305]], last_only=False)
    assert lt.shape == (2305, cfg.vocab)
    _same(lt, lf, "all-row logits")
    for ct, cf in zip(trimmed.cache, full.cache):
        _same(ct[:2305], cf[:2305], "cache")


@gpu
def test_head_dim_64_takes_the_untrimmed_path(monkeypatch):
    """a shape the rotary GEMM epilogue does not serve runs every row, as before: no second, tolerance-only trim"""
    cfg = LM.Qwen2ConfigLite(hidden=1024, layers=2, heads=16, kv_heads=4, intermediate=2816, vocab=512, head_dim=64)
    sd = LM.random_qwen2_state_dict(cfg, seed=5)
    a, b = LM.Qwen2Model(sd, cfg, max_seq=512), LM.Qwen2Model(sd, cfg, max_seq=512, trim_last_layer=False)
    emb = a.embed_tokens(torch.randint(0, cfg.vocab, (300,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(6)))
    log = _AttnLog(monkeypatch)
    la = a.forward(emb)
    assert log.sq == [300, 300]
    lb = b.forward(emb)
    _same(la, lb, "logits")
    for ca, cb in zip(a.cache, b.cache):
        _same(ca[:300], cb[:300], "cache")
    cfg = LM.Qwen2ConfigLite(hidden=1024, layers=2, heads=8, kv_heads=2, intermediate=2816, vocab=512, head_dim=128)
    short = LM.Qwen2Model(LM.random_qwen2_state_dict(cfg, seed=8), cfg, max_seq=512)          # head dim 128 but n < 256: untrimmed too
    log.sq[:] = []
    short.forward(short.embed_tokens(torch.arange(1, 201, device="cuda")))
    assert log.sq == [200, 200]


@gpu
def test_batch_decoder_prefills_pick_the_trim_up(models, monkeypatch):
    """BatchDecoder prefills every sequence through forward(): trimmed, and the decoded tokens equal the untrimmed model's"""
    cfg, trimmed, full, emb = models
    prompts = [emb[:300], emb[100:2405]]
    log = _AttnLog(monkeypatch)
    dt = LM.BatchDecoder(trimmed, prompts, max_new_tokens=6)
    assert log.sq == [300] * (cfg.layers - 1) + [44] + [2305] * (cfg.layers - 1) + [1]          # last layer of each prefill: rows 256.. of 300, row 2304 of 2305
    df = LM.BatchDecoder(full, prompts, max_new_tokens=6)
    _same(dt.logits, df.logits, "first logits")
    assert dt.generate(6) == df.generate(6)


# ------------------------------------------------------------------------------------------------------------------------------------
# GPU: the two dispatch hints on their own - a row block equals those rows of the whole launch, and writes nothing else
# ------------------------------------------------------------------------------------------------------------------------------------
def _rand(shape, seed, scale=1.0):
    return (torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed)) * scale).half()


GEMM_BLOCKS = {
    # k_gemm_fat, one tile per workgroup in both launches; the block starts inside a 256-row tile and ends in the ragged last one
    "fat_1154_rows_960": dict(Mf=1154, r0=960, N=512, K=256, epi="none", res=True),
    # k_gemm_fat: the whole launch is a PERSISTENT walk (272 tiles), the block one tile per workgroup
    "fat_persistent_4099_rows_4032": dict(Mf=4099, r0=4032, N=4096, K=128, epi="quick_gelu", res=True),
    "fat_swiglu_2305_one_row": dict(Mf=2305, r0=2304, N=512, K=128, epi="swiglu", res=False),
    # k_gemm128 for a block that would take the weight-streaming kernels on its own (24 rows, K % 128 == 0)
    "gemm128_600_rows_576": dict(Mf=600, r0=576, N=256, K=128, epi="none", res=True),
    "gemm128_swiglu_257_one_row": dict(Mf=257, r0=256, N=512, K=2048, epi="swiglu", res=False),
}


@gpu
@pytest.mark.parametrize("case", sorted(GEMM_BLOCKS))
def test_gemm_row_block_dispatched_as_the_whole_gemm(case):
    """rows [r0, Mf) of an Mf-row GEMM launched with dispatch_rows = Mf: the bits of the whole launch, exactly M rows written (the write-bound
    idea of tests/test_gpu_write_bounds.py: guarded arena, frozen inputs)"""
    from tests._guard import Arena, frozen
    c = GEMM_BLOCKS[case]
    Mf, r0, N, K = c["Mf"], c["r0"], c["N"], c["K"]
    a, w, b = _rand((Mf, K), 1), _rand((N, K), 2, K ** -0.5), _rand((N,), 3)
    r = _rand((Mf, N), 4) if c["res"] else None
    whole = ops.gemm(a, w, b, r, c["epi"])
    ncol = whole.shape[1]
    ar = Arena("cuda")
    out = ar.out(Mf - r0, ncol, torch.float16, ld=ncol + 8, tail_rows=256)
    with frozen(a, w, b, r):
        ops.gemm(a[r0:], w, b, None if r is None else r[r0:], c["epi"], out=out, dispatch_rows=Mf)
    torch.cuda.synchronize()
    ar.check(case)
    _same(out, whole[r0:], case)


# the rotary q GEMM of the trimmed layer: sc_gemm_headed_f16 always runs k_gemm_fat, so it takes no hint - but the trim launches it with 1 to 192
# rows (ONE ragged 256-row tile) and with the table rows pos0 + b0.. .  (Mf, r0, pos0): one row, 191 rows, a block behind a first chunk, 128 rows
@gpu
@pytest.mark.parametrize("Mf, r0, pos0", [(2305, 2304, 0), (2495, 2304, 0), (2400, 2304, 1000), (1024, 896, 3)])
def test_rotary_gemm_row_block_on_its_own(Mf, r0, pos0):
    """rows [r0, Mf) of the rotary-epilogue GEMM launched alone at positions pos0 + r0..: the bits of the whole launch, exactly those rows written"""
    from tests._guard import Arena, frozen
    N, K, Dh = 512, 256, 128
    assert ops.attention_q_block_rows(Dh, Mf, 1) in (128, 192) and r0 == LM.last_block_start(Mf, ops.attention_q_block_rows(Dh, Mf, 1))
    a, w, b = _rand((Mf, K), 21), _rand((N, K), 22, K ** -0.5), _rand((N,), 23)
    tab = ops.rope_table(pos0 + Mf, Dh, 1e6, Dh ** -0.5 * ops.LOG2E, "cuda")
    whole = torch.empty((Mf, N), dtype=torch.float16, device="cuda")
    assert ops.gemm_headed_ok(N, K, a, w, b, whole)
    ops.gemm_headed(a, w, b, whole, "rope", N - Dh, tab, pos0)           # three rotary heads and one plain one (the k | v launch's layout)
    ar = Arena("cuda")
    out = ar.out(Mf - r0, N, torch.float16, ld=N + 8, tail_rows=256)
    assert ops.gemm_headed_ok(N, K, a[r0:], w, b, out)
    with frozen(a, w, b, tab):
        ops.gemm_headed(a[r0:], w, b, out, "rope", N - Dh, tab, pos0 + r0)
    torch.cuda.synchronize()
    ar.check(f"rotary GEMM rows {r0}..{Mf}")
    _same(out, whole[r0:], f"rotary GEMM rows {r0}..{Mf} at pos0 {pos0}")


@gpu
@pytest.mark.parametrize("Sq, pos0", [(1153, 0), (1000, 300), (1024, 0)])
def test_attention_last_128_row_q_block_on_its_own(Sq, pos0):
    """below 2048 queries the launch is k_attn with 128-row q-blocks and the block alone needs no flag: that block's bits, only its rows written"""
    from tests._guard import Arena, frozen
    Hq, Hkv, Dh = 4, 2, 128
    Skv = pos0 + Sq
    q, k, v = _rand((1, Sq, Hq * Dh), 31, 4.0), _rand((1, Skv, Hkv * Dh), 32), _rand((1, Skv, Hkv * Dh), 33)
    whole = ops.attention(q, k, v, Hq, Hkv, Dh, Dh ** -0.5, causal=True, q_prescaled=True)
    assert ops.attention_variant(Dh, Sq, 1) == 0 and ops.attention_q_block_rows(Dh, Sq, 1) == 128
    b0, long_prefill = LM.last_q_block(Sq, Dh)
    assert b0 == LM.last_block_start(Sq, 128) and not long_prefill
    ar = Arena("cuda")
    out = ar.out(Sq - b0, Hq * Dh, torch.float16, ld=Hq * Dh + 8, tail_rows=192)
    with frozen(q, k, v):
        ops.attention(q[0, b0:].unsqueeze(0), k, v, Hq, Hkv, Dh, Dh ** -0.5, causal=True, out=out.unsqueeze(0), q_prescaled=True, long_prefill=long_prefill)
    torch.cuda.synchronize()
    ar.check(f"attention Sq={Sq}")
    _same(out, whole[0, b0:], f"attention Sq={Sq} pos0={pos0}")


@gpu
@pytest.mark.parametrize("Sq, pos0", [(2400, 0), (2305, 77), (2304, 0)])
def test_attention_last_q_block_on_its_own(Sq, pos0):
    """the trailing 192-row q-block of a long causal launch, launched alone with long_prefill: that block's bits, only its rows written"""
    from tests._guard import Arena, frozen
    Hq, Hkv, Dh = 4, 2, 128
    Skv = pos0 + Sq
    q, k, v = _rand((1, Sq, Hq * Dh), 11, 4.0), _rand((1, Skv, Hkv * Dh), 12), _rand((1, Skv, Hkv * Dh), 13)
    whole = ops.attention(q, k, v, Hq, Hkv, Dh, Dh ** -0.5, causal=True, q_prescaled=True)
    assert ops.attention_variant(Dh, Sq, 1) == 1 and ops.attention_q_block_rows(Dh, Sq, 1) == 192
    b0 = LM.last_block_start(Sq, 192)
    ar = Arena("cuda")
    out = ar.out(Sq - b0, Hq * Dh, torch.float16, ld=Hq * Dh + 8, tail_rows=192)
    with frozen(q, k, v):
        ops.attention(q[0, b0:].unsqueeze(0), k, v, Hq, Hkv, Dh, Dh ** -0.5, causal=True, out=out.unsqueeze(0), q_prescaled=True, long_prefill=True)
    torch.cuda.synchronize()
    ar.check(f"attention Sq={Sq}")
    _same(out, whole[0, b0:], f"attention Sq={Sq} pos0={pos0}")
