"""GPU: the one-call text-encoder forward (sc_text_encoder_f16, BertEncoder.forward's default) against the layer-by-layer body
(forward(layerwise=True)): the same launches behind one entry point, so the hidden states must be EQUAL bit for bit - torch.equal, no
tolerance.  Widths: the tiny golden BERT's (H 128, 4 heads of 32, I 256), MiniLM's (H 384, 12 heads of 32, I 1536) and BERT-large's (H 1024,
16 heads of 64, I 4096), two layers each.  Batches: one short text (B * L <= 32 rows: the skinny GEMMs), ragged lengths, 10 x 40 (400 rows:
the mid-M GEMM), 16 texts with one of length 1, and no lengths at all."""
import functools

import pytest
import torch

from streamchat_amd import ops, text as T

pytestmark = pytest.mark.gpu

CONFIGS = {
    "tiny": dict(hidden=128, layers=2, heads=4, intermediate=256, vocab=500, max_pos=64),
    "minilm": dict(T.MINILM_L6, layers=2),
    "bert-large": dict(T.BERT_LARGE, layers=2),
}
# name -> (B, L, lengths or None)
BATCHES = {
    "B1-L7": (1, 7, [7]),
    "B3-ragged": (3, 40, [9, 40, 23]),
    "B10-L40": (10, 40, [40] * 10),
    "B16-one-len1": (16, 12, [12, 1, 5, 12, 7, 3, 12, 9, 2, 11, 12, 4, 6, 8, 10, 12]),
    "no-lengths": (4, 19, None),
}


@functools.lru_cache(maxsize=None)
def _encoder(name):
    cfg = T.BertConfigLite(**CONFIGS[name])
    return T.BertEncoder(T.random_bert_state_dict(cfg, seed=7, std=0.05), cfg)


def _ids(enc, B, L, lengths, seed=0):
    g = torch.Generator().manual_seed(seed + 131 * B + L)
    ids = torch.randint(1, enc.cfg.vocab, (B, L), generator=g)
    if lengths is not None:
        for b, n in enumerate(lengths):
            ids[b, n:] = 0                                         # right padding
    return ids.cuda()


def _both(enc, ids, lengths):
    got = enc.forward(ids, lengths)
    ref = enc.forward(ids, lengths, layerwise=True)
    torch.cuda.synchronize()
    return got, ref


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_native_forward_equals_layerwise(name, batch):
    enc = _encoder(name)
    B, L, lengths = BATCHES[batch]
    got, ref = _both(enc, _ids(enc, B, L, lengths), lengths)
    assert got.shape == ref.shape == (B, L, enc.cfg.hidden) and got.dtype == torch.float16
    assert not torch.isnan(ref.float()).any()
    assert torch.equal(got, ref), f"{int((got != ref).sum())} of {got.numel()} hidden-state elements differ"


@pytest.mark.parametrize("name", list(CONFIGS))
def test_result_does_not_depend_on_stale_scratch(name):
    """a large call, then the stream's scratch filled with NaN, then a small call: every buffer the small call reads was written by it"""
    enc = _encoder(name)
    B, L, lengths = BATCHES["B10-L40"]
    enc.forward(_ids(enc, B, L, lengths), lengths)
    ws = ops._workspace(1, enc.device)
    assert ws.numel() >= ops._lib.load().sc_text_encoder_workspace_bytes(B * L, enc.cfg.hidden, enc.cfg.intermediate)
    ws.view(torch.float16).fill_(float("nan"))
    B, L, lengths = BATCHES["B3-ragged"]
    ids = _ids(enc, B, L, lengths)
    got = enc.forward(ids, lengths)
    assert ops._workspace(1, enc.device).data_ptr() == ws.data_ptr()           # the same scratch was reused
    ref = enc.forward(ids, lengths, layerwise=True)
    torch.cuda.synchronize()
    assert not torch.isnan(got.float()).any() and torch.equal(got, ref)


def test_non_default_stream():
    enc = _encoder("minilm")
    B, L, lengths = BATCHES["B10-L40"]
    ids = _ids(enc, B, L, lengths)
    ref = enc.forward(ids, lengths, layerwise=True)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = enc.forward(ids, lengths)
        s.synchronize()
    assert torch.equal(got, ref)


def test_embedding_entry_points_equal_layerwise():
    B, L, lengths = BATCHES["B16-one-len1"]
    lens = torch.tensor(lengths)
    enc = _encoder("bert-large")
    ids = _ids(enc, B, L, lengths)
    cls = enc.embed_cls(ids, lens)
    ref = ops.pool(enc.forward(ids, lens, layerwise=True), lens, "cls", normalize=False)
    assert cls.dtype == torch.float32 and torch.equal(cls, ref)
    enc = _encoder("minilm")
    ids = _ids(enc, B, L, lengths)
    emb = T.SentenceEmbedder(enc).embed(ids, lens)
    ref = ops.pool(enc.forward(ids, lens, layerwise=True), lens, "mean", normalize=True)
    torch.cuda.synchronize()
    assert emb.shape == (B, 384) and torch.equal(emb, ref)


def test_argument_errors_come_back_before_any_device_work():
    from ctypes import c_float, c_void_p
    lib = ops._lib.load()
    p = c_void_p(4096)
    tab = (ops._lib.TextEncoderLayer * 1)()
    rc = lib.sc_text_encoder_f16(tab, 1, 128, 4, 256, c_float(1e-12), p, p, p, p, p, 500, p, None, 1, 8, p, None, 0, None)
    assert rc == -1 and b"null pointer" in lib.sc_last_error()
    rc = lib.sc_text_encoder_f16(tab, 1, 128, 4, 256, c_float(1e-12), p, p, p, p, p, 500, p, None, 1, 8, p, p, 16, None)
    assert rc == -2 and b"workspace" in lib.sc_last_error()
    rc = lib.sc_text_encoder_f16(tab, 1, 100, 4, 256, c_float(1e-12), p, p, p, p, p, 500, p, None, 1, 8, p, p, 1 << 20, None)
    assert rc == -1 and b"multiples of 128" in lib.sc_last_error()
    rc = lib.sc_text_encoder_f16(tab, 1, 128, 4, 256, c_float(1e-12), p, p, p, p, p, 500, p, None, 1, 8, p, p, 1 << 20, None)
    assert rc == -1 and b"layer 0 has a null" in lib.sc_last_error()
