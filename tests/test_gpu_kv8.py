"""GPU: the FP8 (e4m3) KV cache (include/streamchat_hip_kv8.h, attention_kv8.hip, llm.Qwen2Model(kv_cache="fp8")).  The quantiser is bit-identical
to the torch specification (tests/_kv8.py), the dequantiser exact, both write only their rows (tests/_guard.py), sc_attention_kv8 equals bit
for bit the fp16 decode attention with the same nsplit on the dequantised cache (the comparison tests/test_kv8_cpu.py shows to reject wrong
kernels), and an fp8-cache model prefills, decodes (eagerly and from a DecodeGraph), prefills in chunks, serves BatchDecoder and searches with
two beams (beam.beam_search over BatchDecoder steps) as the fp16-cache model does."""
import pytest
import torch

from streamchat_amd import llm as LM, ops
from tests import _kv8, _w8
from tests._guard import Arena, frozen

pytestmark = pytest.mark.gpu
DH = 128


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).cpu()


def _padded(rows, cols, dtype, pad):
    return torch.zeros((rows, cols + pad), dtype=dtype, device="cuda")[:, :cols]


# ---- quantiser / dequantiser
@pytest.mark.parametrize("Hkv", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 3, 64, 257])
@pytest.mark.parametrize("pad,dev_row", [(0, False), (128, True), (0, True), (128, False)])
def test_quantiser_equals_the_cpu_specification(n, Hkv, pad, dev_row):
    w, row0, cap = 2 * Hkv * DH, 5, 5 + n + 3
    # the edge rows come first at every n (all five at n = 64 and 257); at n = 1 and 3 the last row mixes edge segments of different kinds, as
    # many as the row has segments, so the short launches see them too and one row holds segments that want different scales
    x = torch.cat([_kv8.edge_rows(Hkv), _kv8.random_rows(max(n - 5, 1), Hkv, seed=n + Hkv)])[:n].clone()
    if n < 5:
        e = _kv8.edge_rows(1).view(5, 2, DH)
        mixed = _kv8.random_rows(1, 4, seed=50 + n).view(8, DH)[:2 * Hkv].clone()
        for i in range(min(5, 2 * Hkv)):
            mixed[i] = e[(i + n) % 5, i % 2]
        x[n - 1] = mixed.view(-1)
    codes_ref, scale_ref = _kv8.quantize_ref(x, Hkv)
    xin = _padded(n, w, torch.float16, pad // 2)
    xin.copy_(x)
    cache, scales = _padded(cap, w, torch.uint8, pad), torch.full((cap, 2 * Hkv), -1.0, device="cuda")
    cache.fill_(0xAA)
    r = torch.tensor([row0], dtype=torch.int32, device="cuda") if dev_row else row0
    with frozen(xin):
        ops.kv8_quantize_rows(xin, cache, scales, r, Hkv, DH)
    assert torch.equal(cache[row0:row0 + n].cpu(), codes_ref) and torch.equal(_bits(scales[row0:row0 + n]), _bits(scale_ref))
    keep = torch.ones(cap, dtype=torch.bool)
    keep[row0:row0 + n] = False
    assert bool((cache.cpu()[keep] == 0xAA).all()) and bool((scales.cpu()[keep] == -1).all())
    # the inverse: code * scale exactly
    out = _padded(n, w, torch.float16, pad // 2)
    ops.kv8_dequantize_rows(cache, scales, row0, n, Hkv, DH, out)
    assert torch.equal(out.cpu().double(), _kv8.dequantize_ref(codes_ref, scale_ref))


def test_quantiser_follows_a_device_row_of_a_cache_shaped_source():
    """the decode step's form: x is a staging buffer laid out like the cache, the row lives on the device"""
    Hkv, cap, w = 2, 40, 512
    stage = _kv8.random_rows(cap, Hkv, seed=9).cuda()
    cache, scales = torch.zeros((cap, w), dtype=torch.uint8, device="cuda"), torch.zeros((cap, 2 * Hkv), device="cuda")
    ops.kv8_quantize_rows(stage, cache, scales, torch.tensor([23], dtype=torch.int32, device="cuda"), Hkv, DH, x_follows_row=True)
    cr, sr = _kv8.quantize_ref(stage[23:24], Hkv)
    assert torch.equal(cache[23:24].cpu(), cr) and torch.equal(scales[23:24].cpu(), sr)
    assert int(cache.cpu().ne(0).any(dim=1).sum()) == 1 and int(scales.cpu().ne(0).any(dim=1).sum()) == 1


@pytest.mark.parametrize("n,Hkv", [(3, 1), (37, 4)])
def test_quantiser_and_dequantiser_write_only_their_rows(n, Hkv):
    """cache bytes, scales and the dequantised rows are arena views with guard bands (lead, the row pad of every row, tail); rows outside
    row0 .. row0 + n - 1 of the views keep their fill.  The source rows sit in a wider buffer whose other columns are NaN."""
    w, cap, row0 = 2 * Hkv * DH, n + 9, 4
    full = torch.full((n, w + 64), float("nan"), dtype=torch.float16, device="cuda")
    full[:, :w] = _kv8.random_rows(n, Hkv, seed=3).cuda()
    x = full[:, :w]
    ar = Arena("cuda")
    cache = ar.out(cap, w, torch.uint8, ld=w + 128, tail_rows=64)
    scales = ar.out(cap, 2 * Hkv, torch.float32, tail_rows=64)
    back = ar.out(n, w, torch.float16, ld=w + 64, tail_rows=64)
    cache.fill_(0x11); scales.fill_(3.0)
    with frozen(full):
        ops.kv8_quantize_rows(x, cache, scales, row0, Hkv, DH)
    with frozen(cache, scales):
        ops.kv8_dequantize_rows(cache, scales, row0, n, Hkv, DH, back)
    cr, sr = _kv8.quantize_ref(x, Hkv)
    assert torch.equal(cache[row0:row0 + n].cpu(), cr) and torch.equal(scales[row0:row0 + n].cpu(), sr)
    assert torch.equal(back.cpu().double(), _kv8.dequantize_ref(cr, sr))
    keep = torch.ones(cap, dtype=torch.bool)
    keep[row0:row0 + n] = False
    assert bool((cache.cpu()[keep] == 0x11).all()) and bool((scales.cpu()[keep] == 3.0).all())
    ar.check("sc_kv8_quantize_rows / sc_kv8_dequantize_rows")


# ---- attention
def _attend_both(codes, scale, q, Hkv, nsplit, pad, kv_len=None, rows=None):
    """(sc_attention_kv8, the fp16 decode attention on the dequantised cache) with the same nsplit, both [G, Hkv * 128]"""
    S, G, w = codes.shape[0], q.shape[0], 2 * Hkv * DH
    cache = _padded(S, w, torch.uint8, pad)
    cache.copy_(codes)
    sc = scale.cuda()
    deq = _padded(S, w, torch.float16, pad // 2)
    deq.copy_(_kv8.dequantize_ref(codes if rows is None else torch.cat([codes[:rows], torch.zeros_like(codes[rows:])]),
                                  scale if rows is None else torch.cat([scale[:rows], torch.ones_like(scale[rows:])])).half())
    # q [G, Hkv * 128]: query row g of KV head h at g * (Hkv * 128) + h * 128
    qd = q.cuda().view(1, G, Hkv * DH)
    kl = None if kv_len is None else torch.tensor([kv_len], dtype=torch.int32, device="cuda")
    a = ops.attention_kv8(qd, cache, sc, Hkv, DH, DH ** -0.5, kv_len=kl, nsplit=nsplit, q_prescaled=True)
    b = ops.attention(qd, deq[:, :Hkv * DH].unsqueeze(0), deq[:, Hkv * DH:].unsqueeze(0), Hkv, Hkv, DH, DH ** -0.5, causal=False, kv_len=kl, nsplit=nsplit,
                      q_prescaled=True)
    return a[0], b[0]


@pytest.mark.parametrize("G", [1, 7, 16])
@pytest.mark.parametrize("S", [1, 31, 32, 33, 767, 768, 769, 2273])
def test_attention_kv8_is_bit_identical_to_the_fp16_kernel_on_the_dequantised_cache(S, G):
    Hkv = 2
    codes, scale, q = _kv8.attention_case(S, G, Hkv, seed=100 + S + G)
    ref = _kv8.attention_fp64(q, codes, scale, Hkv)
    for i, nsplit in enumerate(dict.fromkeys([LM.decode_nsplit(DH, S), 2, 3, 5])):
        a, b = _attend_both(codes, scale, q, Hkv, nsplit, pad=128 if (i + S) % 2 else 0)
        assert ops.attention_variant(DH, G, nsplit) == 3
        assert _kv8.same_bits(a, b), f"S={S} G={G} nsplit={nsplit}: {int((a != b).sum())} of {a.numel()} elements differ"
        assert bool(torch.isfinite(a).all()) and ((a.cpu().double() - ref).abs().max() / ref.abs().max()).item() < 2e-2      # and both are an attention at all


@pytest.mark.parametrize("S,G,nsplit", _kv8.DECODE_BITS_CASES)
def test_decode_attention_keeps_its_recorded_bits(S, G, nsplit):
    """both kernels take the chunk partition, softmax step, P.V accumulation and wave merge from attention_decode_common.h, so the comparison
    above cannot see a mistake in that text; tests/golden/decode_attention_bits.npz holds what k_attn_decode + k_attn_combine gave before the
    two kernels shared it (tools/make_golden_decode_bits.py)"""
    import os
    import numpy as np
    nsplit = nsplit or LM.decode_nsplit(DH, S)
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "decode_attention_bits.npz"))
    codes, scale, q, crc = _kv8.decode_bits_inputs(S, G)
    assert crc == int(d[f"crc_{S}_{G}_{nsplit}"]), "the input generator drifted (not a kernel failure): re-record tests/golden/decode_attention_bits.npz"
    want = torch.from_numpy(d[f"bits_{S}_{G}_{nsplit}"].view(np.int16))
    a, b = _attend_both(codes, scale, q, 2, nsplit, pad=128)
    assert ops.attention_variant(DH, G, nsplit) == 3
    for name, got in (("ops.attention on the dequantised cache", b), ("ops.attention_kv8", a)):
        n = int((_bits(got) != want).sum())
        assert n == 0, f"{name}, S={S} G={G} nsplit={nsplit}: {n} of {want.numel()} elements differ from the recorded bits"


def test_poisoned_tail_contributes_nothing():
    """kv_len (device) below the allocated rows; the bytes behind it are 0x7F (NaN), their scales NaN: the result equals the unpoisoned one"""
    Hkv, G, S, extra = 2, 7, 777, 60
    codes, scale, q = _kv8.attention_case(S + extra, G, Hkv, seed=4)
    clean, ref16 = _attend_both(codes, scale, q, Hkv, 3, pad=128, kv_len=S)
    pc, ps = codes.clone(), scale.clone()
    pc[S:], ps[S:] = 0x7F, float("nan")
    poisoned, _ = _attend_both(pc, ps, q, Hkv, 3, pad=128, kv_len=S, rows=S)
    assert bool(torch.isfinite(poisoned).all()) and _kv8.same_bits(poisoned, clean) and _kv8.same_bits(clean, ref16)


# ---- the model
CFG = dict(hidden=256, layers=3, heads=4, kv_heads=2, intermediate=512, vocab=1024, head_dim=128)


def _models(decode_weights, max_seq=128):
    cfg = LM.Qwen2ConfigLite(**CFG)
    m16 = LM.Qwen2Model(LM.random_qwen2_state_dict(cfg, seed=3, std=0.05), cfg, max_seq=max_seq, decode_weights=decode_weights, kv_cache="fp16")
    m8 = m16.shared_view().set_kv_cache("fp8")
    return cfg, m16, m8


def _embeds(cfg, n, seed=0):
    return (torch.randn(n, cfg.hidden, generator=_w8.gen(seed)) * 0.5).half().cuda()


def _restated_token(ref, m8_rows, h, pos, nsplit):
    """one decode token on the fp16-cache model `ref`, whose cache holds the DEQUANTISED rows: projection, rope, a quantise -> dequantise round
    trip of the new row (CPU specification), _decode_attention (fp16), _decode_tail - the same methods the fp8 model calls"""
    c = ref.cfg
    dq, dkv, Dh = c.heads * c.head_dim, c.kv_heads * c.head_dim, c.head_dim
    tq, tk = ref.rope_tabs(pos + 1)
    for l, L in enumerate(ref.L):
        P = ref._decode_proj(l)
        q32 = LM._gemv(P["wq"], h, L["bq"], out_f32=True, rms_gamma=L["ln1"], rms_eps=c.eps).view(1, dq)
        kv32 = LM._gemv(P["wkv"], h, L["bkv"], out_f32=True, rms_gamma=L["ln1"], rms_eps=c.eps).view(1, 2 * dkv)
        q = ops.rope_f32in(q32, tq, c.heads, Dh, torch.empty((1, dq), dtype=torch.float16, device="cuda"), 0, pos)
        ops.rope_f32in(kv32, tk, c.kv_heads, Dh, ref.cache[l][pos:pos + 1], dkv, pos)
        cr, sr = _kv8.quantize_ref(ref.cache[l][pos:pos + 1], c.kv_heads)
        m8_rows.append((l, pos, cr, sr))
        ref.cache[l][pos:pos + 1].copy_(_kv8.dequantize_ref(cr, sr).half())
        h = ref._decode_tail(l, P, h, ref._decode_attention(q, ref.cache[l][:pos + 1], nsplit))
    return ref._decode_logits(h)


@pytest.mark.parametrize("decode_weights", ["fp16", "fp8"])
def test_model_prefill_decode_graph_and_chunks(decode_weights):
    cfg, m16, m8 = _models(decode_weights)
    assert m8.kv_cache == "fp8" and m16.kv_cache == "fp16" and (m8.w8 is None) == (decode_weights == "fp16")
    n = 36
    e = _embeds(cfg, n + 9)
    # prefill from an empty cache: logits bit-identical, the fp8 cache = the CPU quantiser applied to the fp16 model's cache rows
    l16, l8 = m16.forward(e[:n]), m8.forward(e[:n])
    assert torch.equal(_bits(l16), _bits(l8))
    for l in range(cfg.layers):
        cr, sr = _kv8.quantize_ref(m16.cache[l][:n], cfg.kv_heads)
        assert torch.equal(m8.kv8[l][0][:n].cpu(), cr) and torch.equal(m8.kv8[l][1][:n].cpu(), sr), l
    # eight eager tokens against the restatement on an fp16-cache model holding the dequantised rows
    ref = m16.shared_view()
    ref.reset_cache()
    for l in range(cfg.layers):
        ref.cache[l][:n].copy_(_kv8.dequantize_ref(m8.kv8[l][0][:n], m8.kv8[l][1][:n]).half())
    nsplit = LM.decode_nsplit(128, n)
    eager, rows = [], []
    for t in range(8):
        want = _restated_token(ref, rows, e[n + t:n + t + 1], n + t, nsplit)
        got = m8.forward(e[n + t:n + t + 1])
        assert torch.equal(_bits(got), _bits(want)), t
        eager.append(got.clone())
    for l, pos, cr, sr in rows:
        assert torch.equal(m8.kv8[l][0][pos:pos + 1].cpu(), cr) and torch.equal(m8.kv8[l][1][pos:pos + 1].cpu(), sr)
    # DecodeGraph: the same logits and tokens as the eager loop fed its own arg-max tokens
    def greedy(model, use_graph):
        model.reset_cache()
        first = int(model.forward(e[:n]).argmax())
        if use_graph:
            g = LM.DecodeGraph(model, max_new_tokens=16)
            g.start(first)
            toks = g.run(6)
            assert g.valid()
            return toks, g.logits.clone(), g
        toks, tok = [], first
        for _ in range(6):
            lg = model.forward(model.embed_tokens(torch.tensor([tok])))
            tok = int(lg.argmax())
            toks.append(tok)
        return toks, lg.clone(), None
    te, le, _ = greedy(m8, False)
    tg, lgr, g = greedy(m8, True)
    assert te == tg and torch.equal(_bits(le), _bits(lgr))
    m8.reset_cache(max_seq=256)                      # a reallocated fp8 cache invalidates the captured graph
    assert not g.valid()
    # chunked prefill: 20 + 16 rows, then a token, against the restatement
    m8.reset_cache(max_seq=128)
    m8.forward(e[:20])
    lc = m8.forward(e[20:36])
    ref.reset_cache()
    ref.forward(e[:20])
    first = []
    for l in range(cfg.layers):                      # the second chunk attends the first one's rows in their dequantised form
        cr, sr = _kv8.quantize_ref(ref.cache[l][:20], cfg.kv_heads)
        first.append((cr, sr))
        ref.cache[l][:20].copy_(_kv8.dequantize_ref(cr, sr).half())
    assert torch.equal(_bits(lc), _bits(ref.forward(e[20:36])))
    for l in range(cfg.layers):
        # rows 0-19 keep the codes of their ONE quantisation (quantising a dequantised row again may pick a smaller scale: its amax has been
        # rounded), rows 20-35 are the quantised form of what the second chunk computed
        cr, sr = _kv8.quantize_ref(ref.cache[l][20:36], cfg.kv_heads)
        cr, sr = torch.cat([first[l][0], cr]), torch.cat([first[l][1], sr])
        assert torch.equal(m8.kv8[l][0][:36].cpu(), cr) and torch.equal(m8.kv8[l][1][:36].cpu(), sr), l
        ref.cache[l][20:36].copy_(_kv8.dequantize_ref(cr[20:], sr[20:]).half())
    want = _restated_token(ref, [], e[36:37], 36, LM.decode_nsplit(128, 36))
    assert torch.equal(_bits(m8.forward(e[36:37])), _bits(want))


def _beams(m, prompt, n_new, num_beams=2):
    """the num_beams branch of generate_with_image_embedding, statement for statement: the prompt prefilled once into a BatchDecoder's slots,
    beam.beam_search driving reorder + step"""
    from streamchat_amd.beam import beam_search
    dec = LM.BatchDecoder(m, [prompt], n_new, replicate=num_beams)
    dec.prepare_steps(n_new)
    seen = []

    def step(tokens, origin):
        dec.reorder(origin)
        seen.append(dec.step(tokens.to(device=m.device, dtype=torch.int32)).clone())
        return seen[-1]
    toks, score = beam_search(dec.logits, step, num_beams, n_new, ())
    return toks, score, torch.stack(seen)


def test_shared_view_batch_decoder_and_beams():
    cfg, m16, m8 = _models("fp16")
    e = _embeds(cfg, 24, seed=5)
    v = m8.shared_view()
    assert v.kv_cache == "fp8" and v.kv8 is None
    a, b = m8.forward(e), v.forward(e)
    assert torch.equal(_bits(a), _bits(b)) and v.kv8[0][0].data_ptr() != m8.kv8[0][0].data_ptr()
    assert torch.equal(_bits(m8.forward(e[:1])), _bits(v.forward(e[:1])))
    # BatchDecoder keeps fp16 caches of its own: the tokens of the fp16-cache model, and the model's mode and cache come back
    prompts = [e[:24], e[:17]]
    t16 = LM.BatchDecoder(m16, prompts, 6).generate(6)
    held = m8.kv8[0][0].data_ptr()
    t8 = LM.BatchDecoder(m8, prompts, 6).generate(6)
    assert t8 == t16 and m8.kv_cache == "fp8" and m8.kv8[0][0].data_ptr() == held and m8.cache[0] is m8._kv_stage
    # two beams: they live in BatchDecoder's own fp16 caches, so the fp8-cache model searches exactly as the fp16-cache model over the same weights
    # does - the same tokens, the same score, the same logits of every beam at every step - and its own mode and fp8 rows are untouched by it
    m8.reset_cache()
    m8.forward(e[:9])                                   # the model holds a prompt of its own in its fp8 cache while the beams run
    held, rows = m8.kv8[0][0].data_ptr(), [(kb[:9].clone(), ks[:9].clone()) for kb, ks in m8.kv8]
    b16, s16, l16 = _beams(m16, e, 7)
    b8, s8, l8 = _beams(m8, e, 7)
    assert len(b16) >= 2 and l16.shape[0] >= 2 and b8 == b16 and s8 == s16 and torch.equal(_bits(l8), _bits(l16))
    assert m8.kv_cache == "fp8" and m8.cache_len == 9 and m8.kv8[0][0].data_ptr() == held and m8.cache[0] is m8._kv_stage
    assert all(torch.equal(kb[:9], a) and torch.equal(ks[:9], b) for (kb, ks), (a, b) in zip(m8.kv8, rows))


def test_entry_point_runs_a_question_with_an_fp8_cache(tmp_path, monkeypatch):
    import json
    import inference_streaming_longva_v2 as E
    real = LM.Qwen2ConfigLite
    monkeypatch.setattr(LM, "Qwen2ConfigLite", lambda **kw: real(**{**kw, "head_dim": 128}))      # (--tiny has head dim 64: the fp8 cache serves 128)
    seen = []
    real_attn = ops.attention_kv8
    monkeypatch.setattr(ops, "attention_kv8", lambda *a, **k: (seen.append(1), real_attn(*a, **k))[1])
    args = E.parse_args(["--video_dir", "none", "--model_name", "none", "--memory_basic_dir", str(tmp_path / "mem"), "--save_file",
                         str(tmp_path / "out.json"), "--annotations", "none", "--language", "en", "--conv-mode", "qwen_1_5", "--synthetic", "1",
                         "--tiny", "--chunk_size", "4", "--num_clusters", "2", "--interval", "3", "--short_window", "6", "--remember_window", "3",
                         "--max_new_tokens", "4", "--multi_modal_memory", "--kv_cache", "fp8"])
    E.run_inference(args)
    out = json.load(open(tmp_path / "out.json"))
    assert len(out) >= 1 and all("predict" in r for r in out) and seen
