"""GPU: the FP8 (e4m3) KV cache of the BATCHED decode (include/streamchat_hip_kv8_batched.h, attention_kv8.hip, llm.BatchDecoder(kv_cache="fp8")).
sc_attention_kv8_batched equals, for every sequence, the batch-1 kernel on that sequence's slice and, as a whole, the fp16 batched decode attention on
the dequantised caches, bit for bit; a sequence reads only its own valid rows; batch offsets are 64-bit; sc_kv8_rope_qkv_rows equals the fp16 rope
followed by the CPU specification of the quantiser and writes only its rows; an fp8 BatchDecoder (eager, from a captured graph, under beam search)
has the bits of a restated fp16 run whose cache rows pass through quantise -> dequantise; the defaults hold; the entry point takes the flag."""
import contextlib
import functools

import pytest
import torch

from streamchat_amd import llm as LM, ops
from tests import _kv8, _w8
from tests._guard import Arena, frozen

pytestmark = pytest.mark.gpu
DH = 128
HKV, B4, CAP = 2, 4, 800
KV_LEN = [1, 33, 769, 800]          # one chunk | a chunk boundary + 1 | a 24-chunk boundary + 1 | a full slice


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()]).cpu()


# ---- attention
@functools.lru_cache(maxsize=None)
def _case(G):
    """B4 slices of CAP rows, generated once per G and left unchanged: (codes [B, CAP, w] uint8, scales [B, CAP, 2 Hkv], q [B, G, Hkv * 128] fp16, all
    on the CPU; the fp64 attention of every sequence over its KV_LEN[b] valid rows)"""
    parts = [_kv8.attention_case(CAP, G, HKV, seed=500 + 10 * b + G) for b in range(B4)]
    codes, scale, q = (torch.stack([p[i] for p in parts]) for i in range(3))
    ref = [_kv8.attention_fp64(q[b], codes[b], scale[b], HKV, kv_len=KV_LEN[b]) for b in range(B4)]
    return codes, scale, q, ref


def _q_views(q, packed):
    """q [B, G, Hkv * 128] (query row g of KV head h at g * Hkv * 128 + h * 128) on the device, as the (tensor, strides) the calls take: as it is, or
    head-packed as BatchDecoder.step holds it - [B, Hq * 128] with query head h * G + g, addressed as G rows of stride 128 with head stride G * 128
    and batch stride Hq * 128"""
    Bn, G = q.shape[0], q.shape[1]
    if not packed:
        return q.cuda(), dict()
    flat = q.view(Bn, G, HKV, DH).permute(0, 2, 1, 3).reshape(Bn, HKV * G * DH).contiguous().cuda()
    return flat.as_strided((Bn, G, DH), (HKV * G * DH, DH, 1)), dict(q_head_stride=G * DH, o_head_stride=G * DH, out_ld=DH)


def _canonical(out, packed):
    """the result as [B, G, Hkv * 128] whichever addressing produced it"""
    if not packed:
        return out
    Bn, G = out.shape[0], out.shape[1]
    return out.reshape(Bn, HKV, G, DH).permute(0, 2, 1, 3).reshape(Bn, G, HKV * DH)


def _batched(codes, scale, q, kv_len, nsplit, packed):
    qd, kw = _q_views(q, packed)
    kl = torch.tensor(kv_len, dtype=torch.int32, device="cuda")
    out = ops.attention_kv8_batched(qd, codes.cuda(), scale.cuda(), HKV, DH, DH ** -0.5, kv_len=kl, nsplit=nsplit, q_prescaled=True, **kw)
    return _canonical(out, packed)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("G", [1, 7, 16])
def test_batched_attention_equals_the_batch1_kernel_and_the_fp16_kernel_on_the_dequantised_caches(G, packed):
    codes, scale, q, ref = _case(G)
    w, dkv = 2 * HKV * DH, HKV * DH
    deq = torch.stack([_kv8.dequantize_ref(codes[b], scale[b]).half() for b in range(B4)]).cuda()
    cd, sd = codes.cuda(), scale.cuda()
    kl = torch.tensor(KV_LEN, dtype=torch.int32, device="cuda")
    for nsplit in (2, 3, 5):
        assert ops.attention_variant(DH, G, nsplit) == 3
        got = _batched(codes, scale, q, KV_LEN, nsplit, packed)
        # the fp16 batched decode attention, same nsplit, same kv_len, same q addressing
        qd, kw = _q_views(q, packed)
        f16 = _canonical(ops.attention(qd, deq[:, :, :dkv], deq[:, :, dkv:], HKV, HKV, DH, DH ** -0.5, causal=False, kv_len=kl, nsplit=nsplit,
                                       q_prescaled=True, **kw), packed)
        assert _kv8.same_bits(got, f16), f"G={G} nsplit={nsplit} packed={packed}: {int((got != f16).sum())} of {got.numel()} elements differ from the fp16 kernel"
        for b in range(B4):
            qb, kwb = _q_views(q[b:b + 1], packed)
            one = _canonical(ops.attention_kv8(qb, cd[b], sd[b], HKV, DH, DH ** -0.5, kv_len=kl[b:b + 1], nsplit=nsplit, q_prescaled=True, **kwb), packed)
            assert _kv8.same_bits(got[b], one[0]), f"G={G} nsplit={nsplit} packed={packed}: sequence {b} differs from the batch-1 kernel on its slice"
            a = got[b].cpu().double()
            assert bool(torch.isfinite(got[b]).all()) and ((a - ref[b]).abs().max() / ref[b].abs().max()).item() < 2e-2, (b, nsplit)
    assert w == codes.shape[2]


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("G", [1, 7, 16])
def test_a_sequence_reads_only_its_own_valid_rows(G, packed):
    """rows at and behind kv_len[b] are 0x7F (NaN) bytes with NaN scales in every slice: the same bits as with clean tails.  A sequence with
    kv_len = 0 gives a finite row and leaves the others as they were."""
    codes, scale, q, _ = _case(G)
    pc, ps = codes.clone(), scale.clone()
    for b, n in enumerate(KV_LEN):
        pc[b, n:], ps[b, n:] = 0x7F, float("nan")
    for nsplit in (2, 3, 5):
        clean = _batched(codes, scale, q, KV_LEN, nsplit, packed)
        poisoned = _batched(pc, ps, q, KV_LEN, nsplit, packed)
        assert bool(torch.isfinite(poisoned).all()) and _kv8.same_bits(poisoned, clean), nsplit
        kv0 = [0] + KV_LEN[1:]
        pc0, ps0 = pc.clone(), ps.clone()
        pc0[0], ps0[0] = 0x7F, float("nan")                 # nothing of sequence 0 is valid any more
        empty = _batched(pc0, ps0, q, kv0, nsplit, packed)
        assert bool(torch.isfinite(empty).all()) and _kv8.same_bits(empty[1:], clean[1:]), nsplit


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("G", [1, 7, 16])
def test_one_split_equals_the_batch1_kernel(G, packed):
    """ONE split is what the unchanged split rule picks for short batches, and there sc_attention_f16 runs its tile kernel: no fp16 bits to compare
    with.  The batched call still equals the batch-1 kernel on every slice bit for bit, and both are an attention (fp64, the 2e-2 bound)."""
    codes, scale, q, ref = _case(G)
    cd, sd = codes.cuda(), scale.cuda()
    kl = torch.tensor(KV_LEN, dtype=torch.int32, device="cuda")
    got = _batched(codes, scale, q, KV_LEN, 1, packed)
    for b in range(B4):
        qb, kwb = _q_views(q[b:b + 1], packed)
        one = _canonical(ops.attention_kv8(qb, cd[b], sd[b], HKV, DH, DH ** -0.5, kv_len=kl[b:b + 1], nsplit=1, q_prescaled=True, **kwb), packed)
        assert _kv8.same_bits(got[b], one[0]), f"G={G} packed={packed}: sequence {b} differs from the batch-1 kernel on its slice"
        assert bool(torch.isfinite(got[b]).all()) and ((got[b].cpu().double() - ref[b]).abs().max() / ref[b].abs().max()).item() < 2e-2, b


def test_batch_offsets_are_64_bit():
    """one slice is just over 1 GiB, so sequence 2 starts beyond 2^31 bytes (one allocation of ~3 GiB, touched sparsely: 100 rows per sequence)"""
    Hkv, G, Bn, rows, nsplit = 1, 7, 3, 100, 2
    w = 2 * Hkv * DH
    cap = (1 << 30) // w + 64
    assert cap * w > (1 << 30) and 2 * cap * w > (1 << 31) and cap * w < (1 << 31)
    cache = torch.empty((Bn, cap, w), dtype=torch.uint8, device="cuda")
    scales = torch.empty((Bn, cap, 2 * Hkv), dtype=torch.float32, device="cuda")
    small = [_kv8.attention_case(rows, G, Hkv, seed=900 + b) for b in range(Bn)]
    for b, (c, s, _) in enumerate(small):
        cache[b, :rows].copy_(c)
        scales[b, :rows].copy_(s)
    q = torch.stack([p[2] for p in small]).cuda()                          # [B, G, 128]
    kl = torch.full((Bn,), rows, dtype=torch.int32, device="cuda")
    got = ops.attention_kv8_batched(q, cache, scales, Hkv, DH, DH ** -0.5, kv_len=kl, nsplit=nsplit, q_prescaled=True)
    for b, (c, s, qb) in enumerate(small):
        one = ops.attention_kv8(qb.cuda().unsqueeze(0), c.cuda(), s.cuda(), Hkv, DH, DH ** -0.5, nsplit=nsplit, q_prescaled=True)
        ref = _kv8.attention_fp64(qb, c, s, Hkv)
        assert _kv8.same_bits(got[b], one[0]), f"sequence {b} (byte offset {b * cap * w}) differs from the batch-1 call on a copy of its rows"
        assert ((got[b].cpu().double() - ref).abs().max() / ref.abs().max()).item() < 2e-2
    del cache, scales
    torch.cuda.empty_cache()


# ---- rotary + quantised append
@pytest.mark.parametrize("Hkv", [1, 2])
def test_rope_and_quantised_append_equals_the_fp16_rope_then_the_cpu_specification(Hkv):
    Bn, Hq, cap, tab_rows = 5, 4, 64, 66
    w, width = 2 * Hkv * DH, (Hq + 2 * Hkv) * DH
    pos_host = [0, 1, 37, cap - 1, cap + 5]          # the last one is clamped: cache row cap - 1, table row tab_rows - 1, as the fp16 kernel clamps
    g = _w8.gen(40 + Hkv)
    sig = torch.exp2(torch.randint(-12, 11, (Bn, Hq + 2 * Hkv, 1), generator=g).float())
    x = (torch.randn(Bn, Hq + 2 * Hkv, DH, generator=g) * sig)
    k0, v0 = Hq, Hq + Hkv
    x[0, k0] = 0.0                                                          # an all-zero K head: scale 1, codes 0
    x[1, v0] = torch.randn(DH, generator=g).clamp(-3, 3) * 2e-3             # amax <= 6e-3 < 448 * 2^-14: e = -14
    x[2, v0] = torch.randn(DH, generator=g) * 100
    x[2, v0, 5] = 40000.0                                                   # 448 * 2^6 < amax <= 448 * 2^7: e = 7
    x[3, k0] = torch.randn(DH, generator=g) * 10
    x[3, k0, 3], x[3, k0, 67] = 30000.0, -30000.0                           # a rotary pair whose rotated magnitude stays below 65504: e = 6 or 7
    x = x.view(Bn, width).cuda()
    tq, tk = ops.rope_table(tab_rows, DH, 1e6, DH ** -0.5 * ops.LOG2E, "cuda"), ops.rope_table(tab_rows, DH, 1e6, 1.0, "cuda")
    pos = torch.tensor(pos_host, dtype=torch.int32, device="cuda")
    # the fp16 kernel into an fp16 cache, then the CPU specification of the quantiser on the rows it wrote
    q_ref = torch.zeros((Bn, Hq * DH), dtype=torch.float16, device="cuda")
    c16 = torch.zeros((Bn, cap, w), dtype=torch.float16, device="cuda")
    ops.rope_qkv_rows(x, tq, tk, pos, Hq, Hkv, DH, q_ref, c16)
    rows = [min(max(p, 0), cap - 1) for p in pos_host]
    want = [_kv8.quantize_ref(c16[b, r:r + 1], Hkv) for b, r in enumerate(rows)]
    all_scales = torch.cat([s.view(-1) for _, s in want])
    assert 2.0 ** -14 in all_scales and 2.0 ** 7 in all_scales and want[0][1][0, 0] == 1.0 and not want[0][0][0, :DH].any()      # the edges are there
    ar = Arena("cuda")
    q_out = ar.out(Bn, Hq * DH, torch.float16, ld=Hq * DH + 64, tail_rows=16)
    cache = ar.out(Bn * cap, w, torch.uint8, ld=w + 128, tail_rows=64).view(Bn, cap, w)
    scales = ar.out(Bn * cap, 2 * Hkv, torch.float32, tail_rows=64).view(Bn, cap, 2 * Hkv)
    q_out.fill_(0.5); cache.fill_(0x11); scales.fill_(3.0)
    with frozen(x, tq, tk, pos):
        ret = ops.kv8_rope_qkv_rows(x, tq, tk, pos, Hq, Hkv, DH, q_out, cache, scales)
    assert ret is q_out and torch.equal(_bits(q_out), _bits(q_ref))
    keep = torch.ones((Bn, cap), dtype=torch.bool)
    for b, r in enumerate(rows):
        cr, sr = want[b]
        assert torch.equal(cache[b, r:r + 1].cpu(), cr), f"bytes of sequence {b}, row {r}"
        assert torch.equal(_bits(scales[b, r:r + 1]), _bits(sr)), f"scales of sequence {b}, row {r}"
        keep[b, r] = False
    assert bool((cache.cpu()[keep] == 0x11).all()) and bool((scales.cpu()[keep] == 3.0).all())
    ar.check("sc_kv8_rope_qkv_rows")


# ---- the decoder
CFG = dict(hidden=256, layers=3, heads=4, kv_heads=2, intermediate=512, vocab=1024, head_dim=128)
N_NEW = 6
# The batched split rule gives ONE split at these prompt lengths, where sc_attention_f16 serves the fp16 decoder with its tile kernel: the bit
# identity is a statement about the two streaming kernels, so both decoders run them, at two splits (the decoders' own nsplit_override knob).
NSPLIT = 2


def _model(**kw):
    cfg = LM.Qwen2ConfigLite(**CFG)
    return cfg, LM.Qwen2Model(LM.random_qwen2_state_dict(cfg, seed=3, std=0.05), cfg, max_seq=128, **{"kv_cache": "fp16", **kw})


def _embeds(cfg, n, seed):
    return (torch.randn(n, cfg.hidden, generator=_w8.gen(seed)) * 0.5).half().cuda()


def _round_trip(rows, kv_heads):
    """fp16 cache rows [n, w] (device) through the CPU specification: quantise -> dequantise, in place"""
    cr, sr = _kv8.quantize_ref(rows, kv_heads)
    rows.copy_(_kv8.dequantize_ref(cr, sr).half())
    return cr, sr


@contextlib.contextmanager
def _restated_append(monkeypatch):
    """inside the block every row ops.rope_qkv_rows appends to an fp16 batch cache passes through quantise -> dequantise: what an fp16 decoder
    would hold if its new rows were stored in e4m3"""
    real = ops.rope_qkv_rows

    def patched(x32, tab_q, tab_k, positions, q_heads, kv_heads, Dh, q_out, cache):
        q = real(x32, tab_q, tab_k, positions, q_heads, kv_heads, Dh, q_out, cache)
        for b, p in enumerate(positions.cpu().tolist()):
            r = min(max(p, 0), cache.shape[1] - 1)
            _round_trip(cache[b, r:r + 1], kv_heads)
        return q
    with monkeypatch.context() as mp:
        mp.setattr(ops, "rope_qkv_rows", patched)
        yield


def _restated_decoder(m, prompts, replicate=None):
    """an fp16 BatchDecoder whose prefilled rows went through the round trip; also the (bytes, scales) the fp8 decoder's prefill must hold"""
    ref = LM.BatchDecoder(m, prompts, N_NEW, replicate=replicate, kv_cache="fp16")
    ref.nsplit_override = NSPLIT
    held = []
    for cl in ref.cache:
        held.append([_round_trip(cl[b, :int(n)], m.cfg.kv_heads) for b, n in enumerate(ref.len.cpu().tolist())])
    return ref, held


def _record_steps(dec):
    seen, step = [], dec.step
    dec.step = lambda tokens: (seen.append(step(tokens).clone()), seen[-1])[1]
    return seen


def _model_state(m):
    return (m.kv_cache, m.cache, None if m.cache is None else [c.data_ptr() for c in m.cache], m.kv8,
            None if m.kv8 is None else [t.data_ptr() for p in m.kv8 for t in p], m._kv_stage, m.cache_len, m.max_seq, m._nsplit_prompt)


def _same_state(a, b):
    return all(x is y or x == y for x, y in zip(a, b))


def test_decoder_is_bit_exact_against_a_restated_fp16_run(monkeypatch):
    cfg, m16 = _model()
    m8 = m16.shared_view().set_kv_cache("fp8")
    prompts = [_embeds(cfg, 24, 5), _embeds(cfg, 17, 6), _embeds(cfg, 33, 7)]
    Bn = len(prompts)
    # the models hold prompts of their own while the decoders run
    own = _embeds(cfg, 9, 8)
    m16.reset_cache(); m16.forward(own)
    m8.reset_cache(); m8.forward(own)
    rows16 = [c[:9].clone() for c in m16.cache]
    rows8 = [(kb[:9].clone(), ks[:9].clone()) for kb, ks in m8.kv8]
    st16, st8 = _model_state(m16), _model_state(m8)
    # the restated fp16 run, eager
    ref, held = _restated_decoder(m16, prompts)
    ref_steps = _record_steps(ref)
    with _restated_append(monkeypatch):
        ref_tokens = ref.generate(N_NEW, use_graph=False)
    assert ref.nsplit == NSPLIT and len(ref_steps) == N_NEW - 1 and all(len(t) == N_NEW for t in ref_tokens)
    for model, st in ((m16, st16), (m8, st8)):
        # eager
        dec = LM.BatchDecoder(model, prompts, N_NEW, kv_cache="fp8")
        assert dec.kv_cache == "fp8" and dec.cache is None and dec.kv8[0][0].dtype == torch.uint8 and dec.kv8[0][0].shape == (Bn, 33 + N_NEW, 512)
        assert dec.kv8[0][1].shape == (Bn, 33 + N_NEW, 4) and torch.equal(_bits(dec.logits), _bits(ref.logits))
        for l, (kb, ks) in enumerate(dec.kv8):
            for b, (cr, sr) in enumerate(held[l]):
                assert torch.equal(kb[b, :cr.shape[0]].cpu(), cr) and torch.equal(ks[b, :cr.shape[0]].cpu(), sr), (l, b)
        dec.nsplit_override = NSPLIT
        steps = _record_steps(dec)
        tokens = dec.generate(N_NEW, use_graph=False)
        assert tokens == ref_tokens and len(steps) == len(ref_steps)
        for t, (a, b) in enumerate(zip(steps, ref_steps)):
            assert torch.equal(_bits(a), _bits(b)), f"eager step {t}"
        # the step replayed from a captured graph, fed the reference's tokens
        dec = LM.BatchDecoder(model, prompts, N_NEW, kv_cache="fp8")
        dec.nsplit_override = NSPLIT
        dec.prepare_steps(N_NEW)
        tok = torch.zeros(Bn, dtype=torch.int32, device="cuda")
        graph, out = LM._capture_graph(model.device, lambda: dec.step(tok), (dec.len,))
        for t in range(N_NEW - 1):
            tok.copy_(torch.tensor([seq[t] for seq in ref_tokens], dtype=torch.int32))
            graph.replay()
            assert torch.equal(_bits(out), _bits(ref_steps[t])), f"replayed step {t}"
        # generate() captures the fp8 step as it captures the fp16 one
        dec = LM.BatchDecoder(model, prompts, N_NEW, kv_cache="fp8")
        dec.nsplit_override = NSPLIT
        assert dec.generate(N_NEW) == ref_tokens
        # the model's own state is back as it was
        assert _same_state(_model_state(model), st)
    assert m16.kv_cache == "fp16" and m16.kv8 is None and m16._kv_stage is None and m16.cache_len == 9
    assert all(torch.equal(c[:9], r) for c, r in zip(m16.cache, rows16))
    assert m8.kv_cache == "fp8" and m8.cache_len == 9 and all(c is m8._kv_stage for c in m8.cache)
    assert all(torch.equal(kb[:9], a) and torch.equal(ks[:9], b) for (kb, ks), (a, b) in zip(m8.kv8, rows8))
    # the split rule's own choice at these lengths (one split: partials at nsplit = 1 need a workspace too): an attention, close to the two-split run
    dec = LM.BatchDecoder(m16, prompts, N_NEW, kv_cache="fp8")
    steps = _record_steps(dec)
    real_attn, calls = ops.attention_kv8_batched, []

    def checked(q, cache, scales, kv_heads, Dh, scale, kv_len=None, nsplit=1, **kw):
        """every attention launch of the production path: each sequence equals the batch-1 kernel on its slice (same split) bit for bit and the
        fp64 attention over its dequantised valid rows within the 2e-2 bound"""
        out = real_attn(q, cache, scales, kv_heads, Dh, scale, kv_len=kv_len, nsplit=nsplit, **kw)
        G = q.shape[1]
        for b, n in enumerate(kv_len.cpu().tolist()):
            one = ops.attention_kv8(q[b:b + 1], cache[b], scales[b], kv_heads, Dh, scale, kv_len=kv_len[b:b + 1], nsplit=nsplit,
                                    **{k: v for k, v in kw.items() if k != "ws"})
            assert _kv8.same_bits(out[b], one[0]), (len(calls), b)
            qc = q[b].as_strided((kv_heads, G, Dh), (G * Dh, Dh, 1)).permute(1, 0, 2).reshape(G, kv_heads * Dh).cpu()
            want = _kv8.attention_fp64(qc, cache[b].cpu(), scales[b].cpu(), kv_heads, kv_len=n)
            have = out[b].reshape(kv_heads, G, Dh).permute(1, 0, 2).reshape(G, kv_heads * Dh).cpu().double()
            assert ((have - want).abs().max() / want.abs().max()).item() < 2e-2, (len(calls), b)
        calls.append(nsplit)
        return out
    with monkeypatch.context() as mp:
        mp.setattr(ops, "attention_kv8_batched", checked)
        dec.generate(N_NEW, use_graph=False)
    assert dec.nsplit == LM.batched_decode_nsplit(Bn, cfg.kv_heads, 33 + N_NEW) == 1 and calls == [1] * (cfg.layers * (N_NEW - 1))
    # (same inputs at step 0 only: fp16 rounding of the attention output, amplified by three layers; 1e-2 of the logits' range is generous for it
    #  and far below the difference any wrong row or scale makes)
    d = (steps[0] - ref_steps[0]).abs().max() / ref_steps[0].abs().max()
    assert bool(torch.isfinite(steps[0]).all()) and d.item() < 1e-2


def _beams(dec, num_beams):
    """the num_beams branch of generate_with_image_embedding: beam.beam_search driving reorder + step"""
    from streamchat_amd.beam import beam_search
    dec.nsplit_override = NSPLIT
    dec.prepare_steps(N_NEW)
    seen = []

    def step(tokens, origin):
        dec.reorder(origin)
        seen.append(dec.step(tokens.to(device="cuda", dtype=torch.int32)).clone())
        return seen[-1]
    toks, score = beam_search(dec.logits, step, num_beams, N_NEW, ())
    return toks, score, torch.stack(seen)


def test_beams_search_over_fp8_caches_as_the_restated_fp16_run(monkeypatch):
    cfg, m16 = _model()
    prompt = _embeds(cfg, 24, 5)
    ref, _ = _restated_decoder(m16, [prompt], replicate=3)
    with _restated_append(monkeypatch):
        t16, s16, l16 = _beams(ref, 3)
    dec = LM.BatchDecoder(m16, [prompt], N_NEW, replicate=3, kv_cache="fp8")
    assert dec.B == 3 and all(torch.equal(kb[0, :24], kb[i, :24]) and torch.equal(ks[0, :24], ks[i, :24]) for kb, ks in dec.kv8 for i in (1, 2))
    t8, s8, l8 = _beams(dec, 3)
    assert len(t16) >= 2 and l16.shape[0] >= 2 and t8 == t16 and s8 == s16 and torch.equal(_bits(l8), _bits(l16))


def test_defaults_hold():
    cfg, m16 = _model()
    m8 = m16.shared_view().set_kv_cache("fp8")
    prompts = [_embeds(cfg, 12, 1), _embeds(cfg, 7, 2)]
    assert m16.batch_kv_cache == "fp16" and m8.batch_kv_cache == "fp16"
    dec = LM.BatchDecoder(m8, prompts, 4)                                   # an fp8-cache model, nothing asked: fp16 caches
    assert dec.kv_cache == "fp16" and dec.kv8 is None and dec.cache[0].dtype == torch.float16 and dec.cache[0].shape == (2, 16, 512)
    dec = LM.BatchDecoder(m16, prompts, 4, kv_cache="fp8")                  # asked on the decoder
    assert dec.kv_cache == "fp8" and dec.cache is None and dec.kv8[0][0].dtype == torch.uint8
    mb = m16.shared_view().set_batch_kv_cache("fp8")                        # asked on the model; a view inherits it; the argument still wins
    assert mb.kv_cache == "fp16" and mb.shared_view().batch_kv_cache == "fp8" and m16.batch_kv_cache == "fp16"
    assert LM.BatchDecoder(mb, prompts, 4).kv_cache == "fp8" and LM.BatchDecoder(mb, prompts, 4, kv_cache="fp16").kv_cache == "fp16"
    _, mc = _model(batch_kv_cache="fp8")
    assert mc.batch_kv_cache == "fp8" and LM.BatchDecoder(mc, prompts, 4).kv8 is not None
    with pytest.raises(ValueError, match="batch_kv_cache must be one of"):
        LM.BatchDecoder(m16, prompts, 4, kv_cache="int4")
    # head dim 64 is refused before any allocation
    c64 = LM.Qwen2ConfigLite(**{**CFG, "head_dim": 64})
    with pytest.raises(ValueError, match="head_dim 128"):
        LM.Qwen2Model({}, c64, batch_kv_cache="fp8")
    m64 = LM.Qwen2Model(LM.random_qwen2_state_dict(c64, seed=3, std=0.05), c64, max_seq=64)
    with pytest.raises(ValueError, match="head_dim 128"):
        m64.set_batch_kv_cache("fp8")
    p64 = [_embeds(c64, 8, 1)]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="head_dim 128"):
        LM.BatchDecoder(m64, p64, 4, kv_cache="fp8")
    assert torch.cuda.memory_allocated() == before and m64.cache is None and m64.batch_kv_cache == "fp16"


def test_entry_point_captions_with_fp8_batch_caches(tmp_path, monkeypatch):
    import json
    import inference_streaming_longva_v2 as E
    real = LM.Qwen2ConfigLite
    monkeypatch.setattr(LM, "Qwen2ConfigLite", lambda **kw: real(**{**kw, "head_dim": 128}))      # (--tiny has head dim 64: the fp8 cache serves 128)
    seen = []
    real_attn = ops.attention_kv8_batched
    monkeypatch.setattr(ops, "attention_kv8_batched", lambda *a, **k: (seen.append(1), real_attn(*a, **k))[1])
    args = E.parse_args(["--video_dir", "none", "--model_name", "none", "--memory_basic_dir", str(tmp_path / "mem"), "--save_file",
                         str(tmp_path / "out.json"), "--annotations", "none", "--language", "en", "--conv-mode", "qwen_1_5", "--synthetic", "1",
                         "--tiny", "--chunk_size", "4", "--num_clusters", "2", "--interval", "3", "--short_window", "6", "--remember_window", "3",
                         "--max_new_tokens", "4", "--multi_modal_memory", "--batch_captions", "1", "--batch_kv_cache", "fp8"])
    assert args.batch_kv_cache == "fp8" and args.kv_cache == "fp16"
    E.run_inference(args)
    out = json.load(open(tmp_path / "out.json"))
    assert len(out) >= 1 and all("predict" in r for r in out) and seen
