"""GPU: direct references for the small ops that only the tiny end-to-end models reach (gather_rows, patchify_f16, the preprocess and
rotary kernels past their grid caps, avgpool_tokens, vit_embed_ln, bert_embed_ln, pool).  Each reference is a float64 restatement of the
ABI comment in include/streamchat_hip.h, written here and not derived from the kernel; shapes are the product widths plus the edges the
tiny models never touch: the NV = 2 / 4 / 8 instantiations of the embed + LayerNorm kernels, the second trip of the grid-stride loops
behind the grid caps, id clamps, ldo > H, len[b] = 0 / > L, r not dividing P.  No bound below was tuned on the kernels' output; the
figures observed on the GPU are printed as `[small-ops] ...`."""
import numpy as np
import pytest
import torch

from streamchat_amd import ops
from tests._guard import Arena, frozen
from tests._tol import assert_close_fp16
from tests.test_gpu_heavy_tail import MASSIVE
from tests.test_gpu_misc import ref_preprocess

pytestmark = pytest.mark.gpu
U = 2.0 ** -24                  # unit roundoff of fp32


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randh(shape, seed, scale=1.0):
    return (torch.randn(shape, device="cuda", generator=_gen(seed)) * scale).half()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ulp16(x):
    """spacing of fp16 at |x| (fp64 tensor): 2^(e - 10) with e = floor(log2 |x|) clamped to the subnormal exponent -14 - exponent and power
    taken from / written to the fp64 bit pattern (no transcendental function: exact)"""
    e = (torch.frexp(x.abs())[1].to(torch.int64) - 1).clamp(min=-14, max=15)
    e = torch.where(x == 0, torch.full_like(e, -14), e)
    return ((e - 10 + 1023) << 52).view(torch.float64)


def _ulp16_distance(a, b):
    """distance of two fp16 tensors in units in the last place, from their bit patterns (sign-magnitude -> a monotonic integer line)"""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (key(a) - key(b)).abs()


# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,H,ldo", [(1, 256, 256), (37, 256, 264), (37, 3584, 3584), (8200, 3584, 3592)])
def test_gather_rows_bit_exact_with_id_edges(rows, H, ldo):
    """sc_gather_rows_f16 / k_gather_rows: out[r] = table[ids[r]]; ids outside [0, vocab) give ZERO rows (-200 is the image sentinel of the
    splice; the kernel treats ids >= vocab the same way - pinned here and stated in the header).  8200 x 3584 is 3.67 M 8-element vectors
    against the grid cap of 8192 x 256 = 2.1 M threads: the second trip of the grid-stride loop.  ldo > H: rows land ldo apart."""
    vocab = 152064
    table = _randh((vocab, H), 1)
    ids = torch.randint(0, vocab, (rows,), device="cuda", generator=_gen(2), dtype=torch.int64)
    edge = [-200, -1, vocab - 1, vocab, 2 ** 31 - 1, 0]
    for i, v in enumerate(edge[:rows]):
        ids[(i * 7919) % rows if rows > 6 else i] = v
    if rows > 6:
        ids[rows - 1] = vocab - 1
        ids[rows - 2] = -200
    ids32 = ids.to(torch.int32)
    a = Arena("cuda")
    out = a.out(rows, H, torch.float16, ld=ldo, tail_rows=8)
    with frozen(ids32, table):
        ops.gather_rows(ids32, table, out=out)
    ok = (ids >= 0) & (ids < vocab)
    ref = torch.where(ok[:, None], table[ids.clamp(0, vocab - 1)], torch.zeros((), dtype=torch.float16, device="cuda"))
    assert torch.equal(_bits(out), _bits(ref))
    assert int((~ok).sum()) >= min(rows, 5) - 1 and float(out[~ok].abs().max()) == 0.0
    a.check("gather_rows")


def _unfold_ref(chw, p):
    n, _, h, w = chw.shape
    return torch.nn.functional.unfold(chw.float(), kernel_size=p, stride=p).transpose(1, 2).reshape(n * (h // p) * (w // p), 3 * p * p).half()


@pytest.mark.parametrize("n,h,w,p,ld", [(97, 336, 336, 14, 608), (2, 56, 56, 14, 592), (3, 28, 42, 14, 640), (2, 32, 48, 8, 192), (2, 56, 56, 14, 640)])
def test_patchify_f16_bit_exact_vs_unfold(n, h, w, p, ld):
    """sc_patchify_f16 / k_patchify_f16 against torch.nn.functional.unfold (column = c p^2 + py p + px), pad columns zero.  97 ViT-L images are
    55872 rows x 76 vectors = 4.25 M against the grid cap of 16384 x 256 = 4.19 M threads (second grid-stride trip); 3 x 8 x 8 = 192 is
    ld = 3 p^2 exactly (no pad); 28 x 42 is non-square."""
    x = _randh((n, 3, h, w), 3)
    with frozen(x):
        out = ops.patchify_f16(x, p, ld)
    w3 = 3 * p * p
    assert torch.equal(_bits(out[:, :w3]), _bits(_unfold_ref(x, p)))
    assert ld == w3 or int(torch.count_nonzero(_bits(out[:, w3:]))) == 0


def test_preprocess_u8_past_the_grid_cap():
    """sc_preprocess_u8 / k_pre_chw: 52 frames of 336 x 336 are 52 x 3 x 14112 = 2.20 M 8-pixel groups against 8192 x 256 = 2.10 M threads;
    bit-exact against the numpy restatement of HF's rescale + normalize used for the small shapes (test_gpu_misc.ref_preprocess)."""
    u8 = np.random.default_rng(11).integers(0, 256, (52, 336, 336, 3), dtype=np.uint8)
    out = ops.preprocess_u8(torch.from_numpy(u8).cuda())
    assert np.array_equal(out.cpu().numpy().view(np.uint16), ref_preprocess(u8).view(np.uint16))


def test_preprocess_patchify_u8_past_the_grid_cap():
    """sc_preprocess_patchify_u8 / k_pre_patch: 97 frames -> 55872 rows x 76 vectors = 4.25 M against 16384 x 256 = 4.19 M threads"""
    n, P, ld = 97, 14, 608
    u8 = np.random.default_rng(12).integers(0, 256, (n, 336, 336, 3), dtype=np.uint8)
    out = ops.preprocess_patchify_u8(torch.from_numpy(u8).cuda(), P, ld).cpu()
    ref = _unfold_ref(torch.from_numpy(ref_preprocess(u8)), P)
    assert torch.equal(_bits(out[:, :588]), _bits(ref)) and int(torch.count_nonzero(_bits(out[:, 588:]))) == 0


def _rope_fma_ref(x, tab_rows, heads, Dh):
    """the kernels' documented arithmetic, restated through fp64: lo' = fl32(fma(-hi, sin, fl32(lo cos))), hi' = fl32(fma(lo, sin, fl32(hi cos))),
    then ONE rounding to fp16.  Products of two fp32 numbers are exact in fp64.  x holds fp16-representable values, so that the fp64 sum
    of the fma is exact as well for all but vanishing sines and the double rounding fp64 -> fp32 cannot differ from the single one."""
    rows, half = x.shape[0], Dh // 2
    xr = x[:, :heads * Dh].double().view(rows, heads, Dh)
    lo, hi = xr[..., :half], xr[..., half:]
    cs, sn = tab_rows[:, None, 0].double(), tab_rows[:, None, 1].double()
    ra = ((lo * cs).float().double() - hi * sn).float()
    rb = ((hi * cs).float().double() + lo * sn).float()
    return torch.cat([ra, rb], -1).half().view(rows, heads * Dh)


def test_rope_f32in_past_the_grid_cap():
    """sc_rope_f32in_f16 / k_rope_f32in: 9500 rows x 28 heads x 16 vector pairs = 4.26 M work items against 16384 x 256 = 4.19 M threads"""
    rows, heads, Dh = 9500, 28, 128
    x = _randh((rows, heads * Dh), 5, 3.0).float()
    tab = ops.rope_table(rows + 100, Dh, 1e6, 1.0, "cuda:0")
    with frozen(x):
        out = ops.rope_f32in(x, tab, heads, Dh, torch.empty((rows, heads * Dh), dtype=torch.float16, device="cuda"), 0, 100)
    ref = torch.cat([_rope_fma_ref(x[i:i + 2500], tab[100 + i:100 + min(i + 2500, rows)], heads, Dh) for i in range(0, rows, 2500)])
    assert torch.equal(_bits(out), _bits(ref))


def test_rope_qkv_rows_past_the_grid_cap():
    """sc_rope_qkv_rows_f16 / k_rope_qkv_rows: B = 2048 sequences at the Qwen2-7B heads (28 q, 4 kv, Dh 128): 2048 x (32 x 16 + 128) = 1.31 M work
    items against 4096 x 256 = 1.05 M threads.  q rows and the appended cache rows against the fma restatement; all other cache rows keep
    their bits."""
    B, Hq, Hkv, Dh, cap = 2048, 28, 4, 128, 6
    dq, dkv = Hq * Dh, Hkv * Dh
    x = _randh((B, dq + 2 * dkv), 6, 3.0).float()
    tq, tk = ops.rope_table(64, Dh, 1e6, Dh ** -0.5 * ops.LOG2E, "cuda:0"), ops.rope_table(64, Dh, 1e6, 1.0, "cuda:0")
    rows = min(tq.shape[0], tk.shape[0])                              # (the cached tables grow independently; the ABI takes one row count)
    tq, tk = tq[:rows], tk[:rows]
    pos = torch.randint(0, cap, (B,), device="cuda", generator=_gen(7), dtype=torch.int32)
    cache = torch.full((B, cap, 2 * dkv), 7.0, dtype=torch.float16, device="cuda")
    q = torch.empty((B, dq), dtype=torch.float16, device="cuda")
    with frozen(x, pos):
        ops.rope_qkv_rows(x, tq, tk, pos, Hq, Hkv, Dh, q, cache)
    p = pos.long()
    assert torch.equal(_bits(q), _bits(_rope_fma_ref(x[:, :dq], tq[p], Hq, Dh)))
    want = torch.full_like(cache, 7.0)
    want[torch.arange(B, device="cuda"), p] = torch.cat([_rope_fma_ref(x[:, dq:dq + dkv], tk[p], Hkv, Dh), x[:, dq + dkv:].half()], 1)
    assert torch.equal(_bits(cache), _bits(want))


@pytest.mark.parametrize("r", [1, 2, 4, 5, 24])
def test_avgpool_tokens_vs_fp64_mean(r):
    """sc_avgpool_tokens_f16 at P 24 / D 3584 (the LongVA token map): fp16(fp64 mean) up to where the fp32 accumulation moves the rounding -
    at most 1 fp16 ulp anywhere and >= 99.9 % of the elements exact.  r = 5 does not divide 24: floor, like avg_pool2d (rows / columns 20..23
    dropped); r = 1 is a copy; r = P one token per image."""
    B, P, D = 2, 24, 3584
    x = _randh((B, P * P, D), 8)
    with frozen(x):
        out = ops.avgpool_tokens(x, r)
    g = P // r
    ref64 = x.double().view(B, P, P, D)[:, :g * r, :g * r].reshape(B, g, r, g, r, D).mean(dim=(2, 4)).reshape(B, g * g, D)
    assert out.shape == (B, g * g, D)
    ref = ref64.half()
    exact = float((_bits(out) == _bits(ref)).double().mean())
    worst = int(_ulp16_distance(out, ref).max())
    print(f"\n[small-ops] avgpool_tokens r={r}: {100 * exact:.4f} % exact, largest difference {worst} ulp16")
    assert worst <= 1 and exact >= 0.999, (r, exact, worst)
    if r == 1:
        assert torch.equal(_bits(out), _bits(x))


# ------------------------------------------------------------------------------------------------------------------------------------
def _ln_bound_check(out, v64, gamma, beta, eps, what, mean_term=False, depth=0):
    """LayerNorm over the last dim of v64 (fp64, the exactly known pre-norm values) against the kernel's fp16 output.  Per element:
        |out - ref| <= 0.5 ulp16(ref) + 8 * 2^-24 * (|n g| + |b|)          n = the normalised value
    (the fp16 output rounding plus a few fp32 roundings).  mean_term (inputs with a large common offset only): the term above knows nothing
    of the rounding of the fp32 MEAN, which is relative to |mean|, not to |v - mean|.  A summation of `depth` dependent additions has
    |err(sum)| <= depth * 2^-24 * sum|v| (first-order standard bound), the division adds one rounding: the mean is off by at most
    (depth + 1) * 2^-24 * mean|v|, and n * g by that times rstd * |g|.  Added to the bound for those inputs, from this arithmetic alone."""
    g, b = gamma.double(), beta.double()
    mu = v64.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((v64 - mu) ** 2).mean(-1, keepdim=True) + eps)
    n = (v64 - mu) * rstd
    ref = n * g + b
    bound = 0.5 * _ulp16(ref) + 8 * U * ((n * g).abs() + b.abs())
    if mean_term:
        bound = bound + (depth + 1) * U * v64.abs().mean(-1, keepdim=True) * rstd * g.abs()
    err = (out.double() - ref).abs()
    ratio = float((err / bound).max())
    print(f"\n[small-ops] {what}: max |err| / bound {ratio:.3f}, max |err| {float(err.max()):.3e}")
    assert torch.isfinite(out).all() and ratio <= 1.0, (what, ratio)
    return ref


def _ln_params(D, seed):
    return (1 + _randh((D,), seed, 0.1).float()).half(), _randh((D,), seed + 1, 0.1)


def _heavy(x, offset):
    """the recipe of tests/test_gpu_heavy_tail.py on one tensor [rows, D]: massive channels in every row, a sink row x 30, plus a large
    common offset (where a one-pass variance E[x^2] - E[x]^2 cancels; the kernels are two-pass)"""
    x = x.float() + offset
    cols = [c % x.shape[1] for c in MASSIVE]
    x[:, cols] += torch.tensor([350.0, -500.0, 800.0], device=x.device)
    x[0] *= 30.0
    return x.half()


def _heavy_gains(D, seed):
    g, b = _ln_params(D, seed)
    g = g.float()
    g[[c % D for c in MASSIVE]] = 0.04
    idx = torch.randperm(D, device="cuda", generator=_gen(seed + 2))[:12]
    g[idx] = 4.0 + 8.0 * torch.rand(12, device="cuda", generator=_gen(seed + 3))
    return g.half(), b


@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("D,P,N", [(128, 16, 1), (1024, 576, 3), (1280, 16, 5), (4096, 16, 3), (1024, 16, 5)])
def test_vit_embed_ln_vs_fp64(D, P, N, heavy):
    """sc_vit_embed_ln_f16: out[n, 0] = LN(cls + pos[0]), out[n, 1 + p] = LN(patch[n P + p] + pos[1 + p]) with the fp16-rounded sum (HF's fp16
    embeddings), LayerNorm restated in fp64.  D 128 / 1024 / 1280 / 4096 are k_vit_embed_ln<1 / 2 / 4 / 8> (1280 leaves the last vector group of
    NV = 4 partial); N (P + 1) is 17, 1731, 85, 51, 85 rows - never a multiple of the 4 rows of a workgroup.  The cls row must be token 0 of
    EVERY image and the position row the token index (not the row index): N > 1 with distinct pos rows tells.  heavy: massive channels, a
    sink row and a common offset of 40 (see _ln_bound_check for the one term the bound gains there)."""
    patch, cls, pos = _randh((N * P, D), 21), _randh((D,), 22), _randh((P + 1, D), 23, 0.5)
    g, b = _ln_params(D, 24)
    if heavy:
        patch, cls, (g, b) = _heavy(patch, 40.0), _heavy(cls[None], 40.0)[0].contiguous(), _heavy_gains(D, 27)
    with frozen(patch, cls, pos, g, b):
        out = ops.vit_embed_ln(patch, cls, pos, g, b, 1e-5, N, P)
    tok = torch.cat([cls.expand(N, 1, D), patch.view(N, P, D)], 1)                 # [N, P + 1, D]
    v = (tok + pos[None]).double().view(N * (P + 1), D)                            # fp16 add, rounded to fp16: the documented behaviour
    nv = {128: 1, 1024: 2, 1280: 4, 4096: 8}[D]
    ref = _ln_bound_check(out, v, g, b, 1e-5, f"vit_embed_ln D={D} P={P} N={N} heavy={heavy}", mean_term=heavy, depth=8 * nv + 6)
    assert_close_fp16(out, ref, what=f"vit_embed_ln D={D} heavy={heavy}")


@pytest.mark.parametrize("heavy", [False, True])
@pytest.mark.parametrize("H,L,B", [(128, 11, 1), (384, 64, 9), (1024, 512, 1), (1024, 11, 9), (384, 512, 9)])
def test_bert_embed_ln_vs_fp64(H, L, B, heavy):
    """sc_bert_embed_ln_f16: out[b L + t] = LN(word[ids[b, t]] + type0 + pos[t]), the sum in fp32 in that order, LayerNorm restated in fp64 on
    that fp32 sum.  H 128 / 384 are k_bert_embed_ln<1> (384: partial vector group), 1024 is <2>; B L is 11, 576, 512, 99, 4608 rows.
    ids < 0 and ids >= vocab CLAMP to rows 0 and vocab - 1 (pinned; HF would raise); the position row is t = row % L for B > 1."""
    vocab = 30522
    word, pos, type0 = _randh((vocab, H), 31), _randh((512, H), 32, 0.5), _randh((H,), 33, 0.5)
    g, b = _ln_params(H, 34)
    if heavy:
        word, (g, b) = _heavy(word, 40.0), _heavy_gains(H, 36)
    ids = torch.randint(0, vocab, (B, L), device="cuda", generator=_gen(37), dtype=torch.int64)
    flat = ids.view(-1)
    flat[0], flat[-1], flat[B * L // 2] = -5, vocab + 7, vocab - 1
    if B * L > 8:
        flat[3], flat[5] = vocab, -(2 ** 31)
    ids32 = ids.to(torch.int32)
    with frozen(ids32, word, pos, type0, g, b):
        out = ops.bert_embed_ln(ids32, word, pos, type0, g, b, 1e-12)
    t = torch.arange(B * L, device="cuda") % L
    v = ((word[flat.clamp(0, vocab - 1)].float() + type0.float()) + pos[t].float()).double()
    ref = _ln_bound_check(out, v, g, b, 1e-12, f"bert_embed_ln H={H} L={L} B={B} heavy={heavy}", mean_term=heavy, depth=8 * ((H + 511) // 512) + 6)
    assert_close_fp16(out, ref, what=f"bert_embed_ln H={H} heavy={heavy}")


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("mode", ["cls", "mean"])
@pytest.mark.parametrize("H,L,B", [(384, 1, 1), (384, 64, 9), (1024, 512, 9), (1024, 64, 1)])
def test_pool_vs_fp64(H, L, B, mode, normalize):
    """sc_pool_f16: mode 0 the CLS row, mode 1 the mean over the first min(len[b], L) tokens (len NULL = L; len 0 gives zeros: pinned), optional
    L2 normalisation out / max(||out||, 1e-12): an all-zero row stays zero, never NaN.  fp32 output against fp64.  Sequential fp32 sum of n
    terms and one division: |err(mean)| <= gamma_n * sum|h| / n + 2^-24 |mean| with gamma_n = n u / (1 - n u) (inside the L * 2^-24 * sum|h| of the
    task, n <= L).  After normalisation the error of every component also moves the norm: |err| <= E_i / ||m|| + |ref_i| (||E|| / ||m|| + 2^-22)."""
    hidden = _randh((B, L, H), 41)
    if B > 2:
        hidden[2] = 0                                                  # all-zero row
    cases = [None]
    if B > 1:
        ln = torch.tensor(([0, 1, L, L + 5] * B)[:B], dtype=torch.int32, device="cuda")
        ln[B - 1] = max(1, L // 3)
        cases.append(ln)
    for lengths in cases:
        with frozen(hidden, lengths):
            out = ops.pool(hidden, lengths, mode, normalize)
        h = hidden.double()
        if mode == "cls":
            ref, E = h[:, 0], torch.zeros((B, H), dtype=torch.float64, device="cuda")
        else:
            n = torch.full((B,), L, device="cuda") if lengths is None else lengths.clamp(max=L).long()
            keep = (torch.arange(L, device="cuda")[None] < n[:, None]).double()[..., None]
            nn_ = n.clamp(min=1).double()[:, None]
            ref = (h * keep).sum(1) / nn_
            gam = (n.double() * U / (1 - n.double() * U))[:, None]
            E = gam * (h.abs() * keep).sum(1) / nn_ + U * ref.abs()
        if normalize:
            nrm = ref.norm(dim=1, keepdim=True).clamp(min=1e-12)
            E = E / nrm + (ref / nrm).abs() * (E.norm(dim=1, keepdim=True) / nrm + 2.0 ** -22)
            ref = ref / nrm
        err = (out.double() - ref).abs()
        slack = float((err - E).max())
        print(f"\n[small-ops] pool H={H} L={L} B={B} {mode} normalize={normalize} lengths={'None' if lengths is None else 'edges'}: "
              f"max |err| {float(err.max()):.3e}, max (|err| - bound) {slack:.3e}")
        assert out.dtype == torch.float32 and torch.isfinite(out).all()
        assert bool((err <= E).all()), (mode, normalize, float(err.max()), slack)
        if B > 2:
            assert float(out[2].abs().max()) == 0.0                    # the all-zero row: 0, not NaN
        if lengths is not None and mode == "mean":
            assert float(out[0].abs().max()) == 0.0                    # len 0
