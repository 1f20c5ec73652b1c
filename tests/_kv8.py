"""The FP8 (e4m3) KV-cache format on the CPU (include/streamchat_hip_kv8.h), next to tests/_w8.py: the SPECIFICATION of sc_kv8_quantize_rows in
torch, its inverse, generated caches for the attention tests and an fp64 decode attention over a (de)quantised cache with the wrong readings a
broken kernel could take (tests/test_kv8_cpu.py shows that the GPU tests' comparison rejects each of them).  Everything comes from a seed on the
CPU, so the GPU tests and the CPU tests see the same numbers."""
import torch

from tests import _w8

DH = 128
E_MIN, E_MAX = -14, 7


def quantize_ref(x, kv_heads):
    """fp16 [n, 2 * kv_heads * 128] -> (bytes uint8 [n, 2 * kv_heads * 128], scales fp32 [n, 2 * kv_heads]): one power-of-two scale per
    128-element segment, e the smallest integer with 448 * 2^e >= amax, clamped to [-14, 7] (0 for an all-zero segment)"""
    n = x.shape[0]
    xs = x.cpu().float().view(n, 2 * kv_heads, DH)
    amax = xs.abs().amax(dim=2)
    m, e = torch.frexp(amax / 448)
    e = torch.where(m == 0.5, e - 1, e)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp(E_MIN, E_MAX)
    scale = torch.exp2(e.float())
    codes = (xs / scale[:, :, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    return codes.view(n, 2 * kv_heads * DH), scale


def dequantize_ref(codes, scale, values=_w8.e4m3_values):
    """fp64 code * scale, [n, 2 * kv_heads * 128]"""
    n, nseg = scale.shape
    return (values(codes.cpu()).view(n, nseg, DH) * scale.cpu().double()[:, :, None]).view(n, nseg * DH)


def edge_rows(kv_heads):
    """fp16 [5, 2 * kv_heads * 128], every segment of row i the i-th edge: all zero | one element of 65504 | amax below 448 * 2^-14 | amax exactly
    448 * 2^k (k = -3) | a -0.0 among small values"""
    g = _w8.gen(77)
    x = torch.zeros(5, 2 * kv_heads, DH)
    x[1] = torch.randn(2 * kv_heads, DH, generator=g) * 100
    x[1, :, 5] = 65504.0
    x[2] = torch.randn(2 * kv_heads, DH, generator=g).clamp(-3, 3) * 2e-3                 # |x| <= 6e-3 < 448 * 2^-14 = 0.0273
    x[3] = (torch.rand(2 * kv_heads, DH, generator=g) * 2 - 1) * 50
    x[3, :, 9] = -56.0                                                                      # 448 * 2^-3
    x[4] = torch.randn(2 * kv_heads, DH, generator=g)
    x = x.half()
    x[4, :, 3] = -0.0
    return x.view(5, 2 * kv_heads * DH)


def random_rows(n, kv_heads, seed):
    """fp16 rows whose segments have sigma spread over 2^-12 .. 2^10"""
    g = _w8.gen(seed)
    sig = torch.exp2(torch.randint(-12, 11, (n, 2 * kv_heads, 1), generator=g).float())
    return (torch.randn(n, 2 * kv_heads, DH, generator=g) * sig).half().view(n, 2 * kv_heads * DH)


def random_cache(S, kv_heads, seed):
    """(bytes uint8 [S, 2 * kv_heads * 128] drawn over all 254 finite codes, scales fp32 [S, 2 * kv_heads] = 2^e with e uniform in [-14, 7],
    independent per row, head and K / V)"""
    g = _w8.gen(seed)
    codes = _w8.FINITE[torch.randint(0, 254, (S, 2 * kv_heads * DH), generator=g)]
    e = torch.randint(E_MIN, E_MAX + 1, (S, 2 * kv_heads), generator=g)
    return codes, torch.exp2(e.float())


def attention_case(S, G, kv_heads, seed):
    """codes, scales and a pre-scaled q fp16 [G, kv_heads * 128] (row g, head h = query row g of KV head h).  The logits of random codes with
    scales up to 2^7 are huge, so q is small (logit sigma of about 8 in log2 units): the softmax still spreads over several keys."""
    codes, scale = random_cache(S, kv_heads, seed)
    q = (torch.randn(G, kv_heads * DH, generator=_w8.gen(seed + 1)) * 1e-4).half()
    return codes, scale, q


# (S, G, nsplit) of tests/golden/decode_attention_bits.npz (tools/make_golden_decode_bits.py records it, tests/test_gpu_kv8.py reads it), the
# smallest shapes at which each piece that the two decode attention kernels share can go wrong: one partial chunk with empty waves and an empty
# split | a chunk boundary with a one-row masked tail and Sq < 16 | more splits than chunks | uneven chunk shares across waves and splits
# (twice) | the production split rule (None: llm.decode_nsplit(128, S)).  Hkv = 2, q pre-scaled, inputs from decode_bits_inputs.
DECODE_BITS_CASES = [(1, 1, 2), (33, 7, 2), (33, 16, 5), (769, 1, 3), (769, 16, 5), (2273, 7, None)]


def decode_bits_inputs(S, G):
    """(codes, scale, q, crc): the generated inputs of one DECODE_BITS_CASES case and the CRC32 of their bytes"""
    import zlib
    codes, scale, q = attention_case(S, G, 2, seed=100 + S + G)
    crc = 0
    for t in (codes, scale, q):
        crc = zlib.crc32(t.contiguous().numpy().tobytes(), crc)
    return codes, scale, q, crc


def attention_fp64(q, codes, scale, kv_heads, kv_len=None, values=_w8.e4m3_values, scale_k=None, scale_v=None):
    """fp64 decode attention of pre-scaled q (logits in log2 units, as the kernels take them) over the dequantised cache -> [G, kv_heads * 128].
    `values`, `scale_k`, `scale_v` ([S, kv_heads] each): what a WRONG kernel would use; kv_len: rows past it are masked."""
    S = codes.shape[0] if kv_len is None else kv_len
    sk = (scale[:, :kv_heads] if scale_k is None else scale_k).double()
    sv = (scale[:, kv_heads:] if scale_v is None else scale_v).double()
    vals = values(codes).view(codes.shape[0], 2 * kv_heads, DH)
    K, V = vals[:S, :kv_heads] * sk[:S, :, None], vals[:S, kv_heads:] * sv[:S, :, None]
    qh = q.double().view(-1, kv_heads, DH)
    p = torch.softmax(torch.einsum("ghd,shd->hgs", qh, K) * 0.6931471805599453, dim=-1)
    return torch.einsum("hgs,shd->ghd", p, V).reshape(q.shape[0], kv_heads * DH)


def same_bits(a, b):
    """THE comparison of the GPU attention tests: fp16 results equal bit for bit"""
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))
