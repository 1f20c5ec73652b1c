"""Attention inputs with structure, an fp64 probe-row reference, a per-row check, wrong references ("mutants") and the case table of the
production call signatures.  Plain torch: runs on the CPU (tests/test_attention_case_power.py proves that the cases can tell a wrong
kernel from a right one) and on the GPU (tests/test_gpu_attention_power.py runs ops.attention on the same cases).

Why: with i.i.d. q / k / v the softmax is flat, the output is a mean of ~S value rows (magnitude 1/sqrt(S)) and an absolute tolerance of
2e-3 is as large as the output at S = 49 k.  The families below put O(1) structure where kernels go wrong, and the check is relative to
what each row holds.

Conventions: q [B, Sq, Hq*Dh], k / v [B, Skv, Hkv*Dh] fp16, dense (the GPU test moves them into the production layouts); query head h reads
KV head h // (Hq / Hkv); under the causal mask query i sits at key position i + Skv - Sq; kv_len[b] keys of batch b are valid.  A PROBE ROW
is a (batch, query) pair the reference is computed for.  Probe rows get their q from a CPU generator (the same bits on every device);
the other ("filler") query rows are i.i.d. and are never compared.  Logits are kept in the log2 domain throughout: the kernels compute
p = 2^(s - m), and a pre-scaled q (fp16(q32 * scale * log2 e), rounded once from fp32 as its producer does) is what the reference uses.

Families (logits in nats where not said otherwise):
  iid          q, k, v ~ N(0, 1): logits of standard deviation 1 (what the suite had; kept for continuity)
  peaked       q ~ 2.5 N(0, 1): logits of standard deviation 2.5, tens of effective keys per row
  needle       per probe row (per head when Sq = 1) one key at a swept position scores 40 above a body of standard deviation ~2: the output is
               that key's V row.  Needle keys of one batch point along distinct columns of a random orthogonal matrix, so a row sees the other
               rows' needles as ordinary keys.  A late needle exceeds fp16 P around the first tile's reference: k_attn redoes the block exactly.
  needle_soft  the same sweep, but the needle stays INSIDE the fp16 window of the steady-state loop (~2^13 above the first tile's row max, over
               a flat body of standard deviation 0.5): the fast loop itself has to deliver the key; weight 0.3 .. 1 depending on the key count
  anti_needle  a needle-strength key where the row must not see it: at the row's position + 1 (causal) or at kv_len[b] (finite, not NaN)
  sink_in      peaked body; key 0 scores SINK_IN_LOG2 (log2 domain) above the best body key of every probe row and head (set exactly, per row and
               head), so every body P lands in fp16 subnormals (2^-15 and below) around the reference the first tile sets.  The output is V[0] plus
               2^-15 of a body row.  (Measured with V[0] = 0, which leaves the body's share alone: the EMULATION is then at 0.5 .. 1.3 of the bound at
               65 keys already - every key adds half a subnormal step of absolute error whatever its weight - so subnormal P carries such a
               residue to ~2^-8 of itself, not better.  That is a property of fp16 P, not something a bound relative to the row can assert.)
  sink_out     the same with a margin of SINK_OUT_LOG2: every body P flushes to zero, the output is V[0]; must be harmless
  late_peak    peaked body whose first 64 keys are dull (K x 0.1); for each probe row a key 71 positions before its last visible one scores about
               as much as the whole body together AND more than 2^16 above the first tile's maximum: the exact-pass redo has to produce a real
               mixture (weight ~0.5), not a single V row."""
import math
from dataclasses import dataclass, field

import torch

LOG2E = 1.4426950408889634
MAX_REL, COS_MIN = 4e-3, 0.9999          # tests/_tol.py: max_rel, cos_min - applied per probe row and head
NEEDLE_NATS = 40.0
SINK_IN_LOG2, SINK_OUT_LOG2 = 15.0, 40.0
FAMILIES = ("iid", "peaked", "needle", "needle_soft", "anti_needle", "sink_in", "sink_out", "late_peak")
SWEEP = ("last", "last-1", "0", "31", "32", "63", "64", "third", "last_tile_first", "split_first", "split_last", "run_first", "run_last")


@dataclass
class Case:
    name: str
    B: int
    Sq: int
    Skv: int                      # key rows handed to the kernel (a cache's capacity where kv_len is given)
    Hq: int
    Hkv: int
    Dh: int
    causal: bool
    rows: list                    # probe rows (b, i)
    kv_len: list = None           # per batch, or None
    nsplit: int = 1
    split_rule: str = None        # "tiles": k_attn (t_lo = split * per, 64-key tiles); "chunks": k_attn_decode (even shares of 32-key chunks)
    prescaled: bool = True
    variant: int = None           # what ops.attention_variant must say (None: the table names none)
    layout: str = "dense"         # how the GPU test hands the operands over
    families: tuple = FAMILIES
    seed: int = 0
    scale: float = field(init=False)

    def __post_init__(self):
        self.scale = self.Dh ** -0.5
        self.G = self.Hq // self.Hkv

    def nvis(self, b, i, dc=0, dk=0):
        """visible keys of probe row (b, i) are [0, n); dc / dk shift the causal diagonal / kv_len (the mutants' knobs)"""
        n = self.Skv if self.kv_len is None else min(self.Skv, max(0, self.kv_len[b] + dk))
        if self.causal:
            n = min(n, max(0, i + self.Skv - self.Sq + 1 + dc))
        return n

    def late(self, b, i):
        """second half of the sequence (a single query row is the last one)"""
        return self.Sq == 1 or 2 * i >= self.Sq

    # ---- split geometry of the two kernels (attention.hip: per = ceil(nt / nsplit), t_lo = split * per; attention_decode.hip: the first
    # nch % nsplit splits take nch // nsplit + 1 chunks, wave w of a split takes chunks [(ns * w) >> 2, (ns * (w + 1)) >> 2)) ----
    def split_bounds(self, n):
        """key ranges [lo, hi) of every split for a row with n visible keys"""
        if self.nsplit == 1 or self.split_rule is None:
            return [(0, n)]
        if self.split_rule == "tiles":
            nt = (n + 63) // 64
            per = (nt + self.nsplit - 1) // self.nsplit
            return [(min(n, 64 * s * per), min(n, 64 * min(nt, (s + 1) * per))) for s in range(self.nsplit)]
        nch = (n + 31) // 32
        cq, cr = divmod(nch, self.nsplit)
        out = []
        for s in range(self.nsplit):
            lo = s * cq + min(s, cr)
            out.append((min(n, 32 * lo), min(n, 32 * (lo + cq + (1 if s < cr else 0)))))
        return out

    def probe_split(self, n):
        """the split the needle sweep and the "split dropped" mutant aim at: the middle one of those that hold keys"""
        live = [sb for sb in self.split_bounds(n) if sb[1] > sb[0]]
        return live[len(live) // 2]

    def probe_run(self, n):
        """a wave's chunk run inside probe_split (k_attn_decode): the first non-empty one of waves 1, 2, 3, 0"""
        lo, hi = self.probe_split(n)
        ns = (hi - lo + 31) // 32
        for w in (1, 2, 3, 0):
            c0, c1 = (ns * w) >> 2, (ns * (w + 1)) >> 2
            if c1 > c0:
                return lo + 32 * c0, min(hi, lo + 32 * c1)
        return lo, hi

    def resolve(self, sym, n):
        """swept needle position -> key index in [0, n) or None"""
        if n <= 0:
            return None
        if sym == "last":
            p = n - 1
        elif sym == "last-1":
            p = n - 2
        elif sym == "third":
            p = 64 * (((n + 63) // 64) // 3) + 17
            p = p if p < n else n - 1
        elif sym == "last_tile_first":
            p = 64 * ((n - 1) // 64)
        elif sym in ("split_first", "split_last"):
            if self.nsplit == 1 or self.split_rule is None:
                return None
            lo, hi = self.probe_split(n)
            p = lo if sym == "split_first" else hi - 1
        elif sym in ("run_first", "run_last"):
            if self.nsplit == 1 or self.split_rule != "chunks":
                return None
            lo, hi = self.probe_run(n)
            p = lo if sym == "run_first" else hi - 1
        else:
            p = int(sym)
        return p if 0 <= p < n else None


class Inputs:
    """what one (case, family) hands to the kernel and to the references"""

    def __init__(self, case, family, k, v, qp, q, info):
        self.case, self.family, self.k, self.v, self.qp, self.q, self.info = case, family, k, v, qp, q, info
        self.rows = case.rows
        self.late = torch.tensor([case.late(b, i) for b, i in self.rows])
        self._logits = {}

    def logits(self, kvmap=None, bmap=None):
        """[P, Hq, Skv] fp64 logits in the log2 domain of the probe rows against EVERY key (masks come later), from the kernel's own q"""
        key = (kvmap is not None, bmap is not None)
        if key not in self._logits:
            c = self.case
            mul = 1.0 if c.prescaled else c.scale * LOG2E
            out = torch.empty((len(self.rows), c.Hq, c.Skv), dtype=torch.float64, device=self.k.device)
            kk = self.k.view(c.B, c.Skv, c.Hkv, c.Dh)
            for b in sorted({b for b, _ in self.rows}):
                idx = [r for r, (bb, _) in enumerate(self.rows) if bb == b]
                bs = b if bmap is None else bmap(b)
                for g in range(c.Hkv):
                    hs = [h for h in range(c.Hq) if (h // c.G if kvmap is None else kvmap(h)) == g]
                    kd = kk[bs, :, g].double().t()
                    for h in hs:
                        out[idx, h] = (self.qp[idx, h].double() @ kd) * mul
            self._logits[key] = out
        return self._logits[key]


def _orthogonal(Dh, seed):
    g = torch.Generator().manual_seed(seed)
    qm, _ = torch.linalg.qr(torch.randn(Dh, Dh, generator=g, dtype=torch.float64))
    return qm.float()                                                            # columns: unit, mutually orthogonal


class Base:
    """The i.i.d. K / V body of a case, generated once; every family patches a few rows of it and restores them afterwards."""

    def __init__(self, case, device="cpu"):
        self.case, self.device = case, torch.device(device)
        c = case
        g = torch.Generator().manual_seed(1000 + c.seed)
        self.k = torch.empty((c.B, c.Skv, c.Hkv * c.Dh), dtype=torch.float16, device=self.device)
        self.v = torch.empty_like(self.k)
        for b in range(c.B):                                                     # per batch: bounded fp32 temporaries
            self.k[b] = torch.randn(c.Skv, c.Hkv * c.Dh, generator=g).half().to(self.device)
            self.v[b] = torch.randn(c.Skv, c.Hkv * c.Dh, generator=g).half().to(self.device)
        self.U = _orthogonal(c.Dh, 77 + c.seed)
        self._saved = []

    def _patch(self, t, b, p, val, g=None):
        c = self.case
        sl = slice(0, c.Hkv * c.Dh) if g is None else slice(g * c.Dh, (g + 1) * c.Dh)
        self._saved.append((t, b, p, sl, t[b, p, sl].clone()))
        t[b, p, sl] = val.to(device=self.device, dtype=torch.float16) if torch.is_tensor(val) else val

    def restore(self):
        for t, b, p, sl, old in reversed(self._saved):
            t[b, p, sl] = old
        self._saved = []

    def _body_logits_max(self, qp32, exclude0):
        """exact best body logit (log2 domain, fp64) per probe row and head over the visible keys, for q32 rows given in fp32"""
        c = self.case
        kk = self.k.view(c.B, c.Skv, c.Hkv, c.Dh)
        out = torch.empty((len(c.rows), c.Hq), dtype=torch.float64)
        for r, (b, i) in enumerate(c.rows):
            n = c.nvis(b, i)
            lo = 1 if exclude0 else 0
            for g in range(c.Hkv):
                hs = slice(g * c.G, (g + 1) * c.G)
                if n <= lo:
                    out[r, hs] = 0.0
                    continue
                s = qp32[r, hs].double().to(self.device) @ kk[b, lo:n, g].double().t()
                out[r, hs] = (s.max(dim=1).values * (c.scale * LOG2E)).cpu()
        return out

    def make(self, family, full_q=False):
        """-> Inputs.  full_q: also the [B, Sq, Hq*Dh] tensor a kernel call needs (filler rows from the device's generator)."""
        assert not self._saved, "restore() the previous family first"
        c = self.case
        P, sc = len(c.rows), c.scale
        gen = torch.Generator().manual_seed(5000 + 31 * c.seed + FAMILIES.index(family))
        body = {"iid": 1.0, "peaked": 2.5, "sink_in": 2.5, "sink_out": 2.5, "late_peak": 2.5}.get(family, 0.0)
        qp = torch.randn(P, c.Hq, c.Dh, generator=gen) * body                    # fp32, un-scaled ("q32")
        info = {"pos": torch.full((P, c.Hq), -1, dtype=torch.long)}
        U = self.U
        w = U[:, c.Dh - 1]                                                       # the sink's direction; needles use columns 0 .. Dh-2

        def slot_of(slots, b, p):
            s = slots.setdefault(b, {})
            if p not in s:
                s[p] = len(s)
                assert len(s) <= c.Dh - 2, "more needle positions in one batch than orthogonal directions"
            return s[p]

        if family in ("needle", "needle_soft", "anti_needle"):
            if family == "needle_soft":
                aq, ak = 0.5 / sc, ((0.5 * 2.4 + 13.0 / LOG2E) / 0.5)             # body sd 0.5 nats; needle = est. first-tile max + 13 (log2)
            else:
                aq = ak = math.sqrt(NEEDLE_NATS / sc)
            sweep = [s for s in SWEEP if c.resolve(s, max(c.nvis(b, i) for b, i in c.rows)) is not None]
            slots = {}
            for r, (b, i) in enumerate(c.rows):
                n = c.nvis(b, i)
                for h in range(c.Hq):
                    pick = (r * c.Hq + h) if c.Sq == 1 else r
                    if family == "anti_needle":
                        p = None
                        if c.causal and i + c.Skv - c.Sq + 1 < c.Skv and (c.kv_len is None or i + c.Skv - c.Sq + 1 < c.kv_len[b]):
                            p = i + c.Skv - c.Sq + 1                              # valid key, hidden by the causal mask alone
                        elif c.kv_len is not None and c.kv_len[b] < c.Skv and (not c.causal or c.kv_len[b] <= i + c.Skv - c.Sq):
                            p = c.kv_len[b]                                       # hidden by kv_len alone
                    else:
                        p = c.resolve(sweep[pick % len(sweep)], n)
                        p = c.resolve("last", n) if p is None else p
                    if p is None:
                        qp[r, h] = aq * U[:, c.Dh - 2]                            # no such key for this row: a direction no key uses
                        continue
                    u = U[:, slot_of(slots, b, p) % (c.Dh - 2)]
                    qp[r, h] = aq * u
                    info["pos"][r, h] = p
                    self._patch(self.k, b, p, ak * u, h // c.G)
        elif family in ("sink_in", "sink_out"):
            d = 16.0 / sc                                                        # |k_0|; logit_0 = d * scale * (q . w)
            qp -= (qp @ w)[..., None] * w
            for b in range(c.B):
                self._patch(self.k, b, 0, (d * w).repeat(c.Hkv))
            margin = SINK_IN_LOG2 if family == "sink_in" else SINK_OUT_LOG2
            cw = torch.full((P, c.Hq), (2.5 * 4.0 * LOG2E + margin) / (16.0 * LOG2E))
            for _ in range(2):                                                   # the w-component moves the body logits by ~0.1 nat: two rounds settle it
                best = self._body_logits_max(qp + cw[..., None] * w, exclude0=True)
                cw = ((best + margin) / (16.0 * LOG2E)).float()
            qp = qp + cw[..., None] * w
            info["sink_c"] = float(cw.mean())
        elif family == "late_peak":
            slots = {}
            for b in range(c.B):
                for p in range(min(64, c.Skv)):
                    self._patch(self.k, b, p, self.k[b, p].float() * 0.1)
            for r, (b, i) in enumerate(c.rows):
                n = c.nvis(b, i)
                if n < 200:
                    continue
                p = n - 72
                L = max(math.log(n) + 2.5 ** 2 / 2, 0.6 + 12.5)                   # nats: ~ the whole body's weight, and > 2^16 above the dull first tile
                a = math.sqrt(L / sc)
                u = U[:, slot_of(slots, b, p) % (c.Dh - 2)]
                qp[r] = qp[r] - (qp[r] @ u)[..., None] * u + a * u
                info["pos"][r, :] = p
                self._patch(self.k, b, p, (a * u).repeat(c.Hkv))

        def to_kernel(q32):
            return (q32 * (sc * LOG2E)).half() if c.prescaled else q32.half()

        qk = to_kernel(qp).to(self.device)
        q = None
        if full_q:
            gd = torch.Generator(device=self.device).manual_seed(9000 + c.seed)
            q32 = torch.randn((c.B, c.Sq, c.Hq * c.Dh), generator=gd, device=self.device) * (body if body else 1.0)
            if family in ("sink_in", "sink_out"):
                q32 += (info["sink_c"] * w).repeat(c.Hq).to(self.device)
            q = to_kernel(q32)
            del q32
            for r, (b, i) in enumerate(c.rows):
                q[b, i] = qk[r].reshape(-1)
        return Inputs(c, family, self.k, self.v, qk, q, info)


# ---------------------------------------------------------------- references ----------------------------------------------------------------

def _attend(inp, dc=0, dk=0, drop=None, kvmap=None, bmap=None, logit_mul=1.0, no_max_merge=False, mode="exact", flush=2.0 ** -24):
    """softmax(visible logits) @ V for the probe rows -> [P, Hq, Dh] fp64.
    mode "exact": fp64 throughout.  mode "emul": the kernel's roundings - fp32 scores, reference = row max of the first 64 visible keys, P rounded
    to fp16 (below `flush` -> 0; 2^-24 is what fp16 does by itself), the exact softmax where a P overflows, l summed from the rounded P where the
    kernel does (Dh <= 64 or pre-scaled), output rounded to fp16."""
    c = inp.case
    s = inp.logits(kvmap, bmap) * logit_mul
    P, dev = len(inp.rows), s.device
    j = torch.arange(c.Skv, device=dev)
    vis = torch.zeros((P, c.Skv), dtype=torch.bool, device=dev)
    grp = torch.zeros((P, c.Skv), dtype=torch.long, device=dev) if no_max_merge else None
    for r, (b, i) in enumerate(inp.rows):
        n = c.nvis(b, i, dc, dk)
        vis[r] = j < n
        for lo, hi in (drop(c, b, i) if drop else ()):
            vis[r, lo:hi] = False
        if no_max_merge:
            for si, (lo, hi) in enumerate(c.split_bounds(n)):
                grp[r, lo:hi] = si
    s = s.masked_fill(~vis[:, None, :], float("-inf"))
    if mode == "emul":
        s = s.float().double()
        first = s.masked_fill((vis.cumsum(1) > 64)[:, None, :], float("-inf")).max(dim=2, keepdim=True).values
        m = torch.where(torch.isfinite(first), first, torch.zeros_like(first))
        p16 = torch.exp2(s - m).float().half()
        over = torch.isinf(p16).any(dim=2, keepdim=True)
        mx = s.max(dim=2, keepdim=True).values
        m = torch.where(over, torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx)), m)
        p32 = torch.exp2(s - m).float()
        p16 = p32.half()
        p16 = torch.where(p16.float() < flush, torch.zeros_like(p16), p16)
        wgt = p16.double()
        l = wgt.sum(2) if (c.Dh <= 64 or c.prescaled) else p32.double().sum(2)
    elif no_max_merge:
        wgt = torch.zeros_like(s)
        for si in range(c.nsplit):
            sel = (grp == si)[:, None, :] & vis[:, None, :]
            ms = s.masked_fill(~sel, float("-inf")).max(dim=2, keepdim=True).values
            ms = torch.where(torch.isfinite(ms), ms, torch.zeros_like(ms))
            wgt = torch.where(sel, torch.exp2(s - ms), wgt)
        l = wgt.sum(2)
    else:
        mx = s.max(dim=2, keepdim=True).values
        wgt = torch.exp2(s - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx)))
        l = wgt.sum(2)
    out = torch.zeros((P, c.Hq, c.Dh), dtype=torch.float64, device=dev)
    vv = inp.v.view(c.B, c.Skv, c.Hkv, c.Dh)
    for b in sorted({b for b, _ in inp.rows}):
        idx = [r for r, (bb, _) in enumerate(inp.rows) if bb == b]
        bs = b if bmap is None else bmap(b)
        for h in range(c.Hq):
            g = h // c.G if kvmap is None else kvmap(h)
            out[idx, h] = wgt[idx, h] @ vv[bs, :, g].double()
    out = out / l.clamp(min=1e-300)[..., None]                                   # a row without a visible key (mutants only): zeros
    if mode == "emul":
        out = out.float().half().double()
    return out


def reference_fp64(inp):
    return _attend(inp)


def emulation(inp):
    return _attend(inp, mode="emul")


def _third(c, b, i):
    n = c.nvis(b, i)
    return c.resolve("third", n) if n > 0 else 0


def _drop_tile(c, b, i):
    t = _third(c, b, i) // 64
    return [(64 * t, 64 * t + 64)]


def _drop_chunk(c, b, i):
    t = _third(c, b, i) // 32
    return [(32 * t, 32 * t + 32)]


def _drop_last(c, b, i):
    n = c.nvis(b, i)
    return [(n - 1, n)] if n > 0 else []


def _drop_split(c, b, i):
    return [c.probe_split(c.nvis(b, i))]


def _max_live_splits(c):
    return max(sum(1 for lo, hi in c.split_bounds(c.nvis(b, i)) if hi > lo) for b, i in c.rows)


# name -> (wrong reference with reference_fp64's signature, applies(case)).  "applies" is structural: whether the wrong rule can differ from the
# right one on this call at all (a causal row that already sees the last key of the tensor has no key at its position + 1 to leak; a row with one
# visible key has softmax weight 1 whatever the scale and nothing to merge).
MUTANTS = {
    "causal +1": (lambda inp: _attend(inp, dc=+1), lambda c: c.causal and c.Sq > 1),
    "causal -1": (lambda inp: _attend(inp, dc=-1), lambda c: c.causal),
    "kv_len +1": (lambda inp: _attend(inp, dk=+1), lambda c: c.kv_len is not None and not c.causal and min(c.kv_len) < c.Skv),
    "kv_len -1": (lambda inp: _attend(inp, dk=-1), lambda c: c.kv_len is not None and not c.causal),
    "tile dropped": (lambda inp: _attend(inp, drop=_drop_tile), lambda c: True),
    "chunk dropped": (lambda inp: _attend(inp, drop=_drop_chunk), lambda c: True),
    "last key dropped": (lambda inp: _attend(inp, drop=_drop_last), lambda c: True),
    "split dropped": (lambda inp: _attend(inp, drop=_drop_split), lambda c: c.nsplit > 1),
    "merge without max": (lambda inp: _attend(inp, no_max_merge=True), lambda c: c.nsplit > 1 and _max_live_splits(c) > 1),
    "kv head h % Hkv": (lambda inp: _attend(inp, kvmap=lambda h: h % inp.case.Hkv), lambda c: c.Hkv > 1 and c.G > 1),
    "batch 0's K/V": (lambda inp: _attend(inp, bmap=lambda b: 0), lambda c: c.B > 1),
    "scale without log2 e": (lambda inp: _attend(inp, logit_mul=1.0 / LOG2E), lambda c: c.prescaled and max(c.nvis(b, i) for b, i in c.rows) > 1),
    "P flushed below 2^-14": (lambda inp: _attend(inp, mode="emul", flush=2.0 ** -14), lambda c: True),
}

REFERENCE = reference_fp64        # the spot check: point this at any MUTANTS[name][0] and the "emulation passes" half of the power test fails


def check(out, ref):
    """per probe row and head: max|out - ref| / (MAX_REL * max|ref_row|) -> ratio [P, Hq] (passes at <= 1) and the row cosine [P, Hq]"""
    out, ref = out.double(), ref.double()
    scale = ref.abs().amax(dim=-1)
    ratio = (out - ref).abs().amax(dim=-1) / (MAX_REL * scale).clamp(min=1e-300)
    ratio = torch.where(torch.isfinite(out).all(dim=-1), ratio, torch.full_like(ratio, float("inf")))
    cos = torch.nn.functional.cosine_similarity(out, ref, dim=-1)
    cos = torch.where(scale > 0, cos, torch.ones_like(cos))
    return ratio, cos


def failures(ratio, cos, rows_mask=None):
    bad = (ratio > 1.0) | ~(cos >= COS_MIN)
    if rows_mask is not None:
        bad = bad & rows_mask.to(bad.device)[:, None]
    return bad


def describe_worst(inp, ratio, cos):
    r, h = divmod(int(torch.argmax(torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio))), inp.case.Hq)
    b, i = inp.rows[r]
    return (f"{inp.case.name} / {inp.family}: worst ratio to the bound {float(ratio[r, h]):.3g} (cosine {float(cos[r, h]):.6f}) at batch {b} row {i} head {h}, "
            f"needle position {int(inp.info['pos'][r, h])}, {inp.case.nvis(b, i)} visible keys")


def assert_rows_close(inp, out, what=""):
    """out [P, Hq, Dh] against REFERENCE; prints the worst ratio (as tests/_tol.py does) and returns it"""
    ratio, cos = check(out, REFERENCE(inp))
    msg = describe_worst(inp, ratio, cos)
    print(f"\n[attn] {what}{msg}")
    assert not bool(failures(ratio, cos).any()), msg
    return float(ratio.max())


# ---------------------------------------------------------------- the case table ----------------------------------------------------------------

def _prod_nsplit_trimmed(S):
    """the split factor of the retired single-row trim of Qwen2Model.forward's last layer, which ran the final row alone through the causal
    split-KV attention (~2 tiles of 64 keys per split, up to 128 splits).  No production call takes it any more; it is kept to size the
    coverage of that kernel path (tests/test_host_logic.py pins the values)."""
    return max(1, min(128, ((S + 63) // 64) // 2))


def _prod_nsplit_batched(lens, Hq, Hkv, Dh):
    """the split factor BatchDecoder.prepare_steps takes for a step over sequences that hold `lens` keys after it"""
    import types
    from streamchat_amd import llm as LM
    d = object.__new__(LM.BatchDecoder)
    d.B, d.len = len(lens), torch.tensor(lens, dtype=torch.int32) - 1
    d.lm = types.SimpleNamespace(device=torch.device("cpu"), cfg=types.SimpleNamespace(kv_heads=Hkv, heads=Hq, head_dim=Dh))
    d.prepare_steps(1)
    return int(d.nsplit)


PREFILL_ROWS = [0, 1, 63, 64, 191, 192, 193, 4095, 4096, 20000, 24575, 24576, 30001, 40000, 48959, 48960, 48961, 49000, 49087, 49088, 49150, 49151,
                777, 12345, 36863, 36864, 45000]         # test_attention_full_size_llm_prefill_rows_vs_torch's 24 + three late ones for the sweep
DECODE_S = [1, 33, 767, 768, 769, 2272, 2273, 49120, 49121, 49157, 49920]      # + both sides of decode_nsplit's clamps (2 | 3 splits, 63 | 64, 64 | "65")
BATCHED_LENS = [22100 + 47 * b for b in range(26)]
BATCHED_LENS[5] = 33                                     # one short sequence; the longest (b = 25) fills the cache to capacity


def cases():
    from streamchat_amd import llm as LM
    out = []
    H = dict(Hq=28, Hkv=4, Dh=128)
    out.append(Case("prefill 49152", 1, 49152, 49152, causal=True, rows=[(0, i) for i in PREFILL_ROWS], variant=1, seed=1, **H))
    ch = [0, 1, 47, 48, 191, 192, 2047, 2048, 2100, 2500, 3000, 3071, 3072, 3500, 3903, 3904, 4000, 4094, 4095]
    for pos0 in (1, 63, 20001):
        out.append(Case(f"chunked prefill 4096 behind {pos0}", 1, 4096, pos0 + 4096, causal=True, rows=[(0, i) for i in ch], variant=1, seed=2, **H))
    sh = [0, 1, 63, 64, 149, 150, 191, 192, 200, 230, 255, 256, 270, 280, 290, 298, 299]
    out.append(Case("chunked prefill 300 behind 20001", 1, 300, 20301, causal=True, rows=[(0, i) for i in sh], variant=0, seed=3, **H))
    for S in (65, 127, 128, 129, 8191, 49157):
        out.append(Case(f"trimmed last layer {S}", 1, 1, S, causal=True, rows=[(0, 0)], nsplit=_prod_nsplit_trimmed(S), split_rule="tiles",
                        layout="cache", seed=4, **H))
    for S in DECODE_S:
        out.append(Case(f"decode step {S}", 1, 1, S + 64, causal=False, rows=[(0, 0)], kv_len=[S], nsplit=LM.decode_nsplit(128, S), split_rule="chunks",
                        variant=3, layout="packed", seed=5, **H))
    out.append(Case("batched caption decode", 26, 1, max(BATCHED_LENS), causal=False, rows=[(b, 0) for b in range(26)], kv_len=list(BATCHED_LENS),
                    nsplit=_prod_nsplit_batched(BATCHED_LENS, 28, 4, 128), split_rule="chunks", variant=3, layout="packed_batched", seed=6, **H))
    vr = [0, 1, 100, 288, 300, 350, 400, 450, 511, 512, 575, 576]
    out.append(Case("ViT 4 x 577", 4, 577, 577, 16, 16, 64, causal=False, rows=[(b, i) for b in range(4) for i in vr], layout="fused_qkv", seed=7))
    br = [0, 1, 76, 77, 255, 256, 299, 300, 400, 511]
    for Hh, Dh in ((12, 32), (16, 64)):
        out.append(Case(f"BERT {Hh} x {Dh}", 4, 512, 512, Hh, Hh, Dh, causal=False, rows=[(b, i) for b in range(4) for i in br], kv_len=[512, 1, 300, 77],
                        prescaled=False, layout="fused_qkv", seed=8))
    for c in out:
        fam = [f for f in FAMILIES]
        if not (c.causal and c.Sq > 1) and not (c.kv_len is not None and min(c.kv_len) < c.Skv):
            fam.remove("anti_needle")                                            # no key the row must not see
        if not (c.causal and c.Sq > 1 and c.Dh == 128):
            fam.remove("late_peak")                                              # the steady-state loop of the prefill kernels
        c.families = tuple(fam)
        assert all(c.nvis(b, i) > 0 for b, i in c.rows), c.name                  # share of probe rows without a visible key: 0
    return out
