"""Guarded output buffers for the write-bound tests (tests/test_gpu_write_bounds.py; self-test on the CPU: tests/test_guard_helper.py).

Every parity test compares the dense output region with its reference; none of them can see a store that lands next to it.  `Arena`
hands out output tensors that are VIEWS into a larger allocation whose every byte was first set to one pattern, and `Arena.check`
verifies afterwards that each byte outside the views still holds it:

    lead band | row 0: cols, gap | row 1: cols, gap | ... | row R-1: cols, gap | tail band (tail_rows x ld)

The pattern byte 0x7E reads as a NaN in fp16 (0x7E7E), as 8.4e37 in fp32 and bf16 (no repeated byte but 0xFF, the plausible integer -1, is a
NaN in fp32) and as an implausible integer (2122219134), so a kernel that READS a guard byte shows up in its results as well.  The tail band is sized by the caller from the largest tile of the
kernel that can take the call, so that a plausible overrun lands in the arena - and is reported - instead of in foreign memory.
`frozen(...)` asserts that a call left its inputs alone."""
import contextlib

import torch

PATTERN = 0x7E
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class GuardViolation(AssertionError):
    """a guard byte changed: `first` / `last` are (row, column) of the first / last changed byte relative to the view (row < 0: the lead
    band, row >= rows: the tail band, column >= cols: the leading-dimension gap), `count` the number of changed bytes"""

    def __init__(self, msg, name, first, last, count):
        super().__init__(msg)
        self.name, self.first, self.last, self.count = name, first, last, count


class _Block:
    def __init__(self, raw, start, rows, cols, ld, es, name):
        self.raw, self.start, self.rows, self.cols, self.ld, self.es, self.name = raw, start, rows, cols, ld, es, name

    def guard_regions(self):
        """(byte offset of the region's first element in raw, 2-D uint8 view [n, w], raw row stride) of the three guard areas"""
        row_b, end = self.ld * self.es, self.start + self.rows * self.ld * self.es
        body = self.raw[self.start:end].view(self.rows, row_b)
        return [(0, self.raw[:self.start].view(1, -1), 0), (self.start + self.cols * self.es, body[:, self.cols * self.es:], row_b),
                (end, self.raw[end:].view(1, -1), 0)]

    def locate(self, off):
        """raw byte offset -> (row, column) in elements relative to the view's first element"""
        rel = off - self.start
        return rel // (self.ld * self.es), (rel % (self.ld * self.es)) // self.es


class Arena:
    def __init__(self, device):
        self.device = torch.device(device)
        self.blocks = []

    def out(self, rows, cols, dtype, ld=None, lead_bytes=4096, tail_rows=256, align=256, misalign=0, name=None):
        """[rows, cols] view of `dtype` with row stride ld >= cols (elements).  Guards: at least `lead_bytes` in front, the ld - cols gap of
        every row INCLUDING the last one, and `tail_rows` further rows of ld elements behind.  The first element's address is
        `misalign` bytes past a multiple of `align` (defaults: 256-byte aligned; align=16, misalign=8 gives a start that is 8-byte but not
        16-byte aligned)."""
        ld = cols if ld is None else ld
        es = torch.empty(0, dtype=dtype).element_size()
        assert rows > 0 and cols > 0 and ld >= cols and tail_rows >= 1 and lead_bytes >= 0 and misalign % es == 0 and align % es == 0
        body = rows * ld * es
        raw = torch.full((lead_bytes + 2 * align + body + tail_rows * ld * es,), PATTERN, dtype=torch.uint8, device=self.device)
        start = lead_bytes + (misalign - (raw.data_ptr() + lead_bytes)) % align
        if start == 0:                      # lead_bytes = 0 with a lucky base address: still keep one guard unit in front
            start += align
        blk = _Block(raw, start, rows, cols, ld, es, name or f"out{len(self.blocks)}")
        self.blocks.append(blk)
        t = torch.as_strided(raw[start:start + body].view(dtype), (rows, cols), (ld, 1))
        assert (t.data_ptr() - misalign) % align == 0
        return t

    def flat(self, n, dtype, tail_bytes=1 << 16, **kw):
        """1-D view of exactly n elements (a workspace of exactly the reported size, a vector output), tail band of >= tail_bytes"""
        es = torch.empty(0, dtype=dtype).element_size()
        return self.out(1, n, dtype, tail_rows=max(1, -(-tail_bytes // (n * es))), **kw)[0]

    def check(self, what=""):
        """every guard byte still holds the pattern (compared as integers), else GuardViolation naming where and how much"""
        for b in self.blocks:
            bad, first, last = 0, None, None
            for base, reg, stride in b.guard_regions():
                ne = reg != PATTERN
                n = int(ne.sum())
                if n == 0:
                    continue
                bad += n
                idx = ne.nonzero()
                offs = [base + int(i[0]) * stride + int(i[1]) for i in (idx[0], idx[-1])]
                first = offs[0] if first is None else first
                last = offs[1]
            if bad:
                (r0, c0), (r1, c1) = b.locate(first), b.locate(last)
                raise GuardViolation(
                    f"{what}: {bad} guard byte(s) of '{b.name}' ([{b.rows}, {b.cols}] view, ld {b.ld}, {b.es}-byte elements) changed: first at "
                    f"(row {r0}, col {c0}), last at (row {r1}, col {c1}) relative to the view", b.name, (r0, c0), (r1, c1), bad)


def _bits(t):
    return t.view(_INT[t.element_size()])


@contextlib.contextmanager
def frozen(*tensors):
    """the call inside the block did not modify these tensors (None entries are skipped): integer views, compared with torch.equal"""
    ts = [t for t in tensors if t is not None]
    snap = [_bits(t).clone() for t in ts]
    yield
    for i, (t, s) in enumerate(zip(ts, snap)):
        assert torch.equal(_bits(t), s), f"input {i} (shape {tuple(t.shape)}, {t.dtype}) was modified by the call"
