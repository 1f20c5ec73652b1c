"""CPU: the cases tests/test_gpu_attention_power.py runs on the GPU can tell a wrong attention from a right one.
For every case of tests/_attn_cases.cases() (sizes unchanged; only probe rows are computed):
  * an emulation of the kernel's roundings passes the per-row check against the fp64 reference, for every family;
  * every wrong reference ("mutant") that applies to the case FAILS the check for at least one family ON A PROBE ROW IN THE SECOND HALF OF THE
    SEQUENCE (early rows see few keys and catch everything).  A mutant whose effect stays below the bound for every input is listed in
    BELOW_THE_BOUND with the reason; its best ratio is still measured and recorded.
`python -m tests.test_attention_case_power` prints the table case x mutant -> worst late-row ratio to the bound (maximised over families) beside the
emulation's ratio, and rewrites tests/ATTENTION_POWER.md with it."""
import os
import time

import pytest
import torch

from tests import _attn_cases as A

# "P flushed below 2^-14" (a kernel without fp16 subnormals) changes a row by at most the weight of the keys 2^14 below the row's reference, i.e.
# by < 2^-14 x (keys) of the row: below 4e-3 of the row for every input whose reference key carries a non-zero V.  It stays in the table with
# its best ratio.  (A row made ONLY of such keys - sink with V[0] = 0 - would catch it, but there the correct roundings miss the bound too:
# see sink_in in tests/_attn_cases.py.)
BELOW_THE_BOUND = {"P flushed below 2^-14": "at most 2^-14 x keys of a row"}

_CASES = A.cases()
_TABLE = {}


def _measure(case):
    """-> (emulation: {family: worst ratio over all probe rows}, mutants: {name: (best late-row ratio over families, family)}, failures)"""
    base = A.Base(case, "cpu")
    emu, mut, problems = {}, {}, []
    names = [n for n, (_, applies) in A.MUTANTS.items() if applies(case)]
    for fam in case.families:
        inp = base.make(fam)
        ref = A.REFERENCE(inp)
        ratio, cos = A.check(A.emulation(inp), ref)
        emu[fam] = float(ratio.max())
        if bool(A.failures(ratio, cos).any()):
            problems.append("emulation fails: " + A.describe_worst(inp, ratio, cos))
        for n in names:
            if n in mut and mut[n][0] > 1e3:
                continue                                                         # caught by a wide margin already: no need for another family's figure
            r2, c2 = A.check(A.MUTANTS[n][0](inp), ref)
            bad = bool(A.failures(r2, c2, inp.late).any())
            worst = float(torch.nan_to_num(r2[inp.late], nan=float("inf")).max())
            old = mut.get(n, (0.0, fam, False))
            mut[n] = (max(old[0], worst), fam if worst > old[0] else old[1], old[2] or bad)
        base.restore()
    for n in names:
        if not mut[n][2] and n not in BELOW_THE_BOUND:
            problems.append(f"mutant '{n}' passes on every late probe row of every family (best ratio {mut[n][0]:.3g}, {mut[n][1]})")
    return emu, mut, problems


@pytest.mark.parametrize("case", _CASES, ids=[c.name.replace(" ", "_") for c in _CASES])
def test_cases_have_power(case):
    t0 = time.time()
    emu, mut, problems = _measure(case)
    _TABLE[case.name] = (emu, mut)
    print(f"\n[power] {case.name} ({time.time() - t0:.1f} s): emulation " + ", ".join(f"{f} {r:.2g}" for f, r in emu.items()))
    print("[power]   mutants (late rows): " + ", ".join(f"{n} {r:.3g} ({f})" for n, (r, f, _) in mut.items()))
    assert not problems, "\n".join(problems)


def test_every_mutant_applies_somewhere_and_batch_mutant_to_the_batched_case():
    for n, (_, applies) in A.MUTANTS.items():
        assert any(applies(c) for c in _CASES), n
    batched = [c for c in _CASES if c.name == "batched caption decode"][0]
    assert A.MUTANTS["batch 0's K/V"][1](batched) and batched.B == 26 and 33 in batched.kv_len and max(batched.kv_len) == batched.Skv


def _markdown():
    names = list(A.MUTANTS)
    lines = ["# What the attention cases can tell apart", "",
             "Written by `python -m tests.test_attention_case_power`; do not edit.  Every figure is `max|out - ref| / (4e-3 * max|ref_row|)` over probe",
             "rows and heads (a value above 1 fails the check).  *emulation*: the kernel's roundings on the CPU, worst family, all probe rows - it has to",
             "stay below 1.  Mutant columns: a wrong reference, probe rows in the SECOND HALF of the sequence only, best family (in brackets after the",
             "figure) - it has to exceed 1.  `-`: the mutant cannot differ from the reference on this call.  The distance between the emulation and",
             "the weakest caught mutant of a row is the measured margin of the suite for that call.", "",
             "| case | emulation | " + " | ".join(names) + " |", "|---|---|" + "---|" * len(names)]
    for c in _CASES:
        emu, mut = _TABLE[c.name]
        wf = max(emu, key=emu.get)
        cells = [(f"{mut[n][0]:.3g} ({mut[n][1]})" + ("" if mut[n][2] else " below the bound")) if n in mut else "-" for n in names]
        lines.append(f"| {c.name} | {emu[wf]:.2g} ({wf}) | " + " | ".join(cells) + " |")
    lines += ["", "Emulation per family:", "", "| case | " + " | ".join(A.FAMILIES) + " |", "|---|" + "---|" * len(A.FAMILIES)]
    for c in _CASES:
        emu = _TABLE[c.name][0]
        lines.append(f"| {c.name} | " + " | ".join(f"{emu[f]:.2g}" if f in emu else "-" for f in A.FAMILIES) + " |")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    t0 = time.time()
    bad = []
    for c in _CASES:
        emu, mut, problems = _measure(c)
        _TABLE[c.name] = (emu, mut)
        bad += problems
        print(c.name, f"{time.time() - t0:.0f} s", flush=True)
    text = _markdown()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "ATTENTION_POWER.md"), "w") as f:
        f.write(text)
    print(text)
    print("\n".join(bad) if bad else "every mutant caught on a late row, every emulation below the bound")
