#!/usr/bin/env python3
"""The fp16 output BITS of the decode attention (k_attn_decode + k_attn_combine on the dequantised cache) at the cases of
tests/_kv8.DECODE_BITS_CASES -> tests/golden/decode_attention_bits.npz.  Runs on the GPU.

k_attn_decode and k_attn_kv8 share their chunk partition, softmax step, P.V accumulation and wave merge (csrc/attention_decode_common.h), so
their bit-for-bit comparison cannot see a mistake in that shared text: both sides move together.  This file pins what the kernels computed
BEFORE they shared it.  Record it with a library built from a commit whose decode attention is known good, never to make a failing test pass:

    SC_LIB=/path/to/libstreamchat_hip.so python tools/make_golden_decode_bits.py --source <commit hash> [--out FILE]

Per case: `bits_<S>_<G>_<nsplit>` uint16 [G, 2 * 128] and `crc_<S>_<G>_<nsplit>`, the CRC32 of the generated inputs (codes, scales, q: torch's CPU
generator), so that a drifted generator is told apart from a changed kernel.  The recording library's sc_attention_kv8 must give the same bits."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from streamchat_amd import llm as LM, ops  # noqa: E402
from tests import _kv8  # noqa: E402
from tests.test_gpu_kv8 import _attend_both  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--source", required=True, help="the commit the loaded library was built from (stored in the file)")
    p.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "decode_attention_bits.npz"))
    a = p.parse_args()
    out = dict(source=np.array(a.source), build=np.array(ops.build_info()))
    for S, G, nsplit in _kv8.DECODE_BITS_CASES:
        nsplit = nsplit or LM.decode_nsplit(128, S)
        codes, scale, q, crc = _kv8.decode_bits_inputs(S, G)
        kv8, f16 = _attend_both(codes, scale, q, 2, nsplit, pad=0)
        assert ops.attention_variant(128, G, nsplit) == 3, "not the decode kernel"
        assert _kv8.same_bits(kv8, f16), f"S={S} G={G} nsplit={nsplit}: the recording library's two kernels disagree"
        ref = _kv8.attention_fp64(q, codes, scale, 2)
        err = ((f16.cpu().double() - ref).abs().max() / ref.abs().max()).item()
        assert bool(torch.isfinite(f16).all()) and err < 2e-2, f"S={S} G={G} nsplit={nsplit}: not an attention (rel. error {err:.3g})"
        key = f"{S}_{G}_{nsplit}"
        out["bits_" + key] = f16.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
        out["crc_" + key] = np.uint32(crc)
        print(f"S={S} G={G} nsplit={nsplit}: crc {crc:#010x}, rel. error to fp64 {err:.2e}")
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
