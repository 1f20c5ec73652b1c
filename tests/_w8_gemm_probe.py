"""Child process of tests/test_gpu_w8_gemm.py: the e4m3-weight GEMM launches of tests/_w8_gemm.SHAPES, every output into one .npz.  The parent
runs it twice - default dispatch, and SC_SKINNY_W8_GENERIC=1 (read once per process, hence the child) - and compares the files bit for bit."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(path):
    from streamchat_amd import ops
    from tests import _w8_gemm as G
    out = {}
    for (N, K), stream in (((N, K), s) for N, K in G.SHAPES for s in G.streams_for(N, K)):
        for name, kw in (("plain", {}), ("bias_res", dict(bias=True, res=True)), ("swiglu", dict(swiglu=True))):
            c = G.contract_case(N, K, seed=5, **kw)
            d = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}
            for M in (1, 16, 26):
                for f32 in ((False,) if c["swiglu"] else (False, True)):
                    with G.on_stream(stream):
                        y = ops.gemm_w8(d["a"][:M], d["q"], d["scale"], d["bias"], None if d["res"] is None else d["res"][:M],
                                        epilogue="swiglu" if c["swiglu"] else "none", out_f32=f32)
                    out[f"{N}x{K}_{name}_M{M}_{'f32' if f32 else 'f16'}{'' if stream is None else '_masked'}"] = y.cpu().numpy()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
