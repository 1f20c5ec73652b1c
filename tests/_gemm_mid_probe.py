"""Helper of test_gpu_gemm_mid.py: sc_gemm_f16 on seeded random fp16 operands at the shapes k_gemm_mid takes over -> an .npz of raw output
bits.  Run in a subprocess once with SC_GEMM_MID=0 (the dispatch without the kernel: k_gemm128) and once without: the two files must be
bit-identical."""
import sys
import numpy as np
import torch
from streamchat_amd import ops

MS, NS, K0 = (33, 63, 64, 65, 129, 577, 1023), (128, 384), 1024
# BERT-large layer shapes at M = 160, each with its real epilogue: (N, K, epilogue, residual)
BERT_LARGE = ((3072, 1024, "none", False), (1024, 1024, "none", True), (4096, 1024, "gelu", False), (1024, 4096, "none", True))
EPIS = ("none", "quick_gelu", "gelu")


def cases():
    out = []
    for i, M in enumerate(MS):
        for j, N in enumerate(NS):
            out.append((M, N, K0, EPIS[(i + j) % 3], (i + j) % 2 == 0, (i + 2 * j) % 3 != 0))           # (.., epilogue, bias?, residual?)
    out += [(160, N, K, epi, True, res) for N, K, epi, res in BERT_LARGE]
    return out


def main(path):
    g = torch.Generator(device="cuda").manual_seed(9)
    rn = lambda *s, std=1.0: (torch.randn(*s, device="cuda", generator=g) * std).half()
    out = {}
    for M, N, K, epi, has_b, has_r in cases():
        a, w = rn(M, K), rn(N, K, std=0.03)
        y = ops.gemm(a, w, rn(N, std=0.1) if has_b else None, residual=rn(M, N) if has_r else None, epilogue=epi)
        out[f"gemm_{M}x{N}x{K}_{epi}_b{int(has_b)}_r{int(has_r)}"] = y.cpu().numpy().view(np.uint16)
    torch.cuda.synchronize()
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1])
