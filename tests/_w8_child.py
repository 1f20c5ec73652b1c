"""Child process of tests/test_gpu_w8.py: a set of w8 launches whose output bytes go to stdout as one sha256 (the parent compares two runs
with different SC_GEMV_WPB_* values), or - with `entry` - the entry point end to end under SC_DECODE_WEIGHTS."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def wpb():
    from streamchat_amd import ops
    from tests import _w8
    h = hashlib.sha256()
    for kw in (dict(N=37, K=1040, bias=True, res=True), dict(N=50, K=3584, norm=True, bias=True), dict(N=50, K=18944, res=True),
               dict(N=16500, K=48), dict(N=36, K=1040, swiglu=True, norm=True)):
        c = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in _w8.gemv_case(**kw).items()}
        for f32 in ((False,) if kw.get("swiglu") else (False, True)):
            y = ops.gemv_w8(c["q"], c["scale"], c["x"], c["bias"], c["res"], epilogue="swiglu" if kw.get("swiglu") else "none", out_f32=f32,
                            rms_gamma=c["gamma"], rms_eps=1e-6)
            h.update(y.cpu().numpy().tobytes())
    for Hq, Hkv, Dh, K in ((4, 2, 64, 256), (28, 4, 128, 3584)):
        dq, dkv = Hq * Dh, Hkv * Dh
        c = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in _w8.gemv_case(dq + 2 * dkv, K, seed=7, norm=True, bias=True).items()}
        tq, tk = ops.rope_table(64, Dh, 1e6, Dh ** -0.5 * ops.LOG2E, "cuda:0"), ops.rope_table(64, Dh, 1e6, 1.0, "cuda:0")
        q_out, cache = torch.zeros(dq, dtype=torch.float16, device="cuda"), torch.zeros((8, 2 * dkv), dtype=torch.float16, device="cuda")
        ops.decode_qkv_tab_w8(c["q"][:dq], c["scale"][:dq], c["q"][dq:], c["scale"][dq:], c["bias"][:dq].contiguous(), c["bias"][dq:].contiguous(), c["x"],
                              c["gamma"], 1e-6, q_out, cache, torch.tensor([3], dtype=torch.int32, device="cuda"), Hq, Hkv, Dh, tq, tk)
        h.update(q_out.cpu().numpy().tobytes()); h.update(cache.cpu().numpy().tobytes())
    print("W8SHA", h.hexdigest())


def entry(out_dir):
    import inference_streaming_longva_v2 as E
    from streamchat_amd import llm as LM
    assert LM.DEFAULT_DECODE_WEIGHTS == "fp8"
    args = E.parse_args(["--video_dir", "none", "--model_name", "none", "--memory_basic_dir", os.path.join(out_dir, "mem"), "--save_file",
                         os.path.join(out_dir, "out.json"), "--annotations", "none", "--language", "en", "--conv-mode", "qwen_1_5", "--synthetic", "1",
                         "--tiny", "--chunk_size", "4", "--num_clusters", "2", "--interval", "3", "--short_window", "6", "--remember_window", "3",
                         "--max_new_tokens", "4", "--multi_modal_memory"])
    seen = []
    orig = LM.ops.gemv_w8
    LM.ops.gemv_w8 = lambda *a, **k: (seen.append(1), orig(*a, **k))[1]
    E.run_inference(args)
    print("W8CALLS", len(seen))


if __name__ == "__main__":
    wpb() if sys.argv[1] == "wpb" else entry(sys.argv[2])
