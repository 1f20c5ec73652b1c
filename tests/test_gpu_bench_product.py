"""GPU: the `product` leg of `bench.py --full` (round 4): the C3 step with the HIP LLM itself as chunk captioner
+ merge summariser (reference utiles.py:539-559,591-607) through llm.BatchDecoder.  A 2-layer model at the Qwen2-7B widths keeps it short; what
is checked is the plumbing the driver line depends on: every chunk of the update goes through ONE batched generate, the record is complete and
self-consistent, the step's retrieval still works on the generated captions, and the headline path is untouched afterwards."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def test_product_step_with_the_llm_as_chunk_captioner():
    import bench
    from streamchat_amd import llm as LM
    dev = torch.device("cuda:0")
    pipe = bench.Pipeline(dev, 440, with_llm=False)                 # 11 chunks of 40 frames: ten of them merge (one k-means T = 400)
    qc = LM.Qwen2ConfigLite(**dict(LM.QWEN2_7B, layers=2))
    pipe.model = LM.LlavaQwenForCausalLM(LM.Qwen2Model(LM.random_qwen2_state_dict(qc, seed=4, device=dev), qc, device=dev, max_seq=53248), pipe.enc)
    plain = pipe.step()                                             # the headline step (synthetic captions)
    ctx_plain, tok_plain = pipe.last["context"], int(pipe.last["first_token"][0, 0])
    rec = bench.measure_product(pipe, 1, 440)
    pipe.captioner = None
    assert rec["chunks_per_step"] == 11 and rec["steps"] == 1
    assert 40 * 576 < rec["prompt_tokens_per_chunk"] < 40 * 576 + 200          # 23 040 image tokens + the caption prompt
    assert rec["product_frames_per_s"] > 0 and rec["caption_prefill_s_per_step"] > 0 and rec["caption_decode_s_per_step"] > 0
    # (the roofline figures use the 28-layer 7B flop / byte model of SURVEY 8(d): with this 2-layer stand-in only their presence is checked)
    assert rec["caption_prefill"]["bound"] == "mfma" and rec["caption_prefill"]["frac"] > 0
    assert rec["caption_decode"]["bound"] == "hbm" and rec["caption_decode"]["frac"] > 0
    assert rec["caption_decode"]["tokens_per_s_aggregate"] > 0 and rec["ms_per_step"] >= 1e3 * (rec["caption_prefill_s_per_step"] + rec["caption_decode_s_per_step"])
    # the step ran the whole path on the generated captions: a tree with one merged node + one depth-0 node, a retrieved context, a first token
    assert [n.depth for n in pipe.last["tree"]] == [1, 0] and pipe.last["context"] > 5 * 576 + 2 * 40 * 576
    # and the headline step is what it was (the captioner is gone again)
    again = pipe.step()
    assert pipe.last["context"] == ctx_plain and int(pipe.last["first_token"][0, 0]) == tok_plain
    assert [n.text for n in again["tree"]] == [n.text for n in plain["tree"]]


def test_bench_dump_outputs_writes_what_the_last_timed_step_computed(tmp_path):
    """`bench.py --steps 2 --dump-outputs DIR` (C2 on a 440-frame stream): the record counts the 2 timed steps and their ms_per_step, and DIR holds
    float .npy files of at most 64 MB in all - the encoded-feature sample equals the same seeded sample of a fresh step's features in this
    process (same inputs, same kernels), the retrieved path's crc32s those of that step."""
    import json
    import subprocess
    import zlib
    import numpy as np
    import bench
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C2", "--frames", "440", "--steps", "2", "--warmup", "0",
                        "--no-cpu-baseline", "--dump-outputs", d], cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0 and rec["dumped_outputs"]["dir"] == d
    names = sorted(f[:-4] for f in os.listdir(d))
    assert names == sorted(rec["dumped_outputs"]["shapes"]) == ["answer_image_embeddings", "encode_features", "path_text_crc32"]
    got = {k: np.load(os.path.join(d, k + ".npy")) for k in names}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values()) and sum(v.nbytes for v in got.values()) <= 64 << 20
    assert got["encode_features"].shape == (bench.DUMP_SAMPLE,) and np.isfinite(got["encode_features"]).all()
    pipe = bench.Pipeline(torch.device("cuda:0"), 440, with_llm=False)
    pipe.step()
    mine = bench.collect_outputs(pipe, "C2", False)
    np.testing.assert_allclose(got["encode_features"], mine["encode_features"], rtol=1e-3, atol=1e-3)
    assert got["path_text_crc32"].tolist() == [zlib.crc32(t.encode()) for t in pipe.last["path_text"]] == mine["path_text_crc32"].tolist()
    np.testing.assert_allclose(got["answer_image_embeddings"], mine["answer_image_embeddings"], rtol=1e-3, atol=1e-3)


def test_plain_bench_runs_no_side_measurement_and_full_adds_them():
    """A plain `bench.py` run prints what its timed steps measured and nothing else; `--full` adds the side measurements that take runs of their
    own.  C2 on a 440-frame stream (one merge k-means T = 400): plain, no CPU baseline and no forced 10-pass k-means; with `--full` (CPU baseline
    left out to keep it short) the k-means is forced through its 10 Lloyd passes, and the headline fields say the same things."""
    import json
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", "C2", "--frames", "440", "--steps", "1", "--warmup", "0"]
    recs = []
    for extra in ([], ["--full", "--no-cpu-baseline"]):
        r = subprocess.run(cmd + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert r.returncode == 0 and len(lines) == 1, r.stdout[-2000:] + r.stderr[-4000:]
        recs.append(json.loads(lines[0]))
    plain, full = recs
    assert "cpu_baseline" not in plain and "kmeans_10_passes" not in plain["roofline_stages"] and plain["roofline_stages"]["kmeans"]["launches"] >= 1
    assert full["roofline_stages"]["kmeans_10_passes"]["lloyd_passes"] == 10 and "cpu_baseline" not in full
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["config"]["retrieval_crc32"] == full["config"]["retrieval_crc32"]
