"""CPU: what a session checkpoint holds besides the tree (streamchat_amd/persistence.py) - host random state that continues in ANOTHER
process where it was captured, a save that refuses rows it does not understand, a save that can be cut short without losing the previous
checkpoint, the settings fingerprint, and files written before checkpoints could resume."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from streamchat_amd import persistence as P, utiles as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = dict(chunk_size=4, num_clusters=2, interval=3, short_window=6, remember_window=3, tau=5, compress_rate=1, sample_rate=0.5)
N = 7


def _tree(scale=1.0):
    bank = torch.arange(6 * 2 * 4, dtype=torch.float16).reshape(6, 2, 4) * scale
    leaves = [U.MultimodalTreeNode(bank[i * 2:(i + 1) * 2], f"chunk {i}", depth=0) for i in range(3)]
    root = U.MultimodalTreeNode(torch.ones(2, 2, 4, dtype=torch.float16) * scale, "summary é", depth=1)
    root.children = leaves[:2]
    return [root, leaves[2]], [bank[5:6]]


def _draw(answers, captions, n=N):
    """n values from each of the five sources a round reads, the way the product draws them"""
    return dict(torch=[torch.randperm(50)[:3].tolist() for _ in range(n)], python=[random.randint(0, 10 ** 9) for _ in range(n)],
                numpy=[np.random.choice(np.arange(20), size=3, replace=False, p=U.calculate_forgetting_probabilities(20, tau=5)).tolist() for _ in range(n)],
                answers=torch.randint(0, 2 ** 62, (n,), generator=answers).tolist(), captions=torch.randint(0, 2 ** 62, (n,), generator=captions).tolist())


def _save(tmp_path, name="video_0", state=None, scale=1.0, **over):
    nodes, short = _tree(scale)
    state = state if state is not None else P.capture_host_state({"answers": torch.Generator().manual_seed(1), "captions": torch.Generator().manual_seed(2)})
    kw = dict(next_segment=2, segments=3, frames_consumed=[0, 240], answers=2, turns=2, host_state=state,
              fingerprint=P.settings_fingerprint(SETTINGS, (2, 4), torch.float16), extra=dict(time=120, question="q"))
    kw.update(over)
    P.save_checkpoint(str(tmp_path), 0, nodes, short, **kw)
    return nodes, short


CHILD = """
import json, random, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[3])
from streamchat_amd import persistence as P
from tests.test_resume_state import _draw
nodes, short, extra, info = P.load_checkpoint(sys.argv[1], device="cpu")
a, c = torch.Generator().manual_seed(99), torch.Generator().manual_seed(98)          # other seeds than the parent's: the state must come from the file
P.restore_host_state(info["host_state"], {"answers": a, "captions": c})
json.dump(_draw(a, c), open(sys.argv[2], "w"))
"""


def test_host_state_continues_in_a_fresh_process(tmp_path):
    torch.manual_seed(3); random.seed(4); np.random.seed(5)
    a, c = torch.Generator().manual_seed(6), torch.Generator().manual_seed(7)
    _draw(a, c, 3)                                                          # not at the seeds any more
    random.gauss(0, 1)                                                      # (leaves Python's cached second gaussian set)
    _save(tmp_path, state=P.capture_host_state({"answers": a, "captions": c}))
    want = _draw(a, c)
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "video_0"), str(tmp_path / "got.json"), ROOT], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert json.load(open(tmp_path / "got.json")) == want
    # ... and in this process, after the generators have moved on
    _, _, _, info = P.load_checkpoint(str(tmp_path / "video_0"), device="cpu")
    P.restore_host_state(info["host_state"], {"answers": a, "captions": c})
    assert _draw(a, c) == want
    with pytest.raises(P.ResumeError, match="captions"):                    # a role that would silently start from its seed again
        P.restore_host_state(info["host_state"], {"answers": a})


def test_a_numpy_sampler_of_the_caller_round_trips():
    rng = np.random.RandomState(11)
    rng.rand(3)
    st = json.loads(json.dumps(P.capture_host_state({"sampler": rng}, which=())))
    want = rng.rand(5).tolist()
    other = np.random.RandomState(0)
    P.restore_host_state(st, {"sampler": other})
    assert other.rand(5).tolist() == want and "torch" not in st


def test_save_refuses_centroids_it_does_not_understand(tmp_path):
    from streamchat_amd.sharded import Ref
    nodes, short = _tree()
    nodes[0].children[1].centroids = Ref([(1, 0, 0, 0, 4)])
    with pytest.raises((TypeError, ValueError), match=r"nodes\[0\]\.children\[1\].*chunk 1"):
        P.save_memory_tree(nodes, str(tmp_path / "t"), short)
    assert not os.listdir(tmp_path)                                        # nothing half written either
    # with a way to materialise them the rows are written
    rows = torch.full((4, 2, 4), 9.0, dtype=torch.float16)
    P.save_memory_tree(nodes, str(tmp_path / "t"), short, materialize=lambda ref: rows[:ref.rows])
    back, _, _ = P.load_memory_tree(str(tmp_path / "t"), device="cpu")
    assert torch.equal(back[0].children[1].centroids, rows)
    nodes[1].centroids = None                                              # None stays allowed (a node without features)
    P.save_memory_tree(nodes[1:], str(tmp_path / "n"))
    assert P.load_memory_tree(str(tmp_path / "n"), device="cpu")[0][0].centroids is None


def _same(a, b):
    assert a.text == b.text and a.depth == b.depth and len(a.children) == len(b.children) and torch.equal(a.centroids, b.centroids)
    for x, y in zip(a.children, b.children):
        _same(x, y)


@pytest.mark.parametrize("cut", ["tensor_write", "between_the_renames", "manifest_write"])
def test_a_save_cut_short_leaves_the_previous_checkpoint(tmp_path, monkeypatch, cut):
    nodes, short = _save(tmp_path)
    before = json.load(open(tmp_path / "video_0.json"))
    if cut == "tensor_write":                    # the tensor file stops half way
        real = P.save_file

        def half(tensors, filename, metadata=None):
            real(tensors, filename, metadata=metadata)
            with open(filename, "r+b") as f:
                f.truncate(os.path.getsize(filename) // 2)
            raise OSError("disk full")
        monkeypatch.setattr(P, "save_file", half)
    elif cut == "between_the_renames":           # the old tensor file has been parked, the new one is not in place yet
        real = os.replace
        calls = []

        def replace(a, b):
            calls.append(b)
            if len(calls) == 2:
                raise KeyboardInterrupt
            real(a, b)
        monkeypatch.setattr(P.os, "replace", replace)
    else:                                        # the new tensor file is in place, the manifest is not
        monkeypatch.setattr(P, "_write_json_atomic", lambda *a: (_ for _ in ()).throw(KeyboardInterrupt()))
    with pytest.raises((OSError, KeyboardInterrupt)):
        _save(tmp_path, scale=2.0, next_segment=3, answers=3, turns=3)
    monkeypatch.undo()
    assert json.load(open(tmp_path / "video_0.json")) == before
    assert P.find_checkpoint(str(tmp_path)) == str(tmp_path / "video_0")
    back, short2, extra, info = P.load_checkpoint(str(tmp_path / "video_0"), device="cpu")
    for a, b in zip(nodes, back):
        _same(a, b)
    assert torch.equal(short2[0], short[0]) and info["next_segment"] == 2 and info["answers"] == 2
    # the next save goes through and is the one found
    _save(tmp_path, scale=2.0, next_segment=3, answers=3, turns=3)
    back, _, _, info = P.load_checkpoint(P.find_checkpoint(str(tmp_path)), device="cpu")
    assert info["next_segment"] == 3 and torch.equal(back[0].centroids, torch.full((2, 2, 4), 2.0, dtype=torch.float16))
    assert sorted(os.listdir(tmp_path)) == ["video_0.json", "video_0.safetensors"]


def test_resume_with_other_settings_is_refused_by_name(tmp_path):
    _save(tmp_path)
    P.load_checkpoint(str(tmp_path / "video_0"), P.settings_fingerprint(SETTINGS, (2, 4), torch.float16), device="cpu")
    with pytest.raises(P.ResumeError, match="chunk_size"):
        P.load_checkpoint(str(tmp_path / "video_0"), P.settings_fingerprint(dict(SETTINGS, chunk_size=8), (2, 4), torch.float16), device="cpu")
    for field, fp in (("tau", P.settings_fingerprint(dict(SETTINGS, tau=6), (2, 4), torch.float16)),
                      ("sample_rate", P.settings_fingerprint(dict(SETTINGS, sample_rate=1.0), (2, 4), torch.float16)),
                      ("feature_row", P.settings_fingerprint(SETTINGS, (2, 8), torch.float16)),
                      ("feature_dtype", P.settings_fingerprint(SETTINGS, (2, 4), torch.bfloat16))):
        with pytest.raises(P.ResumeError, match=field):
            P.load_checkpoint(str(tmp_path / "video_0"), fp, device="cpu")
    with pytest.raises(ValueError, match="interval"):
        P.settings_fingerprint({k: v for k, v in SETTINGS.items() if k != "interval"})


def _save_as_format_1_without_resume_data(nodes, path, short, extra):
    """the files `save_memory_tree` wrote before checkpoints could resume: no save id, `extra` as the caller gave it"""
    from safetensors.torch import save_file
    tensors, seen = {}, {}
    manifest = dict(format="streamchat-memory-tree/1", nodes=P._walk(nodes, tensors, seen), short=[], extra=extra)
    for t in short:
        tensors[f"t{len(tensors)}"] = t.clone()
        manifest["short"].append(f"t{len(tensors) - 1}")
    save_file(tensors, path + ".safetensors", metadata=dict(format="streamchat-memory-tree/1"))
    json.dump(manifest, open(path + ".json", "w", encoding="utf-8"), ensure_ascii=False)


def test_files_without_resume_data_load_but_do_not_resume(tmp_path):
    nodes, short = _tree()
    _save_as_format_1_without_resume_data(nodes, str(tmp_path / "video_0"), short, dict(time=60, question="q"))
    m = json.load(open(tmp_path / "video_0.json"))
    assert "save_id" not in m and set(m["extra"]) == {"time", "question"}
    back, short2, extra = P.load_memory_tree(str(tmp_path / "video_0"), device="cpu")
    for a, b in zip(nodes, back):
        _same(a, b)
    assert extra == dict(time=60, question="q") and torch.equal(short2[0], short[0])
    with pytest.raises(P.ResumeError, match="no resume data"):
        P.load_checkpoint(str(tmp_path / "video_0"), device="cpu")
    with pytest.raises(P.ResumeError, match="no resume data"):             # the entry point's search says so too instead of starting over silently
        P.find_checkpoint(str(tmp_path))
    assert P.find_checkpoint(str(tmp_path / "nothing_here")) is None


def test_find_checkpoint_takes_the_furthest_complete_one(tmp_path):
    assert P.find_checkpoint(str(tmp_path)) is None
    nodes, short = _tree()
    st = P.capture_host_state()
    fp = P.settings_fingerprint(SETTINGS)
    for video, nxt in ((0, 3), (1, 1), (10, 2), (2, 1)):
        P.save_checkpoint(str(tmp_path), video, nodes, short, next_segment=nxt, segments=3, frames_consumed=[0, 1], answers=0, turns=0, host_state=st, fingerprint=fp)
    assert P.find_checkpoint(str(tmp_path)) == str(tmp_path / "video_10")
    os.remove(tmp_path / "video_10.safetensors")                           # incomplete: passed over
    assert P.find_checkpoint(str(tmp_path)) == str(tmp_path / "video_2")
    open(tmp_path / "video_2.json", "w").write("{ cut")
    assert P.find_checkpoint(str(tmp_path)) == str(tmp_path / "video_1")


def test_entry_point_has_the_resume_flag_and_trims_what_came_after_the_checkpoint(tmp_path):
    import inference_streaming_longva_v2 as E
    base = ["--video_dir", "v", "--model_name", "m", "--memory_basic_dir", "d", "--save_file", "s", "--annotations", "a", "--language", "en"]
    assert E.parse_args(base).resume_memory_tree is None
    assert E.parse_args(base + ["--resume_memory_tree", "x", "--memory_tree_dir", "x"]).resume_memory_tree == "x"
    out, mem = str(tmp_path / "out.json"), str(tmp_path / "memory_0.json")
    json.dump([dict(question=f"q{i}") for i in range(3)], open(out, "w"))
    json.dump({"User": {"name": "User", "history": {"2024-01-01": [dict(query="q0", response="a")],
                                                    "2024-01-02": [dict(query="q1", response="b"), dict(query="q2", response="c")]}}}, open(mem, "w"))
    E._truncate_session_files(out, mem, "User", answers=2, turns=2)
    assert [r["question"] for r in json.load(open(out))] == ["q0", "q1"]
    hist = json.load(open(mem))["User"]["history"]
    assert [t["query"] for day in hist.values() for t in day] == ["q0", "q1"]
    E._truncate_session_files(out, mem, "User", answers=2, turns=2)         # nothing beyond the checkpoint: files stay as they are
    assert len(json.load(open(out))) == 2
    with pytest.raises(SystemExit, match="3 answers"):
        E._truncate_session_files(out, mem, "User", answers=3, turns=2)
