"""GPU: `--resume_memory_tree` of the streaming entry point (tiny random-init architectures, synthetic videos, the flags of
tests/test_gpu_entrypoint.py).  A run that is stopped after the second answer of video 0 and started again with the same command line in a
NEW process writes the same answers, dialogue memories and memory trees as the run that was never interrupted - sampled (the reference's
temperatures, seeded) and greedy, whichever of `--overlap` / `--overlap 0` wrote the checkpoint and whichever resumes from it.  All
comparisons are equalities.  The one field left out is `process_time` of the results file: it is a wall-clock measurement.

Every run is a fresh child process (tests/_resume_child.py) whose exit status is checked before the next one starts."""
import json
import os
import shutil
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_resume_child.py")
STOPPED = 17


def _argv(d, *extra):
    return ["--video_dir", "none", "--model_name", "none", "--memory_basic_dir", os.path.join(d, "mem"), "--save_file", os.path.join(d, "out.json"),
            "--annotations", "none", "--language", "en", "--conv-mode", "qwen_1_5", "--synthetic", "2", "--synthetic_breakpoints", "3", "--tiny",
            "--chunk_size", "4", "--num_clusters", "2", "--interval", "3", "--short_window", "6", "--remember_window", "3", "--max_new_tokens", "12",
            "--multi_modal_memory", "--memory_tree_dir", os.path.join(d, "trees")] + list(extra)


def _child(d, *extra, stop_after=0, stop_mode="before", want=0):
    os.makedirs(d, exist_ok=True)
    env = dict(os.environ, SC_TEST_STOP_AFTER=str(stop_after), SC_TEST_STOP_MODE=stop_mode)
    r = subprocess.run([sys.executable, CHILD] + _argv(d, *extra), env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == want, f"exit status {r.returncode}, expected {want}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r


def _resume(d, *extra):
    return _child(d, "--resume_memory_tree", os.path.join(d, "trees"), *extra)


def _tree(path):
    from streamchat_amd.persistence import load_memory_tree
    nodes, short, extra = load_memory_tree(path, device="cpu")

    def one(n):
        return dict(text=n.text, depth=n.depth, rows=int(n.centroids.shape[0]), centroids=n.centroids, children=[one(c) for c in n.children])
    return dict(nodes=[one(n) for n in nodes], short=short, time=extra["time"], question=extra["question"], resume=extra.get("resume"))


def _results(d):
    out = json.load(open(os.path.join(d, "out.json")))
    assert all(set(r) == {"time", "question", "label", "predict", "class", "process_time"} for r in out)
    return dict(out=[{k: v for k, v in r.items() if k != "process_time"} for r in out],
                memory=[json.load(open(os.path.join(d, "mem", f"memory_{v}.json"))) for v in range(2)],
                trees=[_tree(os.path.join(d, "trees", f"video_{v}")) for v in range(2)])


def _equal(a, b, where=""):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f"{where}: tensors differ"
    elif isinstance(a, dict):
        assert set(a) == set(b), f"{where}: {sorted(a)} != {sorted(b)}"
        for k in a:
            _equal(a[k], b[k], f"{where}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), f"{where}: {len(a)} != {len(b)} entries"
        for i, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, f"{where}[{i}]")
    else:
        assert a == b, f"{where}: {a!r} != {b!r}"


def _check_complete(res):
    assert len(res["out"]) == 6 and [r["time"] for r in res["out"]] == [60, 120, 180] * 2
    for v in range(2):
        turns = [t for day in res["memory"][v]["User"]["history"].values() for t in day]
        assert [t["query"] for t in turns] == [r["question"] for r in res["out"][3 * v:3 * v + 3]]          # no question twice, none missing
        assert [t["response"] for t in turns] == [r["predict"] for r in res["out"][3 * v:3 * v + 3]]
        assert res["trees"][v]["resume"]["next_segment"] == 3 and res["trees"][v]["resume"]["answers"] == 3 * (v + 1)
        assert any(n["depth"] > 0 for n in res["trees"][v]["nodes"])                                        # merges (k-means draws) happened


def _stopped_state(d):
    """the checkpoint a stopped run left: everything but the save id"""
    assert not os.path.exists(os.path.join(d, "trees", "video_1.json"))
    t = _tree(os.path.join(d, "trees", "video_0"))
    assert t["resume"]["video"] == 0 and t["resume"]["next_segment"] == 2 and t["resume"]["answers"] == 2 and t["resume"]["turns"] == 2
    return t


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """the uninterrupted run: sampled (default temperature), seeded, default --overlap, one process"""
    d = str(tmp_path_factory.mktemp("reference"))
    _child(d)
    res = _results(d)
    _check_complete(res)
    return res


@pytest.fixture(scope="module")
def stopped_overlap(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("stopped_overlap"))
    _child(d, stop_after=2, want=STOPPED)
    assert len(json.load(open(os.path.join(d, "out.json")))) == 2
    return d


def _copy(src, tmp_path, name):
    """a stopped session's files under another directory (results, dialogue memories + index, checkpoints): resumed there"""
    d = str(tmp_path / name)
    shutil.copytree(src, d)
    return d


def test_stopped_and_resumed_run_equals_the_uninterrupted_run(reference, stopped_overlap, tmp_path):
    d = _copy(stopped_overlap, tmp_path, "resumed")
    r = _resume(d)
    assert "resuming from" in r.stdout and "next segment 2 of 3" in r.stdout
    got = _results(d)
    _check_complete(got)
    _equal(got, reference, "resumed")


def test_checkpoint_does_not_depend_on_overlap_and_resumes_under_either(reference, stopped_overlap, tmp_path):
    serial = str(tmp_path / "stopped_serial")
    _child(serial, "--overlap", "0", stop_after=2, want=STOPPED)
    # the checkpoint after answer 2 describes the session before segment 3 is read - whether or not a look-ahead thread had started on it
    _equal(_stopped_state(serial), _stopped_state(stopped_overlap), "checkpoint written with --overlap 0 / --overlap")
    a = _copy(serial, tmp_path, "serial_then_overlap")
    _resume(a)                                                              # written under --overlap 0, resumed under the default --overlap
    b = _copy(stopped_overlap, tmp_path, "overlap_then_serial")
    _resume(b, "--overlap", "0")                                            # and the other way round
    for name, d in (("serial_then_overlap", a), ("overlap_then_serial", b)):
        got = _results(d)
        _check_complete(got)
        _equal(got, reference, name)


def test_greedy_run_stopped_in_the_middle_of_a_round_resumes_without_a_duplicate(tmp_path):
    """--temperature 0; the stop comes after answer 3 has reached the results file but before its dialogue turn and checkpoint were written:
    the resumed run asks question 3 again and the results file holds it once."""
    ref, d = str(tmp_path / "reference"), str(tmp_path / "stopped")
    _child(ref, "--temperature", "0")
    want = _results(ref)
    _check_complete(want)
    _child(d, "--temperature", "0", stop_after=2, stop_mode="after_write", want=STOPPED)
    assert len(json.load(open(os.path.join(d, "out.json")))) == 3           # one answer beyond the checkpoint
    _stopped_state(d)
    _resume(d, "--temperature", "0")
    got = _results(d)
    _check_complete(got)
    _equal(got, want, "greedy")


def test_resume_flag_on_an_empty_directory_is_a_plain_run(reference, tmp_path):
    d = str(tmp_path / "fresh")
    os.makedirs(os.path.join(d, "trees"))
    r = _resume(d)
    assert "resuming from" not in r.stdout
    got = _results(d)
    _check_complete(got)
    _equal(got, reference, "first start with --resume_memory_tree")
