"""CPU: the helpers behind `bench.py --dump-outputs DIR` - the seeded sample of a large output is the same elements every time and the
elements it names, a small output is kept whole, and what is written is float32 / float64 .npy files of at most 64 MB in all."""
import os

import numpy as np
import pytest
import torch

import bench


def test_small_outputs_are_kept_whole():
    a, b = torch.arange(10, dtype=torch.float16).view(2, 5), torch.arange(4.0)
    got = bench._sample([a, b], n=64)
    assert got.dtype == np.float32 and np.array_equal(got, np.concatenate([a.float().reshape(-1).numpy(), b.numpy()]))


def test_the_sample_of_a_large_output_is_fixed_and_exact():
    pieces = [torch.randn(30, 100).half(), torch.randn(7, 1000)]
    flat = np.concatenate([p.float().reshape(-1).numpy() for p in pieces])
    got = bench._sample(pieces, n=500, seed=3)
    assert got.dtype == np.float32 and got.shape == (500,)
    assert np.array_equal(got, bench._sample(pieces, n=500, seed=3))
    idx = np.sort(np.random.default_rng(3).integers(0, flat.size, 500))
    assert np.array_equal(got, flat[idx])
    assert (idx < 3000).any() and (idx >= 3000).any()          # both pieces are sampled


def test_ids_and_retrieved_frame_rows_are_float64():
    assert bench._ids(torch.tensor([[151643]])).tolist() == [151643.0]
    assert bench._ids([1, [2, 3], torch.tensor([4])]).tolist() == [1.0, 2.0, 3.0, 4.0]
    rows = bench._frame_rows([[("frame", 0, 3), ("centroid", 2, 1)], [("frame", 1, 7)]])
    assert rows.dtype == np.float64 and rows.tolist() == [[0, 0, 3], [1, 2, 1], [0, 1, 7]]


def test_dump_writes_float_npy_files_and_refuses_more_than_64_mb(tmp_path):
    arrays = dict(first_token=np.array([7.0]), encode_features=np.ones(1000, np.float32))
    shapes = bench.dump_outputs(arrays, str(tmp_path / "out"))
    assert shapes == dict(encode_features=[1000], first_token=[1])
    for k, v in arrays.items():
        back = np.load(os.path.join(str(tmp_path / "out"), k + ".npy"))
        assert back.dtype == v.dtype and np.array_equal(back, v)
    with pytest.raises(AssertionError):
        bench.dump_outputs(dict(big=np.zeros((64 << 20) // 4 + 1, np.float32)), str(tmp_path / "big"))
    with pytest.raises(AssertionError):
        bench.dump_outputs(dict(labels=np.zeros(4, np.int64)), str(tmp_path / "int"))
