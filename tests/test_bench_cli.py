"""bench.py's --dump-outputs writer (no GPU needed: the writer takes any torch tensors): whole arrays up to DUMP_SAMPLE
values, a fixed seeded sample of larger ones, stored as float64 that holds every u32 word exactly."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_whole_and_sampled(bench, tmp_path):
    import torch
    n_big = bench.DUMP_SAMPLE + 12345
    words = (np.arange(n_big, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32)).astype(np.uint32)
    small = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)
    outs = {"big": torch.from_numpy(words.view(np.int32)), "small": torch.from_numpy(small.view(np.int32))}
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), outs)
    a_big, a_small = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "small.npy")
    assert a_big.dtype == np.float64 and a_small.dtype == np.float64
    np.testing.assert_array_equal(a_small, small.astype(np.float64))  # whole, and the words above 2^31 stay unsigned
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, n_big, size=bench.DUMP_SAMPLE, dtype=np.int64))
    np.testing.assert_array_equal(a_big, words[pos].astype(np.float64))
    np.testing.assert_array_equal(a_big, np.load(tmp_path / "b" / "big.npy"))  # the same positions run to run
    assert 4 * 8 * bench.DUMP_SAMPLE <= 64 * 1000 * 1000  # the four arrays of a run stay under 64 MB
