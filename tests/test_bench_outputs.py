"""bench.py --dump-outputs on CPU: the files' names, dtype and contents, and the 64 MB limit's fixed
sample (the same elements from run to run, so two builds can be compared output for output)."""
import numpy as np

import bench


def test_small_outputs_are_written_whole_as_float64(tmp_path):
    idx = np.array([7, 3, 4_000_000_000], dtype=np.uint32)
    sums = np.linspace(-1.0, 1.0, 11)
    shapes = bench.dump_outputs(str(tmp_path / 'out'), {'indices': idx, 'running_sums': sums})
    assert shapes == {'indices': [3], 'running_sums': [11]}
    got = np.load(tmp_path / 'out' / 'indices.npy')
    assert got.dtype == np.float64 and got.tolist() == [7.0, 3.0, 4e9]
    np.testing.assert_array_equal(np.load(tmp_path / 'out' / 'running_sums.npy'), sums)


def test_float32_stays_float32(tmp_path):
    bench.dump_outputs(str(tmp_path), {'a': np.arange(4, dtype=np.float32)})
    assert np.load(tmp_path / 'a.npy').dtype == np.float32


def test_over_the_limit_a_fixed_sample_is_kept(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 64 * 1024)
    big = np.arange(20_000, dtype=np.float64).reshape(5_000, 4)   # 160 kB: over its 32 kB share
    small = np.arange(10, dtype=np.float64)
    s1 = bench.dump_outputs(str(tmp_path / 'r1'), {'big': big, 'small': small})
    s2 = bench.dump_outputs(str(tmp_path / 'r2'), {'big': big + 0.5, 'small': small})
    assert s1 == s2 and s1['small'] == [10]
    files = list((tmp_path / 'r1').iterdir())
    assert sum(f.stat().st_size for f in files) <= 64 * 1024
    a, b = np.load(tmp_path / 'r1' / 'big.npy'), np.load(tmp_path / 'r2' / 'big.npy')
    assert a.ndim == 1 and 1_000 < a.size < big.size
    assert np.all(np.diff(a) > 0) and np.all(np.isin(a, big))   # elements of big, ascending positions
    np.testing.assert_array_equal(b, a + 0.5)                   # the same positions in the second run
