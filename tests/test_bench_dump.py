"""bench.py --dump-outputs on the host: the files it writes from an engine's regions, and the seeded trajectory sample that
keeps a large shard within the size budget (the same rows in every file, the same rows on every run)."""
import importlib.util
import os

import numpy as np
import torch

from aslr_to_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Shard(object):
    """The part of aslr_to_amd.engine.Engine that dump_outputs reads, on host tensors whose values name their place."""

    def __init__(self, B, T, nx, nu):
        self.B, self.T = B, T
        self._xs = torch.arange((T + 1) * B * nx, dtype=torch.float64).view(T + 1, B, nx)
        self._us = -torch.arange(T * B * nu, dtype=torch.float64).view(T, B, nu)
        self._k = 0.5 * torch.arange(T * B * nu, dtype=torch.float64).view(T, B, nu)
        self._tf = torch.arange(_abi.TF_COUNT * B, dtype=torch.float64).view(_abi.TF_COUNT, B)

    xs = property(lambda s: s._xs.permute(1, 0, 2))
    us = property(lambda s: s._us.permute(1, 0, 2))

    def cut_u(self, v, axis=-1):
        return v

    def region(self, rid):
        assert rid == _abi.R_KFF
        return self._k

    def traj_f(self, row):
        return self._tf[row]


def test_dump_writes_batch_major_float64_arrays(tmp_path):
    bench = _bench_module()
    e = _Shard(B=6, T=4, nx=8, nu=2)
    bench.dump_outputs(e, str(tmp_path / "out"), 0, 1)
    got = {f: np.load(str(tmp_path / "out" / f)) for f in sorted(os.listdir(str(tmp_path / "out")))}
    assert sorted(got) == ["cost.npy", "k.npy", "stop.npy", "us.npy", "xs.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["xs.npy"], e._xs.permute(1, 0, 2).numpy())
    np.testing.assert_array_equal(got["us.npy"], e._us.permute(1, 0, 2).numpy())
    np.testing.assert_array_equal(got["k.npy"], e._k.transpose(0, 1).numpy())
    np.testing.assert_array_equal(got["cost.npy"], e._tf[_abi.TF_COST].numpy())
    np.testing.assert_array_equal(got["stop.npy"], e._tf[_abi.TF_STOP].numpy())


def test_a_shard_over_the_budget_is_cut_to_the_same_seeded_rows_in_every_file(tmp_path):
    bench = _bench_module()
    e = _Shard(B=100, T=4, nx=8, nu=2)
    per_traj = 8 * (5 * 8 + 4 * 2 + 4 * 2 + 2)
    bench.DUMP_BYTES = 30 * per_traj * 2   # two ranks: 30 trajectories each
    runs = []
    for run in range(2):
        d = tmp_path / ("run%d" % run)
        bench.dump_outputs(e, str(d), 1, 2)
        runs.append({f: np.load(str(d / f)) for f in os.listdir(str(d))})
    first, second = runs
    assert sorted(first) == ["cost_rank1.npy", "k_rank1.npy", "stop_rank1.npy", "us_rank1.npy", "xs_rank1.npy"]
    assert sum(a.nbytes for a in first.values()) <= bench.DUMP_BYTES // 2
    rows = (first["cost_rank1.npy"] - _abi.TF_COST * e.B).astype(int)   # cost of trajectory b is TF_COST * B + b
    assert len(rows) == 30 and (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(first["xs_rank1.npy"], e._xs.permute(1, 0, 2).numpy()[rows])
    np.testing.assert_array_equal(first["k_rank1.npy"], e._k.transpose(0, 1).numpy()[rows])
    np.testing.assert_array_equal(first["stop_rank1.npy"], e._tf[_abi.TF_STOP].numpy()[rows])
    for name, a in first.items():
        np.testing.assert_array_equal(a, second[name])
