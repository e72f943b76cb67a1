"""bench.py --dump-outputs: the file holds the out of the replica the last
timed step wrote, whole when it fits the byte budget and else a sample that is
the same for every run (sorted flat indices from default_rng(0)); N ranks
write their own shard regions only; the positions where the source is not
finite are left out, so every file is finite.  CPU only: plain torch tensors
stand in for the device outs."""

import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

NAN_AT = (1, 2, 3)  # inside the first of the two regions below


@pytest.fixture
def outs(monkeypatch):
    rng = np.random.default_rng(3)
    arrs = [rng.standard_normal((8, 6, 4), dtype=np.float32) for _ in range(4)]
    finite = np.ones((8, 6, 4), bool)
    finite[NAN_AT] = False
    for a in arrs:  # every replica decodes the same source: the NaN sits at one place
        a[NAN_AT] = np.nan
    items = [(None, None, None, (slice(0, 4), slice(0, 6), slice(0, 4))),
             (None, None, None, (slice(4, 8), slice(0, 6), slice(0, 4)))]
    monkeypatch.setattr(bench, "HEADLINE_OUTS", [(torch.from_numpy(a), items) for a in arrs])
    monkeypatch.setattr(bench, "HEADLINE_FINITE", [finite])
    return arrs, finite


def _ctx(world=1, rank=0):
    return types.SimpleNamespace(world=world, rank=rank)


def test_dump_is_the_last_steps_replica_without_the_source_nan(outs, tmp_path):
    arrs, finite = outs
    bench.dump_outputs(_ctx(), 7, str(tmp_path))  # steps 0..6 rotate over 4 replicas: the last is replica 2
    got = np.load(tmp_path / "headline_out.npy")
    assert got.dtype == np.float32 and got.shape == (8 * 6 * 4 - 1,)
    assert np.isfinite(got).all()
    assert got.tobytes() == arrs[2][finite].tobytes()


def test_dump_of_an_all_finite_source_keeps_its_shape(outs, tmp_path, monkeypatch):
    arrs, finite = outs
    arrs[1][NAN_AT] = 0.5
    monkeypatch.setattr(bench, "HEADLINE_FINITE", [np.ones_like(finite)])
    bench.dump_outputs(_ctx(), 2, str(tmp_path))
    got = np.load(tmp_path / "headline_out.npy")
    assert got.shape == (8, 6, 4) and got.tobytes() == arrs[1].tobytes()


def test_dump_keeps_a_non_finite_value_the_source_does_not_have(outs, tmp_path):
    arrs, finite = outs
    arrs[0][5, 0, 0] = np.inf  # a wrong decode must show in the file
    bench.dump_outputs(_ctx(), 1, str(tmp_path))
    assert np.isinf(np.load(tmp_path / "headline_out.npy")).sum() == 1


def test_dump_sample_is_fixed_and_within_budget(outs, tmp_path, monkeypatch):
    arrs, finite = outs
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100 * 4)
    bench.dump_outputs(_ctx(), 4, str(tmp_path / "a"))
    bench.dump_outputs(_ctx(), 8, str(tmp_path / "b"))
    a, b = np.load(tmp_path / "a" / "headline_out.npy"), np.load(tmp_path / "b" / "headline_out.npy")
    idx = np.sort(np.random.default_rng(0).choice(arrs[3].size, 100, replace=False))
    idx = idx[finite.reshape(-1)[idx]]
    assert a.shape == (len(idx),) and 99 <= len(idx) <= 100 and a.tobytes() == b.tobytes()
    assert a.tobytes() == arrs[3].reshape(-1)[idx].tobytes()


def test_dump_of_a_rank_is_its_own_regions(outs, tmp_path):
    arrs, finite = outs
    bench.dump_outputs(_ctx(world=2, rank=1), 1, str(tmp_path))
    got = np.load(tmp_path / "headline_out_rank1.npy")
    want = np.stack([arrs[0][:4], arrs[0][4:]])
    assert np.isfinite(got).all() and got.tobytes() == want[np.isfinite(want)].tobytes()
