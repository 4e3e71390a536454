"""The resident feed's epoch plan (osu_dreamer_amd/resident.py: EpochPlanner, shard_files): host integers only, no kernel, no store."""
import hashlib
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from osu_dreamer_amd.resident import EpochPlanner, shard_files
from osu_dreamer_amd.resident import ResidentBeatmapFeed

# 48 lengths of 20 .. 600 frames in a scrambled order, two too short for a 152-frame window, one of them empty
LENGTHS = [20 + (i * 37 % 59) * 10 for i in range(46)] + [0, 151]
PAD, BUDGET, CAP, POOL, MAX_LEN = 64, 1280, 16, 16, 500


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _bucketed(**kw):
    args = dict(batch_size=CAP, seq_len=None, max_len=MAX_LEN, pad_multiple=PAD, batch_frames=BUDGET, bucket_pool=POOL)
    args.update(kw)
    return EpochPlanner(LENGTHS[:46], **args)


def test_frame_budget_epoch_takes_every_map_once_within_the_budget():
    for pool in (POOL, 7, 1000):                                     # 46 maps: a partial last pool, an odd pool, one pool for everything
        plan = _bucketed(bucket_pool=pool).plan(_gen(1))
        maps = np.concatenate([pb.maps for pb in plan])
        assert sorted(maps.tolist()) == list(range(46)), pool        # every map exactly once: the partial last pool is cut too
        for pb in plan:
            B = len(pb.maps)
            assert 1 <= B <= CAP and B * pb.Lpad <= BUDGET, (pool, B, pb.Lpad)
            assert pb.Lpad % PAD == 0 and pb.Lpad - PAD < pb.lens.max() <= pb.Lpad
            L = np.asarray(LENGTHS)[pb.maps]
            assert (pb.lens == np.minimum(L, MAX_LEN)).all()         # a longer map contributes a max_len window that lies inside it
            assert (pb.starts >= 0).all() and (pb.starts + pb.lens <= L).all() and (pb.starts[L <= MAX_LEN] == 0).all()
    assert any((np.asarray(LENGTHS)[pb.maps] > MAX_LEN).any() for pb in plan)


def test_chunks_of_n_whole_maps_drop_the_partial_chunk():
    plan = EpochPlanner(LENGTHS[:46], batch_size=4, seq_len=None, max_len=MAX_LEN, pad_multiple=PAD).plan(_gen(2))
    assert len(plan) == 46 // 4 and all(len(pb.maps) == 4 for pb in plan)
    maps = np.concatenate([pb.maps for pb in plan])
    assert len(set(maps.tolist())) == 44
    for pb in plan:
        assert pb.Lpad == (int(pb.lens.max()) + PAD - 1) // PAD * PAD


@pytest.mark.parametrize("max_per_map", [-1, 1, 2])
def test_fixed_windows_lie_inside_their_map_and_never_overlap(max_per_map):
    T, B = 152, 8
    plan = EpochPlanner(LENGTHS, batch_size=B, seq_len=T, max_per_map=max_per_map).plan(_gen(3))
    assert plan and all(len(pb.maps) == B and pb.Lpad == T and (pb.lens == T).all() for pb in plan)
    per_map = {}
    for pb in plan:
        for m, s in zip(pb.maps.tolist(), pb.starts.tolist()):
            per_map.setdefault(m, []).append(s)
    L = np.asarray(LENGTHS)
    for m, starts in per_map.items():
        starts = sorted(starts)
        assert L[m] >= T, "a map shorter than the window contributes none"
        assert starts[0] >= 0 and starts[-1] + T <= L[m]
        assert starts[0] % T < min(T, L[m] - T + 1)                  # the grid's offset: start = randint(0, min(seq_len, end))
        assert all((b - a) % T == 0 and b - a >= T for a, b in zip(starts, starts[1:])), (m, starts)
        if max_per_map > 0:
            assert len(starts) <= max_per_map
    total = sum(len(v) for v in per_map.values())
    offered = sum(1 for n in LENGTHS if n >= T) if max_per_map == 1 else None
    if offered is not None:
        assert total == offered // B * B                              # one window per map that has one; the last partial batch is dropped
    if max_per_map == -1:                                             # every window of the grid is taken (up to the dropped partial batch)
        assert total > sum(1 for n in LENGTHS if n >= T) and any(len(v) == (L[m] - min(v) - T) // T + 1 for m, v in per_map.items())


def test_two_epochs_differ_and_a_seed_repeats():
    for planner in (_bucketed(), EpochPlanner(LENGTHS, batch_size=8, seq_len=152, max_per_map=1),
                    EpochPlanner(LENGTHS[:46], batch_size=4, seq_len=None, max_len=MAX_LEN)):
        g = _gen(5)
        first, second = planner.plan(g), planner.plan(g)
        again = planner.plan(_gen(5))
        key = lambda plan: [(pb.maps.tolist(), pb.starts.tolist(), pb.lens.tolist(), pb.Lpad) for pb in plan]   # noqa: E731
        assert key(first) == key(again)
        assert key(first) != key(second)


def test_rank_shards_are_disjoint_and_cover_the_files(tmp_path):
    names = []
    for i in range(7):
        d = tmp_path / f"{i:04d}"
        d.mkdir()
        for k in range(1 + i % 3):                                    # 1, 2 or 3 difficulties per mapset
            (d / f"{k}.latent.npz").write_bytes(b"")
            names.append(d / f"{k}.latent.npz")
    mapsets = sorted(tmp_path.iterdir())
    assert shard_files(mapsets) == names                              # LatentDataset._files() order
    for world in (2, 3):
        shards = [shard_files(mapsets, r, world) for r in range(world)]
        assert sorted(sum(shards, [])) == sorted(names) and sum(len(s) for s in shards) == len(names)
        assert all(s == names[r::world] for r, s in enumerate(shards))
        assert all(isinstance(f, Path) for s in shards for f in s)


# ---- the plans themselves: recorded from this file's helper, so that a change to the feed or the planner that moves one draw shows up
PLAN_LENGTHS = [70, 131, 120, 40, 9, 200]
PLAN_MODES = {
    "windows": dict(batch_size=2, seq_len=8),
    "windows_two_per_map": dict(batch_size=3, seq_len=37, max_per_map=2),
    "windows_one_per_map": dict(batch_size=2, seq_len=8, max_per_map=1),
    "chunks": dict(batch_size=2, seq_len=None, max_len=100, pad_multiple=64),
    "bucketed": dict(batch_size=4, seq_len=None, max_len=128, pad_multiple=64, batch_frames=256, bucket_pool=4),
}
# per mode and epoch: (batches, digest)
PLAN_EXPECTED = {
    "windows": [(33, "b6b35d528128c758"), (33, "59a9fc23156de9a7")],
    "windows_two_per_map": [(2, "8d92f5bd704d45ca"), (2, "7256cc9abaf3418a")],
    "windows_one_per_map": [(3, "dc3d683bf7dc1fba"), (3, "33a6f3e99563d238")],
    "chunks": [(3, "4c156ec0ede1c9e3"), (3, "6fdd0b4d2f2c9f2a")],
    "bucketed": [(3, "8fbd132f739e2cd0"), (3, "0e0f0c92274a7b23")],
}
BEATMAP_FEED_EXPECTED = [(33, "a5b622a4fcaa518e"), (33, "7f4949eca59e3fbf")]


def _plan_digest(plan):
    """(batches, sha256 over every batch's maps, starts, lens as int64, Lpad, and its flips as int32 where it has them)."""
    h = hashlib.sha256()
    for pb in plan:
        for a in (pb.maps, pb.starts, pb.lens):
            h.update(np.ascontiguousarray(a, dtype=np.int64).tobytes())
        h.update(np.int64(pb.Lpad).tobytes())
        if getattr(pb, "flips", None) is not None:
            h.update(b"flips" + np.ascontiguousarray(pb.flips, dtype=np.int32).tobytes())
    return len(plan), h.hexdigest()[:16]


@pytest.mark.parametrize("mode", sorted(PLAN_MODES))
def test_the_plans_of_a_seed_are_the_recorded_ones(mode):
    gen = _gen(1234)
    planner = EpochPlanner(PLAN_LENGTHS, **PLAN_MODES[mode])
    got = [_plan_digest(planner.plan(gen)) for _ in range(2)]
    assert got == PLAN_EXPECTED[mode]


def test_the_beatmap_feed_at_rank_one_plans_the_recorded_windows_and_flips():
    """The feed seeds its generator with torch.initial_seed() + 7919 * rank at the first epoch and draws every window's two flips behind
    the planner's draws; the store plays no part in a plan."""
    torch.manual_seed(1234)
    store = types.SimpleNamespace(device=torch.device("cpu"))
    feed = ResidentBeatmapFeed(store, EpochPlanner(PLAN_LENGTHS, batch_size=2, seq_len=8), rank=1)
    plans = [feed.plan_epoch() for _ in range(2)]
    assert all(pb.flips.dtype == np.int32 and pb.flips.shape == (2,) and ((pb.flips >= 0) & (pb.flips <= 3)).all() for p in plans for pb in p)
    got = [_plan_digest(p) for p in plans]
    assert got == BEATMAP_FEED_EXPECTED
