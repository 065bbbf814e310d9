"""Where a rank keeps its AdamW moments (coral_amd/trainer.py: state_layout) and the full <-> compact copies behind
`consolidate` / `load_moments`, on a toy bucket table without ranks or a GPU."""
import pytest
import torch

from coral_amd.trainer import copy_state, state_layout, state_size

# four buckets in backward-hook order, two sharded: a small replicated head, then a tail of 64 = 8 * world * k elements
BUCKETS = {"head": [176, 200], "layer1": [104, 176], "layer0": [32, 104], "front": [0, 32]}
SHARD = {"layer1": (112, 176), "layer0": (40, 104)}
NUMEL = 200


@pytest.mark.parametrize("world", [1, 2, 4])
def test_segments_inside_their_bucket_and_state_contiguous(world):
    for rank in range(world):
        layout = state_layout(BUCKETS, SHARD, rank, world)
        assert list(layout) == list(BUCKETS)
        n = 0
        for name, segs in layout.items():
            lo, hi = BUCKETS[name]
            assert len(segs) == (2 if name in SHARD else 1)
            pos = lo
            for a, b, so in segs:
                assert pos <= a < b <= hi  # inside the bucket, ordered, not empty
                assert so == n             # compact: contiguous from 0, bucket by bucket
                n += b - a
                pos = b
        assert state_size(layout) == n == sum(
            (SHARD[k][0] - lo) + (hi - SHARD[k][0]) // world if k in SHARD else hi - lo for k, (lo, hi) in BUCKETS.items())


@pytest.mark.parametrize("world", [1, 2, 4])
def test_replicated_ranges_agree_and_slices_partition_the_tails(world):
    layouts = [state_layout(BUCKETS, SHARD, r, world) for r in range(world)]
    for name, (lo, hi) in BUCKETS.items():
        if name not in SHARD:
            assert all(l[name] == layouts[0][name] for l in layouts) and layouts[0][name][0][:2] == (lo, hi)
            continue
        mlo = SHARD[name][0]
        assert all(l[name][0] == layouts[0][name][0] for l in layouts) and layouts[0][name][0][:2] == (lo, mlo)
        pos = mlo
        for l in layouts:  # rank by rank: equal slices, end to end
            a, b, so = l[name][1]
            assert a == pos and b - a == (hi - mlo) // world and so == layouts[0][name][1][2]
            pos = b
        assert pos == hi


def test_unsharded_state_has_the_parameters_layout():
    for rank, world in ((0, 1), (1, 2), (3, 4)):
        layout = state_layout(BUCKETS, {}, rank, world)
        assert {k: v for k, v in layout.items()} == {k: [(lo, hi, lo)] for k, (lo, hi) in BUCKETS.items()}
        assert state_size(layout) == NUMEL


@pytest.mark.parametrize("world", [1, 2, 4])
def test_load_moments_then_consolidate_round_trip(world):
    full = torch.randn(NUMEL, generator=torch.Generator().manual_seed(world))
    back = torch.full((NUMEL,), float("nan"))
    for rank in range(world):
        layout = state_layout(BUCKETS, SHARD, rank, world)
        compact = torch.full((state_size(layout),), float("nan"))
        copy_state(layout, compact, full, to_full=False)
        assert not compact.isnan().any()  # every element of the compact buffer belongs to a segment
        copy_state(layout, compact, back, to_full=True)
    assert torch.equal(back, full)
