"""tests/sync_anchor_ref.py proven on the CPU before tests/test_gpu_sync_anchor.py trusts it:

1. on every case of the table, on column worlds over the value set {NaN, +-0, +-subnormal, small negatives, 1, large, +inf} and
   on a randomised sweep of such worlds, ``min`` over the ranks of ``key_of(local argmin)`` names ``global_winner`` (which is
   ``torch.argmin`` of the concatenation and knows nothing about keys), and the numpy replay of the whole exchange passes
   ``check_exchange``: the check the kernels go through;
2. the check has teeth: every deliberately wrong restatement of ``SYNC_MUTATIONS`` is rejected on at least one case;
3. no hostile case is vacuous: each shows its event in a non-zero number of listed codes (printed; profiles/sync_anchor.txt
   keeps one run's lines).

No GPU is involved."""
import numpy as np
import pytest

import sync_anchor_ref as sr
from oracle import synth

SWEEP = 20000


def _replay_and_check(world, cap, mut=()):
    out = sr.exchange(world, cap, mut)
    sr.check_exchange(world, cap, out['keys'], out['reduced'], out['bufs'], out['totals'])


def _rejected(world, cap, mut) -> bool:
    try:
        _replay_and_check(world, cap, mut)
    except AssertionError:
        return True
    return False


_WORLDS = {}


def _world(sc):
    if sc.name not in _WORLDS:
        _WORLDS[sc.name] = sr.build_world(sc)
    return _WORLDS[sc.name]


def _fixed_column_worlds():
    """-0 on a low (rank, row) against +0 on a high one and the other way round; negatives of three sizes against zero and a
    positive; NaN on the highest rank and on two ranks; +inf everywhere at rank 255; ties inside one rank."""
    f = np.float32
    return [
        sr.column_world((3, 200), [np.array([[0.0, -0.0, 1.0], [1.0, 1.0, -0.0]], f), np.array([[-0.0, 0.0, 0.0], [0.0, 2.0, 1.0]], f)], seed=1),
        sr.column_world((9, 4, 130), [np.array([[-5.9604645e-08, 0.0, -1e-3]], f), np.array([[-1.1920929e-07, -1e-40, 5.9604645e-08]], f),
                                      np.array([[1e-3, -1e-45, -1.1920929e-07]], f)], seed=2),
        sr.column_world((0, 128, 255), [np.array([[1.0, np.nan], [0.5, 1.0]], f), np.array([[0.0, np.nan], [0.0, 0.0]], f),
                                        np.array([[2.0, 1.0], [np.nan, 3.0]], f)], seed=3),
        sr.column_world((255, 254), [np.full((4, 2), np.inf, f), np.full((3, 2), np.inf, f)], seed=4),
        sr.column_world((255,), [np.full((4, 2), np.inf, f)], seed=5),
    ]


@pytest.mark.parametrize('sc', sr.SYNC_CASES, ids=lambda sc: sc.name)
def test_min_of_keys_names_the_global_winner(sc):
    world = _world(sc)
    K, M = world['w'].shape[0], len(world['rows'])
    for cap in sr.caps(M, K):
        _replay_and_check(world, cap)
    ev = sr.events(world)
    print('\n' + sr.events_line(world, ev) + ' mismatches=0 (CPU replay; not a device run)', end='')
    for name in sr.REQUIRED_EVENTS[sc.hostile]:
        if name == 'cross_rank_ties' and len(sc.ranks) == 1:
            continue
        assert ev[name] > 0, f'{sc.name}: the case is built for {name} and shows none'
    assert M > 0 and sorted(world['rows'].tolist()) == world['rows'].tolist()


def test_case_table_covers_the_shape_and_world_classes():
    import update_ref as ur
    Ks = {ur.CVQ_CASES[c.ci].K for c in sr.SYNC_CASES}
    Ds = {ur.CVQ_CASES[c.ci].D for c in sr.SYNC_CASES}
    assert 1 in Ks and any(K % 64 for K in Ks) and any(K % 4 for K in Ks) and any(K % 64 == 0 for K in Ks)
    assert any(D < 64 for D in Ds) and any(D > 64 and D % 64 for D in Ds) and 256 in Ds
    worlds = {c.ranks for c in sr.SYNC_CASES}
    assert (0,) in worlds and (0, 1, 2) in worlds and (0, 7, 255) in worlds and any(list(r) != sorted(r) for r in worlds)
    assert any(len(set(_world(c)['xs'][r].shape[0] for r in range(len(c.ranks)))) > 1 for c in sr.SYNC_CASES)
    assert {c.hostile for c in sr.SYNC_CASES} >= {'dup', 'nan', 'nan_two', 'zero', 'unit', 'inf', 'ulp'}
    assert any(c.bf16 for c in sr.SYNC_CASES) and {c.metric for c in sr.SYNC_CASES} == set(sr.METRICS)
    assert len(sr.CHAIN_CASES) >= 6 and {c.hostile for c in sr.CHAIN_CASES} >= {'dup', 'nan', 'nan_two', 'zero', 'unit', 'ulp'}


def test_column_worlds_and_a_randomised_sweep():
    for world in _fixed_column_worlds():
        M = len(world['rows'])
        for cap in (M + 2, M, M // 2, 0):
            _replay_and_check(world, cap)
    g = synth.rng(20261)
    sizes = {}
    for _ in range(SWEEP):
        world = sr.random_column_world(g)
        M = len(world['rows'])
        _replay_and_check(world, M + int(g.integers(-1, 2)))
        sizes[len(world['ranks'])] = sizes.get(len(world['ranks']), 0) + 1
    print(f'\nsync_anchor sweep: {SWEEP} random column worlds of 1-4 ranks drawn from 0..255 {dict(sorted(sizes.items()))}: mismatches=0', end='')


def test_key_layout_and_its_limits():
    top = sr.key_of(np.inf, 255, sr.MAX_ROWS - 1)
    assert top < sr.INT64_MAX and top == 0x7F800001_FFFFFFFF
    field, rank, row = sr.decode([top])
    assert (int(field[0]), int(rank[0]), int(row[0])) == (0xFF800001, 255, sr.MAX_ROWS - 1)
    assert sr.key_of(np.nan, 0, 0) == -2 ** 63 and sr.key_of(np.nan, 255, 5) == -2 ** 63 + (255 << 24) + 5
    assert sr.key_of(-0.0, 3, 4) == sr.key_of(0.0, 3, 4)
    order = [np.nan, -np.inf, -1.0, -1.1920929e-07, -5.9604645e-08, -1e-45, 0.0, 1e-45, 5.9604645e-08, 1.0, 3e38, np.inf]
    keys = [sr.key_of(d, 255, sr.MAX_ROWS - 1) for d in order]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert all(sr.key_of(a, 255, sr.MAX_ROWS - 1) < sr.key_of(b, 0, 0) for a, b in zip(order, order[1:]))
    assert sr.key_of(1.0, 0, sr.MAX_ROWS - 1) < sr.key_of(1.0, 1, 0) < sr.key_of(1.0, 1, 1)


@pytest.mark.parametrize('winner', [(255, sr.MAX_ROWS - 1), (0, 1 << 23), None])
def test_bit_limits_of_the_rank_and_row_fields(winner):
    world = sr.bit_limit_world(winner)
    for cap in (1, 0):
        _replay_and_check(world, cap)
    out = sr.exchange(world, 1)
    field, rank, row = sr.decode(out['reduced'])
    assert (int(rank[0]), int(row[0])) == (winner or (0, 0))
    if winner == (255, sr.MAX_ROWS - 1):
        assert int(out['reduced'].view(np.uint64)[0] & np.uint64(0xFFFFFFFF)) == 0xFFFFFFFF
    if winner is None:
        assert int(out['keys'][1][0]) == sr.key_of(np.inf, 255, 0) < sr.INT64_MAX


def test_every_mutation_is_rejected_somewhere():
    """Every wrong restatement fails ``check_exchange`` on at least one world of the tables (walked here), and the case table of
    the GPU tests alone rejects every mutation a latent set can reach."""
    seen, seen_latent = set(), set()
    worlds = [(_world(sc), True) for sc in sr.SYNC_CASES] + [(wd, False) for wd in _fixed_column_worlds()]
    worlds += [(sr.bit_limit_world((255, sr.MAX_ROWS - 1)), False)]
    for world, latent in worlds:
        M, K = len(world['rows']), world['w'].shape[0]
        for mut in sorted(sr.SYNC_MUTATIONS - (seen_latent if latent else seen)):
            for cap in (min(K, M + 3), M // 2):
                if cap and _rejected(world, cap, (mut,)):
                    seen.add(mut)
                    if latent:
                        seen_latent.add(mut)
    assert seen == sr.SYNC_MUTATIONS, sr.SYNC_MUTATIONS - seen
    # -0 distances never leave the definition's arithmetic (sqrt of a clamped sum, 1 - c), and a 24-bit row needs 2^23 rows: the
    # column worlds and the bit-limit world (here) and the 2^24-row GPU test carry those two
    assert seen_latent == sr.SYNC_MUTATIONS - {'zero_not_folded', 'row_mask_23_bits'}, sr.SYNC_MUTATIONS - seen_latent
    print(f'\nsync_anchor mutations rejected: {sorted(seen)}; by the latent cases alone: {sorted(seen_latent)}', end='')
