"""The key exchange of NearestAnchor(sync=True) across ranks, restated in plain Python and numpy: the definition the tests of
``ops.cvq_col_keys`` / ``ops.cvq_pack_sync`` hold the kernels to.

A plain helper module (not a conftest, no pytest settings), in the pattern of ``tests/update_ref.py``, whose case table and
per-rank latent sets it reuses.  ``tests/test_sync_anchor_cpu.py`` proves it on the CPU (``min`` over the ranks of
``key_of(local argmin)`` names ``global_winner`` on every case and on a randomised sweep, every mutation is rejected, every
hostile case shows its event); ``tests/test_gpu_sync_anchor.py`` replays whole worlds rank by rank on one GPU and compares bit
for bit through the same ``check_exchange``.

The definition (include/vqhip.h, vqhip_cvq_col_keys; vq/algorithms/cvqvae/anchors.py:50-57,83-84): the anchor of a code is the
latent at ``torch.argmin`` of the concatenation, in rank order, of every rank's distance column.  ``global_winner`` is that
sentence and knows nothing about keys.  ``key_of`` is the 64-bit word whose signed minimum over the ranks must name the same
latent:

    bits 63..32   the distance field: 0 for NaN, else m + 1 with m = ~b for a negative fp32 pattern b and b | 2^31 otherwise
                  (-0 folded into +0 first), so that the unsigned order of the field is torch.argmin's order of the distance
    bits 31..24   the rank        bits 23..0   the row
    the whole word with bit 63 flipped, read as int64; a slot past the count holds INT64_MAX.

A world here is a dict: ``ranks`` (the rank numbers in the order the calls are made), ``xs`` (per rank the latents, fp32 values),
``w``, ``rows`` (the listed codes, ascending), ``cols`` (per rank the [N_r, M] fp32 distances of its latents to the listed
codes, from the C oracle), ``metric``, ``bf16``, and the update's inputs (``p``, ``hists``, the ``CvqCase``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import update_ref as ur
from oracle import c_oracle as co, hostile, synth

INT64_MAX = 2 ** 63 - 1
ROW_BITS = 24
MAX_ROWS = 1 << ROW_BITS
MAX_RANKS = 256
_U64 = np.uint64
NEG_ZERO_BITS = np.int32(-2 ** 31)          # the int32 view of -0.0f


# ------------------------------------------------------------------------------------------------------------------
# the key
# ------------------------------------------------------------------------------------------------------------------

def dist_field(d, mut=()) -> np.ndarray:
    """uint64 distance field of fp32 distances (see the module docstring).  ``mut``: names of SYNC_MUTATIONS."""
    d = np.ascontiguousarray(d, np.float32).reshape(-1)
    b = d.view(np.uint32).astype(_U64)
    if 'zero_not_folded' not in mut:
        b = np.where(d == 0, _U64(0), b)
    neg = (b >> _U64(31)) == _U64(1)
    if 'negative_not_monotone' in mut:
        m = b | _U64(0x80000000)
    else:
        m = np.where(neg, ~b & _U64(0xFFFFFFFF), b | _U64(0x80000000))
    return np.where(np.isnan(d), _U64(0xFFFFFFFF if 'nan_last' in mut else 0), m + _U64(1))


def keys_of(d, rank: int, rows, mut=()) -> np.ndarray:
    """int64 keys of the distances ``d`` at the rows ``rows`` of rank ``rank``."""
    rows = np.asarray(rows).astype(_U64).reshape(-1)
    assert 0 <= rank < MAX_RANKS and (rows.size == 0 or int(rows.max()) < MAX_ROWS)
    r = _U64(255 - rank if 'ties_to_highest_rank' in mut else rank)
    who = (rows << _U64(8)) | r if 'fields_swapped' in mut else (r << _U64(ROW_BITS)) | rows
    u = (dist_field(d, mut) << _U64(32)) | who
    if 'top_bit_not_flipped' not in mut:
        u = u ^ _U64(1 << 63)
    return u.astype(_U64).view(np.int64)


def key_of(d, rank: int, row: int, mut=()) -> int:
    """The int64 key of one (distance, rank, row)."""
    return int(keys_of(np.float32(d), rank, [row], mut)[0])


def decode(keys, mut=()):
    """(distance field, rank, row) of int64 keys, as numpy int64 arrays."""
    u = np.ascontiguousarray(keys, np.int64).reshape(-1).view(_U64)
    if 'top_bit_not_flipped' not in mut:
        u = u ^ _U64(1 << 63)
    who = u & _U64(0xFFFFFFFF)
    if 'fields_swapped' in mut:
        rank, row = who & _U64(0xFF), who >> _U64(8)
    else:
        rank, row = who >> _U64(ROW_BITS), who & _U64((1 << (23 if 'row_mask_23_bits' in mut else ROW_BITS)) - 1)
    if 'ties_to_highest_rank' in mut:
        rank = _U64(255) - rank
    return (u >> _U64(32)).astype(np.int64), rank.astype(np.int64), row.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------
# the reference: torch.argmin of the concatenation, and the payload it implies
# ------------------------------------------------------------------------------------------------------------------

def global_winner(cols, shard_sizes):
    """``cols``: the ranks' distance columns [N_r, M] in RANK ORDER.  (index of the rank in that order [M], row [M]) of
    ``torch.argmin`` over their concatenation."""
    assert [c.shape[0] for c in cols] == list(shard_sizes)
    at = torch.argmin(torch.cat([torch.from_numpy(np.ascontiguousarray(c)) for c in cols]), dim=0).numpy()
    starts = np.concatenate([[0], np.cumsum(shard_sizes)])
    which = np.searchsorted(starts, at, side='right') - 1
    return which.astype(np.int64), (at - starts[which]).astype(np.int64)


def expected_payload(xs, winners, count: int, cap: int) -> np.ndarray:
    """fp32 [cap, D]: the winner's raw latent row for the slots below min(count, cap), +0.0 from the count up to cap.
    ``xs`` in the order ``winners[0]`` indexes."""
    which, row = winners
    D = xs[0].shape[1]
    out = np.zeros((cap, D), np.float32)
    for i in range(min(count, cap)):
        out[i] = xs[int(which[i])][int(row[i])]
    return out


def local_argmin(col: np.ndarray) -> np.ndarray:
    """A rank's own column pass: torch.argmin down every column of its [N_r, M] distances."""
    return torch.argmin(torch.from_numpy(np.ascontiguousarray(col)), dim=0).numpy().astype(np.int64)


def rank_order(world):
    """Positions of ``world['ranks']`` in ascending rank order."""
    return sorted(range(len(world['ranks'])), key=lambda i: world['ranks'][i])


def winners_of(world):
    """(rank number [M], row [M], position of that rank in the call order [M]) of the global winner of every listed code."""
    order = rank_order(world)
    which, row = global_winner([world['cols'][i] for i in order], [world['cols'][i].shape[0] for i in order])
    pos = np.asarray(order, np.int64)[which]
    return np.asarray(world['ranks'], np.int64)[pos], row, pos


def winning_distance(world) -> np.ndarray:
    _, row, pos = winners_of(world)
    return np.array([world['cols'][int(p)][int(r), i] for i, (p, r) in enumerate(zip(pos, row))], np.float32)


# ------------------------------------------------------------------------------------------------------------------
# the exchange, replayed in numpy (the stand-in the mutations are applied to), and the check both sides go through
# ------------------------------------------------------------------------------------------------------------------

SYNC_MUTATIONS = {'nan_last', 'zero_not_folded', 'negative_not_monotone', 'fields_swapped', 'row_mask_23_bits',
                  'top_bit_not_flipped', 'ties_to_highest_rank', 'payload_averaged', 'plus_zero_from_non_winners',
                  'filler_not_int64_max'}


def exchange(world, cap: int, mut=()) -> dict:
    """The three steps in numpy: per rank the key of its local winner, the elementwise MIN, per rank the packed payload (the
    winner its row, everybody else -0.0, +0.0 past the count), the SUM in two association orders.  Returns dict(keys, reduced,
    bufs, totals)."""
    M, D, R = len(world['rows']), world['w'].shape[1], len(world['ranks'])
    live = min(M, cap)
    keys = []
    for r, rank in enumerate(world['ranks']):
        col = world['cols'][r]
        loc = local_argmin(col)[:live] if live else np.zeros(0, np.int64)
        k = np.full(cap, 0 if 'filler_not_int64_max' in mut else INT64_MAX, np.int64)
        k[:live] = keys_of(col[loc, np.arange(live)], rank, loc, mut)
        keys.append(k)
    reduced = np.minimum.reduce(keys) if cap else np.zeros(0, np.int64)
    _, rk, row = decode(reduced[:live], mut)
    bufs = []
    for r, rank in enumerate(world['ranks']):
        buf = np.zeros((cap, D), np.float32)
        buf[:live] = np.float32(0.0 if 'plus_zero_from_non_winners' in mut else -0.0)
        mine = np.nonzero(rk == rank)[0]
        buf[mine] = world['xs'][r][np.minimum(row[mine], world['xs'][r].shape[0] - 1)]
        bufs.append(buf)
    return dict(keys=keys, reduced=reduced, bufs=bufs, totals=sums_in_two_orders(bufs, R if 'payload_averaged' in mut else 1))


def sums_in_two_orders(bufs, divide_by: int = 1):
    """(b0 + b1) + b2 ... and b2 + (b1 + b0) ...: the SUM all-reduce in two association orders."""
    with np.errstate(all='ignore'):
        a = bufs[0]
        for b in bufs[1:]:
            a = a + b
        z = bufs[0]
        for b in bufs[1:]:
            z = b + z
        if divide_by != 1:
            a, z = a / np.float32(divide_by), z / np.float32(divide_by)
    return [a, z]


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check_exchange(world, cap: int, keys, reduced, bufs, totals) -> None:
    """What a replayed exchange (numpy or the kernels) owes the definition, bit for bit; raises AssertionError.
    keys: per rank int64 [cap]; reduced: int64 [cap]; bufs: per rank fp32 [cap, D] payloads; totals: their sums."""
    M = len(world['rows'])
    live = min(M, cap)
    ranks = np.asarray(world['ranks'], np.int64)
    win_rank, win_row, win_pos = winners_of(world)
    for r, rank in enumerate(world['ranks']):                      # every rank's own key: its local winner, its distance
        col = world['cols'][r]
        loc = local_argmin(col)[:live]
        field, rk, row = decode(np.asarray(keys[r])[:live])
        assert np.array_equal(rk, np.full(live, rank)) and np.array_equal(row, loc), f'rank {rank}: the key does not name its own (rank, row)'
        assert np.array_equal(field.astype(_U64), dist_field(col[loc, np.arange(live)])), f'rank {rank}: distance field'
        assert bool((np.asarray(keys[r])[live:] == INT64_MAX).all()), f'rank {rank}: slots past the count must hold INT64_MAX'
    field, rk, row = decode(np.asarray(reduced)[:live])
    assert np.array_equal(rk, win_rank[:live]) and np.array_equal(row, win_row[:live]), 'the reduced key does not name the global winner'
    assert np.array_equal(field.astype(_U64), dist_field(winning_distance(world)[:live])), 'the reduced key does not carry the winning distance'
    assert bool((np.asarray(reduced)[live:] == INT64_MAX).all()), 'reduced slots past the count must hold INT64_MAX'
    assert bool((np.asarray(reduced)[:live] < INT64_MAX).all()), 'a live key must beat the INT64_MAX filler'
    want = expected_payload(world['xs'], (win_pos, win_row), M, cap)
    for t in totals:
        assert np.array_equal(_bits(t), _bits(want)), 'the summed payload is not the winners\' rows bit for bit'
    for r in range(len(ranks)):
        b = _bits(bufs[r])
        lost = np.nonzero(win_pos[:live] != r)[0]
        assert bool((b[lost] == NEG_ZERO_BITS).all()), f'rank {ranks[r]}: a slot it lost must hold -0.0'
        won = np.nonzero(win_pos[:live] == r)[0]
        assert np.array_equal(b[won], _bits(want[won])), f'rank {ranks[r]}: a slot it won must hold its row'
        assert not b[live:].any(), f'rank {ranks[r]}: slots past the count must hold +0.0'


# ------------------------------------------------------------------------------------------------------------------
# distances of the definition (the C oracle) and the operands the kernels are handed
# ------------------------------------------------------------------------------------------------------------------

METRICS = ('L2', 'Cosine', 'CosineBF16')


def dist_columns(metric: str, x: np.ndarray, w: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """fp32 [N, M]: the C oracle's distances of the latents ``x`` to the listed codes ``w[rows]``."""
    e = np.ascontiguousarray(w[rows])
    with np.errstate(all='ignore'):
        if metric == 'L2':
            return co.l2_dist(x, e)
        if metric == 'Cosine':
            return co.cos_dist(x, e)
        # bf16 autocast: the oracle has the row minimum only; against ONE code that minimum is the distance itself
        return np.stack([co.cos_bf16_argmin(x, e[i:i + 1], with_min=True)[1] for i in range(e.shape[0])], axis=1).astype(np.float32)


def operands(metric: str, x: np.ndarray, w: np.ndarray):
    """(xq, eq) as the column pass and ``cvq_col_keys`` are handed them: the latents and the codebook for L2, both normalised
    (and bf16-rounded under the bf16 autocast metric) for cosine."""
    if metric == 'L2':
        return x, w
    with np.errstate(all='ignore'):
        xq, eq = co.normalize_rows(x), co.normalize_rows(w)
    if metric == 'CosineBF16':
        xq, eq = synth.bf16_round(xq), synth.bf16_round(eq)
    return xq, eq


# ------------------------------------------------------------------------------------------------------------------
# case table
# ------------------------------------------------------------------------------------------------------------------

@dataclass
class SyncCase:
    name: str
    ci: int                    # index into update_ref.CVQ_CASES: K, D, g, eps, the codebook, p and the three latent sets
    metric: str
    ranks: tuple               # rank numbers in the order the calls are made
    sizes: tuple               # rows per rank (clipped to the case's N)
    hostile: Optional[str]     # None, 'dup', 'nan', 'nan_two', 'zero', 'unit', 'inf', 'ulp'
    bf16: bool = False


def _ci(K: int, D: int, j: int) -> int:
    return 5 * ur.SHAPES.index((K, D)) + j


BIG = 10 ** 6                  # "the whole set": clipped to the case's N
# K = 1; K no multiple of 64 (5, 1027, 257, 130) and of 4 (5, 1027, 257, 130); D < 64 (1, 8, 24, 63), a tail past 64 (65), 256
SYNC_CASES = [
    SyncCase('k1_d1_l2_one_rank', _ci(1, 1, 0), 'L2', (0,), (BIG,), 'dup'),
    SyncCase('k1_d1_cos_dup', _ci(1, 1, 1), 'Cosine', (0, 7, 255), (BIG, BIG, BIG), 'dup'),
    SyncCase('k5_d8_l2_unequal', _ci(5, 8, 0), 'L2', (0, 1, 2), (300, 1, 777), None),
    SyncCase('k5_d8_cos_nan_high', _ci(5, 8, 1), 'Cosine', (255, 0, 7), (BIG, BIG, BIG), 'nan'),
    SyncCase('k5_d8_cosbf16', _ci(5, 8, 2), 'CosineBF16', (0, 1, 2), (BIG, 400, BIG), 'dup'),
    SyncCase('k1027_d24_l2_dup', _ci(1027, 24, 0), 'L2', (0, 7, 255), (BIG, BIG, BIG), 'dup'),
    SyncCase('k1027_d24_cos_unit', _ci(1027, 24, 1), 'Cosine', (0, 1, 2), (BIG, BIG, BIG), 'unit'),
    SyncCase('k1027_d24_l2_nan_two_bf16', _ci(1027, 24, 2), 'L2', (2, 0, 1), (300, 1, 777), 'nan_two', True),
    SyncCase('k257_d63_l2_zero', _ci(257, 63, 0), 'L2', (2, 0, 1), (BIG, BIG, BIG), 'zero'),
    SyncCase('k257_d63_cos_bf16', _ci(257, 63, 1), 'Cosine', (0, 1, 2), (300, 1, 777), 'dup', True),
    SyncCase('k130_d65_l2_inf', _ci(130, 65, 0), 'L2', (0, 7, 255), (BIG, BIG, BIG), 'inf'),
    SyncCase('k130_d65_l2_bf16_nan', _ci(130, 65, 1), 'L2', (7, 255, 0), (300, 1, 777), 'nan', True),
    SyncCase('k64_d256_cos_unit', _ci(64, 256, 0), 'Cosine', (0, 7, 255), (BIG, BIG, BIG), 'unit'),
    SyncCase('k64_d256_l2_ulp', _ci(64, 256, 1), 'L2', (0, 1, 2), (BIG, BIG, BIG), 'ulp'),
    SyncCase('k64_d256_l2_zero_bf16', _ci(64, 256, 2), 'L2', (255, 7, 0), (BIG, 300, BIG), 'zero', True),
]
# what every hostile kind must show (names of ``events``), each in a non-zero number of listed codes
REQUIRED_EVENTS = {'dup': ('cross_rank_ties', 'same_rank_ties'), 'nan': ('nan_winners',), 'nan_two': ('nan_winners', 'cross_rank_ties'),
                   'zero': ('zero_winners', 'cross_rank_ties', 'neg_zero_rows'), 'unit': ('negative', 'mixed_sign'),
                   'inf': ('inf_winners', 'cross_rank_ties'), 'ulp': ('one_ulp_apart',), None: ()}
CHAIN_CASES = [c for c in SYNC_CASES if ur.CVQ_CASES[c.ci].D % 8 == 0]     # the column pass and the one-call step need D % 8 == 0


def _event_codes(K: int, g, n: int = 8) -> np.ndarray:
    lo = 2 if K >= 8 else 0                      # (the codebook's rows 0 and 1 are the 2^60 / 2^-60 rows where K leaves room)
    return np.sort(g.choice(np.arange(lo, K), size=min(n, K - lo), replace=False))


def _plant(xs, i: int, vs) -> None:
    """Event ``i``: its latent(s) ``vs`` (one per rank position, cycled) go to a HIGH row of the first rank that has room, to a
    low row of the next, to a second row there, and on every third event to a third rank — so that the lowest (rank, row) is
    neither the lowest row nor the last written."""
    room = [r for r in range(len(xs)) if xs[r].shape[0] >= 64]
    a = room[i % len(room)]
    b = room[(i + 1) % len(room)]
    xs[a][xs[a].shape[0] - 1 - i] = vs[a % len(vs)]
    xs[b][i] = vs[b % len(vs)]
    xs[b][i + xs[b].shape[0] // 2] = vs[b % len(vs)]
    if i % 3 == 0 and len(room) >= 3:
        c = room[(i + 2) % len(room)]
        xs[c][i + xs[c].shape[0] // 4] = vs[c % len(vs)]


def build_world(sc: SyncCase) -> dict:
    c = ur.CVQ_CASES[sc.ci]
    inp = ur.cvq_inputs(c)
    K, D, R = c.K, c.D, len(sc.ranks)
    g = synth.rng(c.seed + 77)
    w = inp['w'].numpy().copy()
    xs = [inp['ranks'][r]['x'].numpy()[:min(sc.sizes[r], c.N)].copy() for r in range(R)]
    ev = _event_codes(K, g)
    if sc.hostile == 'ulp':                      # oracle/hostile.py's family, dealt out row by row; far codes for the planted pairs
        x, w = hostile.make('ulp_pairs', c.seed, sum(v.shape[0] for v in xs), K, D)
        xs = [np.ascontiguousarray(x[r::R][:xs[r].shape[0]]) for r in range(R)]
        w[ev] = g.standard_normal((len(ev), D), dtype=np.float32)
    if sc.bf16:
        xs = [synth.bf16_round(v) for v in xs]
    rnd = (lambda v: synth.bf16_round(v)) if sc.bf16 else (lambda v: v)
    if sc.hostile == 'dup':                      # (a) the same latent on two or three ranks and at two rows of one
        for i, k in enumerate(ev):
            v = rnd((w[k] + np.float32(1e-4) * g.standard_normal(D, dtype=np.float32)).astype(np.float32))
            _plant(xs, i, [v])
    elif sc.hostile == 'zero':                   # (c) a latent EQUAL to an integer-valued code: exact +0; (e) -0.0 where the code is 0
        for i, k in enumerate(ev):
            w[k] = g.integers(-2, 3, D).astype(np.float32)
            w[k, i % D] = 0.0
            v = w[k].copy()
            v[w[k] == 0] = -0.0
            _plant(xs, i, [v])
    elif sc.hostile == 'unit':                   # (c) rows that normalise to a code's unit row up to rounding: 1 - c of either sign
        ev = _event_codes(K, g, 48)
        scales = np.array([1.0, 0.3, 3.7, 1.1 / 32, 7.3, 0.77], np.float32)
        for i, k in enumerate(ev):
            _plant(xs, i, [rnd((w[k] * scales[(i + r) % 6]).astype(np.float32)) for r in range(R)])
    elif sc.hostile in ('nan', 'nan_two'):       # (b) a NaN distance on a high rank only / on two ranks
        hi = sorted(range(R), key=lambda r: (xs[r].shape[0] >= 64, sc.ranks[r]))[::-1]
        for r in hi[:2 if sc.hostile == 'nan_two' else 1]:
            # L2: one +inf element poisons the columns whose code is >= 0 there (inf - inf), the others see +inf; cosine: a NaN row
            xs[r][5 + r, 0] = np.inf if sc.metric == 'L2' else np.nan
    elif sc.hostile == 'inf':                    # (d) oracle/hostile.py's huge rows, every row: |x|^2 overflows, every distance is +inf
        xs = [hostile._f32(v * np.float32(3e19)) for v in xs]
    listed = (g.random(K) < 0.67) if K > 1 else np.ones(1, bool)
    listed[ev] = True
    rows = np.nonzero(listed)[0].astype(np.int32)
    world = dict(case=sc, cvq=c, inp=inp, ranks=tuple(sc.ranks), xs=xs, w=w, rows=rows, metric=sc.metric, bf16=sc.bf16, events=ev,
                 p=inp['p'], hists=[inp['ranks'][r]['hist32'] for r in range(R)])
    _columns(world)
    if sc.hostile == 'ulp':
        _plant_ulp_neighbours(world, g)
        _columns(world)
    return world


def _columns(world) -> None:
    world['cols'] = [dist_columns(world['metric'], x, world['w'], world['rows']) for x in world['xs']]


def _plant_ulp_neighbours(world, g) -> None:
    """(g) For the far codes of the case: a copy of the code's nearest latent, moved by a few ulps in one coordinate until the C
    oracle's distance differs from the winner's by exactly one unit of the key's distance field, on another rank."""
    R = len(world['ranks'])
    slot_of = {int(k): i for i, k in enumerate(world['rows'])}
    for n, k in enumerate(world['events']):
        i = slot_of[int(k)]
        _, row, pos = winners_of(world)
        a, v = int(pos[i]), world['xs'][int(pos[i])][int(row[i])]
        f0 = int(dist_field(world['cols'][a][int(row[i]), i])[0])
        cands = np.repeat(v[None], 6 * v.size, axis=0)
        for j in range(v.size):
            for s, step in enumerate((1, -1, 2, -2, 3, -3)):
                cands[6 * j + s, j] = (v[j:j + 1].view(np.int32) + step).view(np.float32)[0]
        f = dist_field(co.l2_dist(cands, world['w'][k:k + 1])).astype(np.int64)
        near = np.nonzero(np.abs(f - f0) == 1)[0]
        if near.size:
            b = (a + 1 + n % (R - 1)) % R
            world['xs'][b][3 * n + 1] = cands[near[0]]
            _columns(world)


# ------------------------------------------------------------------------------------------------------------------
# events: what actually occurs in the listed codes of a world
# ------------------------------------------------------------------------------------------------------------------

def events(world) -> dict:
    cols, M = world['cols'], len(world['rows'])
    _, win_row, win_pos = winners_of(world)
    dwin = winning_distance(world)
    fwin = dist_field(dwin)
    out = dict(listed=M, cross_rank_ties=0, same_rank_ties=0, nan_winners=int(np.isnan(dwin).sum()), negative=int((dwin < 0).sum()),
               mixed_sign=0, zero_winners=int((dwin == 0).sum()), inf_winners=int(np.isposinf(dwin).sum()), neg_zero_rows=0, one_ulp_apart=0)
    for i in range(M):
        fl = [dist_field(c[:, i]) for c in cols]
        hit = [int((f == fwin[i]).sum()) for f in fl]
        out['cross_rank_ties'] += int(sum(h > 0 for h in hit) >= 2)
        out['same_rank_ties'] += int(hit[int(win_pos[i])] >= 2)
        mins = np.array([f.min() for f in fl]).astype(np.int64)
        dmin = [c[local_argmin(c[:, i:i + 1])[0], i] for c in cols]
        out['mixed_sign'] += int(any(d < 0 for d in dmin) and any(d >= 0 for d in dmin))
        order = np.argsort(mins, kind='stable')
        out['one_ulp_apart'] += int(len(mins) >= 2 and mins[order[1]] - mins[order[0]] == 1)
        v = world['xs'][int(win_pos[i])][int(win_row[i])]
        out['neg_zero_rows'] += int(((v == 0) & np.signbit(v)).any())
    return out


def events_line(world, ev: dict) -> str:
    sc = world['case']
    return (f"sync_anchor {sc.name}: metric={sc.metric} bf16={sc.bf16} ranks={sc.ranks} rows={tuple(x.shape[0] for x in world['xs'])} "
            f"hostile={sc.hostile} listed={ev['listed']} cross_rank_ties={ev['cross_rank_ties']} same_rank_ties={ev['same_rank_ties']} "
            f"nan_winners={ev['nan_winners']} negative={ev['negative']} mixed_sign={ev['mixed_sign']} zero_winners={ev['zero_winners']} "
            f"inf_winners={ev['inf_winners']} neg_zero_rows={ev['neg_zero_rows']} one_ulp_apart={ev['one_ulp_apart']}")


def caps(M: int, K: int):
    """A capacity above the count, one below it, and none at all."""
    return sorted({min(K, M + 3), M // 2, 0}, reverse=True)


# ------------------------------------------------------------------------------------------------------------------
# column worlds: distance columns given directly (CPU only: a kernel computes its own distances), for what no latent set
# reaches — -0 distances, negative distances of several sizes, subnormals, and the limits of the rank and row fields
# ------------------------------------------------------------------------------------------------------------------

VALUE_SET = np.array([np.nan, 0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, -5.9604645e-08, -1.1920929e-07, -1e-3, 1.0, 1.0000001, 3e38,
                      np.inf], np.float32)


def column_world(ranks, cols, D: int = 3, seed: int = 0) -> dict:
    """A world whose columns are handed in; latents are random rows with a -0.0 in every one."""
    g = synth.rng(seed)
    xs = []
    for c in cols:
        x = g.standard_normal((c.shape[0], D), dtype=np.float32)
        x[:, 0] = -0.0
        xs.append(x)
    M = cols[0].shape[1]
    return dict(case=None, ranks=tuple(ranks), xs=xs, w=np.zeros((M, D), np.float32), rows=np.arange(M, dtype=np.int32),
                cols=[np.ascontiguousarray(c, np.float32) for c in cols], metric=None, bf16=False)


def random_column_world(g) -> dict:
    R = int(g.integers(1, 5))
    ranks = tuple(int(r) for r in g.choice(256, size=R, replace=False))
    M = int(g.integers(1, 6))
    few = VALUE_SET[g.choice(len(VALUE_SET), size=int(g.integers(1, 5)), replace=False)]      # few distinct values: ties are the rule
    cols = [few[g.integers(0, len(few), (int(g.integers(1, 7)), M))] for _ in range(R)]
    return column_world(ranks, cols, seed=int(g.integers(1 << 30)))


class SparseRows:
    """[N, D] fp32 rows that are zero except for a few planted ones: the latents of a rank with 2^24 rows, without the memory."""

    def __init__(self, N: int, D: int, planted: dict) -> None:
        self.shape, self.planted = (N, D), planted

    def __getitem__(self, rows):
        if np.ndim(rows) == 0:
            return self.planted.get(int(rows), np.zeros(self.shape[1], np.float32))
        return np.stack([self[int(r)] for r in rows]) if len(rows) else np.zeros((0, self.shape[1]), np.float32)


BIT_LIMIT_ROWS = (0, 1 << 23, MAX_ROWS - 1)


def bit_limit_planted(D: int = 8):
    """rank -> {row: a bf16-valued latent with a -0.0 element} at rows 0, 2^23 and 2^24 - 1 of ranks 0 and 255."""
    out = {}
    for rank in (0, 255):
        out[rank] = {}
        for j, row in enumerate(BIT_LIMIT_ROWS):
            v = np.arange(1, D + 1, dtype=np.float32) * np.float32(-(1 + j) if rank else 1 + j)
            v[1] = -0.0
            out[rank][row] = v
    return out


def bit_limit_world(winner) -> dict:
    """Two ranks (0, 255) of 2^24 rows, one listed code whose column is +inf except at the planted rows: every planted row holds
    1.0 except ``winner`` = (rank, row), which holds 0.5.  winner None: every entry is +inf (the key at rank 255 is then the
    largest a live slot can carry below the filler... and the winner is (0, 0))."""
    planted = bit_limit_planted()
    cols = []
    for rank in (0, 255):
        c = np.full((MAX_ROWS, 1), np.inf, np.float32)
        if winner is not None:
            c[list(BIT_LIMIT_ROWS), 0] = 1.0
            if winner[0] == rank:
                c[winner[1], 0] = 0.5
        cols.append(c)
    world = column_world((0, 255), cols, D=8)
    world['xs'] = [SparseRows(MAX_ROWS, 8, planted[0]), SparseRows(MAX_ROWS, 8, planted[255])]
    world['w'] = np.zeros((1, 8), np.float32)
    return world
