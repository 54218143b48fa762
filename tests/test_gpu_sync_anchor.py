"""The key exchange of NearestAnchor(sync=True) (``ops.cvq_col_keys``, ``ops.cvq_pack_sync``) replayed rank by rank in ONE process
on one GPU and held, bit for bit, to the definition of tests/sync_anchor_ref.py (proven on the CPU by
tests/test_sync_anchor_cpu.py).

Each of the two kernels takes its rank as a plain argument and the collectives between them are elementwise (a MIN of int64
keys, a SUM of fp32 buffers), so ``torch.stack(keys).amin(0)`` and a sum in two association orders stand in for them and a whole
world (ranks 0..255, unequal shards, calls in any rank order) needs no second process.  The comparisons of the keys, the
exchange, the bit limits and the one-call route are exact; the only tolerances are those of ``update_ref.cvq_tolerance`` on the
codebook the chain ends in.  Every test hands the kernels in-range ``rows`` / ``col_idx`` only.  Run with ``-s`` for the
per-case lines; profiles/sync_anchor.txt keeps one run's record.
"""
import numpy as np
import pytest
import torch

import sync_anchor_ref as sr
import update_ref as ur

pytestmark = pytest.mark.gpu

_WORLDS = {}


def _world(sc):
    """The case's world with its device tensors, built once and left unchanged."""
    if sc.name not in _WORLDS:
        world = sr.build_world(sc)
        dev = dict(e=torch.from_numpy(world['w']).cuda(), rows=torch.from_numpy(world['rows']).cuda(),
                   count=torch.tensor([len(world['rows'])], dtype=torch.int32, device='cuda'), x=[], xq=[], col=[], hist=[])
        eq = None
        for r, x in enumerate(world['xs']):
            xq, eq = sr.operands(world['metric'], x, world['w'])
            xt = torch.from_numpy(x).cuda()
            dev['x'].append(xt.bfloat16() if world['bf16'] else xt)          # the raw latents: the payload's source
            # L2 hands the column pass and the keys the latents as they are (bf16 included); cosine its fp32 normalised rows
            dev['xq'].append(dev['x'][r] if world['metric'] == 'L2' else torch.from_numpy(xq).cuda())
            dev['col'].append(torch.from_numpy(sr.local_argmin(world['cols'][r])).cuda())      # the C oracle's per-shard col_argmin
            dev['hist'].append(world['hists'][r].cuda())
        dev['eq'] = dev['e'] if world['metric'] == 'L2' else torch.from_numpy(eq).cuda()
        world['dev'] = dev
        _WORLDS[sc.name] = world
    return _WORLDS[sc.name]


def _keys(ops, world, cap, cols=None):
    dev = world['dev']
    return [ops.cvq_col_keys(dev['xq'][r], dev['eq'], dev['rows'], dev['count'], cap, (cols or dev['col'])[r], world['metric'], rank)
            for r, rank in enumerate(world['ranks'])]


def _pack(ops, world, cap, reduced):
    dev, K = world['dev'], world['w'].shape[0]
    return [ops.cvq_pack_sync(dev['hist'][r], world['xs'][r].shape[0], dev['x'][r], reduced, dev['count'], cap, K, rank)
            for r, rank in enumerate(world['ranks'])]


def _sum_two_orders(bufs):
    a, z = bufs[0], bufs[0]
    for b in bufs[1:]:
        a, z = a + b, b + z
    return a, z


def _replay(ops, world, cap, cols=None):
    """keys -> MIN -> pack -> SUM (two orders); checks the header and hands everything to ``check_exchange``.  Returns the sum."""
    K, D = world['w'].shape
    keys = _keys(ops, world, cap, cols)
    reduced = torch.stack(keys).amin(0)
    bufs = _pack(ops, world, cap, reduced)
    totals = _sum_two_orders(bufs)
    hist = sum(h.to(torch.int64) for h in world['hists'])
    numel = sum(x.shape[0] for x in world['xs'])
    for t in totals:
        assert t.numel() == 2 * K + 4 + cap * D
        back = ops.unpack_counts(t, K).cpu()
        assert torch.equal(back[:K], hist) and int(back[K]) == numel, 'the summed header is not the int64 sum of the histograms and token counts'
    head = 2 * K + 4
    sr.check_exchange(world, cap, [k.cpu().numpy() for k in keys], reduced.cpu().numpy(),
                      [b[head:].reshape(cap, D).cpu().numpy() for b in bufs], [t[head:].reshape(cap, D).cpu().numpy() for t in totals])
    return totals[0]


# ------------------------------------------------------------------------------------------------------------------
# a. the keys, in isolation
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('sc', sr.SYNC_CASES, ids=lambda sc: sc.name)
def test_keys_decode_to_their_inputs_and_the_oracles_distance(sc):
    from vector_quantization_amd import ops
    world = _world(sc)
    K, M = world['w'].shape[0], len(world['rows'])
    for cap in sr.caps(M, K):
        live = min(M, cap)
        for r, (rank, keys) in enumerate(zip(world['ranks'], _keys(ops, world, cap))):
            keys = keys.cpu().numpy()
            assert keys.shape == (cap,)
            loc = world['dev']['col'][r].cpu().numpy()[:live]
            field, rk, row = sr.decode(keys[:live])
            assert np.array_equal(rk, np.full(live, rank)) and np.array_equal(row, loc), f'{sc.name} rank {rank} cap {cap}: (rank, row)'
            want = sr.dist_field(world['cols'][r][loc, np.arange(live)])
            bad = np.nonzero(field.astype(np.uint64) != want)[0]
            assert bad.size == 0, (f'{sc.name} rank {rank} cap {cap}: {bad.size} of {live} distance fields differ from the C oracle\'s, first at '
                                   f'slot {bad[0]}: {int(field[bad[0]]):#x} against {int(want[bad[0]]):#x}')
            assert bool((keys[live:] == sr.INT64_MAX).all()), f'{sc.name} rank {rank} cap {cap}: slots past the count'
    print('\n' + sr.events_line(world, sr.events(world)) + ' key mismatches=0', end='')


# ------------------------------------------------------------------------------------------------------------------
# b. the exchange, replayed
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('sc', sr.SYNC_CASES, ids=lambda sc: sc.name)
def test_exchange_replayed_delivers_the_global_winners_rows(sc):
    from vector_quantization_amd import ops
    world = _world(sc)
    K, M = world['w'].shape[0], len(world['rows'])
    for cap in sr.caps(M, K):
        _replay(ops, world, cap)


# ------------------------------------------------------------------------------------------------------------------
# c. the chain: the column pass of the library, the exchange, the update
# ------------------------------------------------------------------------------------------------------------------

def _column_form(world, cap: int, N: int) -> str:
    """The form vqhip_col_argmin_rows takes (include/vqhip.h): a short list of fp32 rows runs the definition's own pass."""
    D = world['w'].shape[1]
    fp32 = world['metric'] != 'L2' or not world['bf16']
    return 'short_list' if fp32 and D % 4 == 0 and ((cap + 31) // 32) * ((N + 127) // 128) * D <= 2 ** 18 else 'pipeline'


def _envelope(world, r: int, slots: np.ndarray) -> np.ndarray:
    """tests/test_oracle_golden.py's envelope on a distance value, per listed code, from rank r's latents (L2)."""
    x, w = world['xs'][r].astype(np.float64), world['w'][world['rows'][slots]].astype(np.float64)
    eps = 2.0 ** -23
    mag_x = (x ** 2).sum(1).max()
    en = (w ** 2).sum(1)
    mag = mag_x + en + 2 * np.sqrt(mag_x * en)
    dmin = np.maximum(world['cols'][r][:, slots].min(0).astype(np.float64), 1e-30)
    return 4 * eps * mag / (2 * dmin) + 4 * eps * dmin


def _apply_reference(world, cap, payload):
    """``update_ref.cvq_reference`` with the anchors ``payload`` [cap, D] for the listed codes below the capacity, nothing for the
    others (w * decay), world = 1 (sync anchors are not averaged); codes with a non-finite anchor are returned apart."""
    c, inp = world['cvq'], world['inp']
    K, D = world['w'].shape
    w = torch.from_numpy(world['w'])
    slot = torch.full((K,), -1, dtype=torch.int64)
    slot[torch.from_numpy(world['rows']).long()] = torch.arange(len(world['rows']))
    payload = torch.from_numpy(payload)
    wild = ~torch.isfinite(payload).all(1)
    ext = torch.cat([torch.where(wild.unsqueeze(1), torch.zeros_like(payload), payload), torch.zeros(1, D)])
    col = torch.where((slot >= 0) & (slot < cap), slot, torch.full_like(slot, cap))
    hist = sum(h.to(torch.int64) for h in world['hists'])
    numel = sum(x.shape[0] for x in world['xs'])
    ref = ur.cvq_reference(w, inp['p'], hist, numel, ext, col, c.g, c.eps, 1)
    tol = ur.cvq_tolerance(w, inp['p'], hist, numel, ext[col].double().abs(), c.g, c.eps, c_anchor=0)
    wild_code = torch.cat([wild, torch.zeros(1, dtype=torch.bool)])[col]
    return ref, tol, slot.to(torch.int32), wild_code


@pytest.mark.parametrize('sc', sr.CHAIN_CASES, ids=lambda sc: sc.name)
def test_chain_column_pass_exchange_and_update_meet_the_reference(sc):
    from vector_quantization_amd import ops
    world = _world(sc)
    c, inp, dev = world['cvq'], world['inp'], world['dev']
    K, M = world['w'].shape[0], len(world['rows'])
    for cap in [v for v in sr.caps(M, K) if v]:
        live = min(M, cap)
        cols, forms = [], set()
        for r in range(len(world['ranks'])):
            col = ops.col_argmin_rows(dev['xq'][r], dev['eq'], dev['rows'], dev['count'], cap, world['metric'])
            forms.add(_column_form(world, cap, world['xs'][r].shape[0]))
            got, want = col.cpu().numpy()[:live], dev['col'][r].cpu().numpy()[:live]
            differ = np.nonzero(got != want)[0]
            if sc.hostile == 'ulp' and differ.size:         # the envelope rule of tests/test_oracle_golden.py, on the oracle's own distances
                gap = world['cols'][r][got[differ], differ].astype(np.float64) - world['cols'][r][want[differ], differ].astype(np.float64)
                assert bool((gap >= 0).all()) and bool((gap <= _envelope(world, r, differ)).all()), f'{sc.name}: a pick outside the envelope'
                col = dev['col'][r][:live]                   # the exchange below is then replayed from the oracle's picks
            else:
                assert differ.size == 0, f'{sc.name} rank {world["ranks"][r]} cap {cap}: {differ.size} local winners differ from the C oracle'
            cols.append(torch.cat([col[:live], torch.zeros(cap - live, dtype=torch.int64, device='cuda')]))
        packed = _replay(ops, world, cap, cols)
        _, win_row, win_pos = sr.winners_of(world)
        ref, tol, slot, wild = _apply_reference(world, cap, sr.expected_payload(world['xs'], (win_pos, win_row), M, cap))
        w_in, p_in = dev['e'].clone(), inp['p'].cuda().clone()
        w_out, p_out = torch.full_like(w_in, 7.0), torch.full_like(p_in, 7.0)
        ops.cvq_apply(w_in, w_out, p_in, p_out, slot.cuda(), ur.f32(c.g), ur.f32(c.eps), packed=packed, world=1, cap=cap)
        gw, gp = w_out.cpu(), p_out.cpu()
        nan = ur.nan_codes(inp['p'])
        assert bool(torch.isnan(gp[nan]).all()) and bool(torch.isnan(gw[nan]).all())
        assert not bool(torch.isfinite(gw[wild & ~nan]).all(1).any()), 'a non-finite anchor must leave a non-finite row'
        keep = ~(nan | wild)
        name = f'sync chain {sc.name} cap={cap}/{M} column pass={"+".join(sorted(forms))}'
        for what, got, key in (('p', gp[~nan], 'p'), ('w', gw[keep], 'w')):
            mask = ~nan if what == 'p' else keep
            v = ur.compare(got, ref[key][mask], tol[key][mask])
            print('\n' + v.line(f'{name} {what}'), end='')
            assert v.ok, v.line(f'{name} {what}')


def test_chain_cases_reach_both_forms_of_the_column_pass():
    forms = set()
    for sc in sr.CHAIN_CASES:
        world = _world(sc)
        for cap in [v for v in sr.caps(len(world['rows']), world['w'].shape[0]) if v]:
            forms |= {_column_form(world, cap, x.shape[0]) for x in world['xs']}
    assert forms == {'short_list', 'pipeline'}


# ------------------------------------------------------------------------------------------------------------------
# d. the bit limits: 2^24 rows per rank, ranks 0 and 255
# ------------------------------------------------------------------------------------------------------------------

def test_bit_limits_rank_255_row_2p24_minus_1():
    from vector_quantization_amd import ops
    N, D, K = sr.MAX_ROWS, 8, 2
    planted = sr.bit_limit_planted(D)
    last, mid = sr.MAX_ROWS - 1, 1 << 23
    xs = {}
    for rank in (0, 255):
        x = torch.zeros(N, D, dtype=torch.bfloat16, device='cuda')
        for row, v in planted[rank].items():
            x[row] = torch.from_numpy(v).cuda().bfloat16()
            assert torch.equal(x[row].float().cpu(), torch.from_numpy(v)), 'the planted rows are bf16 values'
        xs[rank] = x
    # code 0 is rank 255's last row, code 1 rank 0's row 2^23 (with +0.0 where the rows hold -0.0): distance 0 there, > 0 elsewhere
    e = torch.from_numpy(np.stack([planted[255][last], planted[0][mid]])).cuda().contiguous()
    e[:, 1] = 0.0
    rows = torch.arange(K, dtype=torch.int32, device='cuda')
    count = torch.tensor([K], dtype=torch.int32, device='cuda')
    col = {0: torch.tensor([last, mid], device='cuda'), 255: torch.tensor([last, mid], device='cuda')}
    keys = {rank: ops.cvq_col_keys(xs[rank], e, rows, count, K, col[rank], 'L2', rank) for rank in (0, 255)}
    for rank in (0, 255):
        field, rk, row = sr.decode(keys[rank].cpu().numpy())
        assert rk.tolist() == [rank, rank] and row.tolist() == [last, mid]
    reduced = torch.stack([keys[0], keys[255]]).amin(0)
    u = reduced.cpu().numpy().view(np.uint64)
    assert int(u[0] & np.uint64(0xFFFFFFFF)) == 0xFFFFFFFF, 'who of (255, 2^24 - 1)'
    assert int(reduced[0]) == sr.key_of(0.0, 255, last) and int(reduced[1]) == sr.key_of(0.0, 0, mid)
    hist = torch.tensor([3, 5], dtype=torch.int32, device='cuda')
    head = 2 * K + 4
    bufs = {rank: ops.cvq_pack_sync(hist, N, xs[rank], reduced, count, K, K, rank)[head:].reshape(K, D).cpu().numpy() for rank in (0, 255)}
    bits = {rank: np.ascontiguousarray(b).view(np.int32) for rank, b in bufs.items()}
    assert np.array_equal(bits[255][0], planted[255][last].view(np.int32)) and bool((bits[0][0] == sr.NEG_ZERO_BITS).all())
    assert np.array_equal(bits[0][1], planted[0][mid].view(np.int32)) and bool((bits[255][1] == sr.NEG_ZERO_BITS).all())
    for total in (bufs[0] + bufs[255], bufs[255] + bufs[0]):
        assert np.array_equal(total.view(np.int32), np.stack([planted[255][last], planted[0][mid]]).view(np.int32))
    # the host's refusals: a row or a rank that does not fit its field
    with pytest.raises(Exception, match='24 bits'):
        ops.cvq_col_keys(torch.zeros(N + 1, D, dtype=torch.bfloat16, device='cuda'), e, rows, count, K, col[0], 'L2', 0)
    with pytest.raises(Exception, match='24 bits'):
        ops.cvq_col_keys(xs[0], e, rows, count, K, col[0], 'L2', 256)
    with pytest.raises(Exception):
        ops.cvq_pack_sync(hist, N, xs[0], reduced, count, K, K, 256)


# ------------------------------------------------------------------------------------------------------------------
# e. the one-call route: vqhip_cvq_forward's BEFORE_EXCHANGE / PACK_SYNC / AFTER_EXCHANGE phases around recording callbacks
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('sc', sr.CHAIN_CASES, ids=lambda sc: sc.name)
def test_one_call_route_equals_the_hook_by_hook_replay(sc):
    from vector_quantization_amd import ops, train_step
    world = _world(sc)
    c, inp, dev = world['cvq'], world['inp'], world['dev']
    K, D = world['w'].shape
    g, eps = ur.f32(c.g), ur.f32(c.eps)
    p = inp['p'].cuda()
    rows, slot, count = ops.cvq_rows(p, K, g, eps)
    M = int(count.item())
    cap = min(K, M + 3)
    assert M > 0
    R, size = len(world['ranks']), max(world['ranks']) + 1

    def one_pass(keys_in, packed_in):
        rec = dict(keys=[], packed=[], out=[], w=[], p=[])
        for r, rank in enumerate(world['ranks']):
            def on_min(view, r=r):
                rec['keys'].append(view.clone())
                if keys_in is not None:
                    view.copy_(keys_in)

            def on_sum(view, r=r):
                rec['packed'].append(view.clone())
                if packed_in is not None:
                    view.copy_(packed_in)
            w_out, p_out = torch.full_like(dev['e'], 7.0), torch.full_like(p, 7.0)
            out = train_step.cvq_forward(dev['x'][r], dev['e'], p, w_out, p_out, world['metric'], g, eps, 0.25, train_step.CvqStepState(K, p.device, g, eps),
                                         cap=cap, list_ready=False, prefetch=False, exchange=True, world=size, comm=None, all_reduce=on_sum,
                                         tail=False, anchor_sync=True, rank=rank, all_reduce_min=on_min)
            assert out['cap_used'] == cap and out['exchange_floats'] == 2 * K + 4 + cap * D
            rec['out'].append(out), rec['w'].append(w_out), rec['p'].append(p_out)
        return rec
    first = one_pass(None, None)
    reduced = torch.stack(first['keys']).amin(0)
    second = one_pass(reduced, None)
    packed = _sum_two_orders(second['packed'])[0]
    third = one_pass(reduced, packed)
    # the hook-by-hook replay from the same inputs: the library's own column pass, the two kernels, the update
    keys, bufs = [], []
    for r, rank in enumerate(world['ranks']):
        out = first['out'][r]
        assert torch.equal(out['hist'].long(), torch.bincount(out['idx'], minlength=K))
        xq, eq = (dev['x'][r], dev['e']) if world['metric'] == 'L2' else (out['xq'], out['prepared'].exact_rows())
        col = ops.col_argmin_rows(xq, eq, rows, count, cap, world['metric'])
        keys.append(ops.cvq_col_keys(xq, eq, rows, count, cap, col, world['metric'], rank))
        assert torch.equal(keys[r], first['keys'][r]), f'{sc.name} rank {rank}: the one-call keys differ from the separate calls\''
    assert torch.equal(torch.stack(keys).amin(0), reduced)
    for r, rank in enumerate(world['ranks']):
        bufs.append(ops.cvq_pack_sync(first['out'][r]['hist'], world['xs'][r].shape[0], dev['x'][r], reduced, count, cap, K, rank))
        assert torch.equal(bufs[r].view(torch.int32), second['packed'][r].view(torch.int32)), f'{sc.name} rank {rank}: packed buffer'
    total = _sum_two_orders(bufs)[0]
    assert torch.equal(total.view(torch.int32), packed.view(torch.int32))
    w_ref, p_ref = torch.full_like(dev['e'], 7.0), torch.full_like(p, 7.0)
    ops.cvq_apply(dev['e'], w_ref, p, p_ref, slot, g, eps, packed=total, world=1, cap=cap)
    for r, rank in enumerate(world['ranks']):
        assert torch.equal(third['w'][r].view(torch.int32), w_ref.view(torch.int32)), f'{sc.name} rank {rank}: w_out'
        assert torch.equal(third['p'][r].view(torch.int32), p_ref.view(torch.int32)), f'{sc.name} rank {rank}: p_out'
