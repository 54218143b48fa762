"""The hostile input families of oracle/hostile.py bite — proved on the CPU, before any kernel sees them.

tests/test_gpu_hostile.py requires the HIP kernels to return the C oracle's indices on these families.  That is only a test
of the margin machinery (row_margin, the flush accounting, the inf / NaN routing, the slow paths) if a library WITHOUT it
would fail on them.  For every family x metric x D this file checks, at N = 1024, K = 2048:

* the C oracle runs, stays in [0, K) and agrees with a float64 argmin on every row whose float64 gap between the best and
  the second best code exceeds the rounding slop S of the fp32 definition (restated below in numpy; rows
  inside the slop are the oracle's to decide: counted and printed here, NOT excluded from the GPU tests);
* the family has the property it is named for, from the restated image rules (hostile.image_shares);
* THE MUTATION: hostile.bare_fp16_argmin — argmax of the fp16 proposal score with no margin behind it — differs from the
  oracle on at least 1 row in 10 for families 1, 2, 3 (s = 28), 4, 5, 9 at L2 and for every family that reaches that share
  at cosine (MUTATION_COS below: measured with bare_fp16_argmin, then required).  Cosine normalises the code scales of
  family 3 and the row scales of families 4-6 and 9 away by construction (a normalised row has entries <= 1 and a norm
  of 1: nothing overflows, and only rows of large D lose entries below 2^-14), so their cosine share is printed, and
  asserted to be what normalisation leaves: under 1 in 10.  Families 6, 7, 8 and code_outliers(s = 12) are kept for the BRANCHES they enter (all-zero token images, the
  clamped codebook shift, non-finite statistics, exact ties), not for a share: none is asserted for them;
* determinism: sha256 of every (x, w) against constants written here.
"""
import functools

import numpy as np
import pytest

from oracle import c_oracle as co, hostile, synth

N, K = 1024, 2048
SEED = 20261016
DIMS = [8, 32, 256, 768]
U = 2.0 ** -24
F32_MAX = float(np.finfo(np.float32).max)

# families whose bare-proposal error share must reach 1 in 10
MUTATION_L2 = {'channel_scale', 'channel_scale_two', 'channel_offset', 'code_outliers_s28', 'row_scales', 'huge_rows',
               'huge_rows_1e16', 'huge_rows_3e19', 'mixed'}
MUTATION_L2.add('channel_offset_2p28')
MUTATION_COS = {'channel_scale', 'channel_scale_two'}
# cosine normalises these away — every row and every code is divided by its own norm before the images are made — so the
# share must stay UNDER 1 in 10 (it is what normalisation leaves).  channel_offset is printed only: at +3000 0.9 at D = 8
# and under 0.02 from D = 32 on (the hot channel's fp16 rounding is the same for every code: common mode); at +2^28 the fp32
# DEFINITION no longer tells the codes apart (every similarity rounds to 1: index 0 everywhere, for the bare proposal too)
NORMALISED_AWAY_COS = {'code_outliers_s12', 'code_outliers_s28', 'row_scales', 'huge_rows', 'huge_rows_1e16', 'huge_rows_3e19',
                       'tiny_rows', 'tiny_rows_all', 'mixed'}

SHA = {}   # filled below: (case, D) -> 'sha(x)[:16]:sha(w)[:16]'


@functools.lru_cache(maxsize=4)
def _inputs(case, D):
    return hostile.make(case, SEED, N, K, D)


def l2_slop(x, w):
    """S of row_margin() per row, in squared-distance units (float64): the D-term fma chain, the two additions and the sqrt
    tie window of the fp32 definition, plus (not in row_margin: its scores cannot see it) the absolute error of fp32
    underflow, 2^-149 per operation.  inf where the fp32 definition itself overflows: such a row is the oracle's to decide."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    D = x.shape[1]
    xn = np.sqrt((x64 ** 2).sum(1))
    e2 = (w64 ** 2).sum(1)
    emax, enmax = np.sqrt(e2.max()), e2.max()
    mag = xn * xn + enmax + 2.0 * xn * emax
    s = 2.0 * (1.01 * D * U * 2.0 * xn * emax + 2.1 * U * mag) + 4.0 * U * mag + (4 * D + 8) * 2.0 ** -149
    return np.where(mag < F32_MAX, s, np.inf)


def cos_slop(xn, wn):
    """The definition's share of row_margin()'s cosine branch, in similarity units."""
    D = xn.shape[1]
    a = np.sqrt((xn.astype(np.float64) ** 2).sum(1))
    e = np.sqrt((wn.astype(np.float64) ** 2).sum(1).max())
    return 2.0 * (D + 4.0) * U * a * e + 8.0 * U + (2 * D + 8) * 2.0 ** -149


def float64_argmin(x, w, metric):
    """(index, gap between best and second best, slop) per row in float64 — x, w normalised fp32 rows for cosine."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        if metric == 'L2':
            cost = (x64 ** 2).sum(1)[:, None] - 2.0 * (x64 @ w64.T) + (w64 ** 2).sum(1)[None, :]
            slop = l2_slop(x, w)
        else:
            cost = -(x64 @ w64.T)
            slop = cos_slop(x, w)
    two = np.partition(cost, 1, axis=1)[:, :2]
    return cost.argmin(1), two[:, 1] - two[:, 0], slop


def report(case, metric, D):
    """Everything this file asserts about one case, as a dict (also what profiles/hostile_inputs.txt tabulates)."""
    x, w = _inputs(case, D)
    if metric == 'L2':
        xe, we = x, w
        ref = co.l2_argmin(x, w)
    else:
        xe, we = co.normalize_rows(x), co.normalize_rows(w)
        ref = co.cos_argmin(x, w)
    i64, gap, slop = float64_argmin(xe, we, metric)
    decided = gap > slop
    bare = hostile.bare_fp16_argmin(xe, we, metric)
    sh = hostile.image_shares(xe, we, metric)
    return dict(x=x, w=w, ref=ref, i64=i64, decided=decided, shares=sh,
                wrong_decided=int(((ref != i64) & decided).sum()), inside=int((~decided).sum()),
                mutation=float((bare != ref).mean()))


def check_property(case, metric, r, D):
    """The property each family is named for, from its parameters (L2: the raw inputs meet the images; the cosine images
    see normalised rows, where only the codebook-side properties of families 1-3 survive)."""
    sh, x, w = r['shares'], r['x'], r['w']
    kind = hostile.CASES[case][0]
    every5, every3 = len(range(0, N, 5)), len(range(0, N, 3))
    if kind in ('channel_scale', 'channel_offset'):
        # the hot channel sits at 2^11 .. 2^14 of a scale whose fp16 ulp there is 2 .. 4 unscaled units: the worst of 2048
        # codes is rounded by more than the planted noise (0.3) in that channel alone
        if metric == 'L2':
            assert sh['cb_resid_max'] >= 0.5, sh
        c = D // 3
        assert np.abs(w[:, c]).mean() >= 500 * np.abs(np.delete(w, c, 1)).mean()
    elif case == 'code_outliers_s28' and metric == 'L2':
        assert sh['cb_flushed'] >= 0.98, sh
    elif case == 'code_outliers_s12' and metric == 'L2':
        assert sh['cb_flushed'] <= 0.01, sh                       # the image keeps the small codes: the margin's easy side
        out = np.arange(96, K, 97)
        assert np.abs(w[out]).mean() >= 2000 * np.abs(np.delete(w, out, 0)).mean()
    elif metric == 'Cosine' and kind in ('row_scales', 'huge_rows', 'tiny_rows'):
        assert sh['x_inf_rows'] == 0 and sh['x_zero_rows'] <= (every5 if case == 'huge_rows_3e19' else 0), sh
    elif kind == 'row_scales':
        # 2^U{-20..20}: 6 of 41 exponents flush every entry and -14..-10 a falling share (>= 0.15 in all); 17..20 overflow
        # most entries and 15, 16 some (>= 0.08)
        assert sh['x_flushed'] >= 0.15 and sh['x_inf'] >= 0.08, sh
    elif kind == 'huge_rows':
        assert sh['x_inf_rows'] >= every5, sh
        x2 = (x[::5].astype(np.float64) ** 2).sum(1)
        f = hostile.CASES[case][1].get('factor', 1e6)
        if f == 1e16:
            assert (x2 >= 1e30).all() and (x2 < F32_MAX).all()     # past the margin's magnitude guard, finite in fp32
        if f == 3e19:
            assert (x2 > F32_MAX).all() and np.isfinite(x).all()   # |x|^2 overflows fp32, x itself does not
    elif case == 'tiny_rows':
        assert sh['x_zero_rows'] == every3, sh
    elif case == 'tiny_rows_all':
        assert sh['x_zero_rows'] == N, sh
    elif kind == 'codebook_scale' and metric == 'L2':
        s = hostile.CASES[case][1].get('s')
        if case == 'codebook_scale_subnormal':
            assert (np.abs(w) < 2.0 ** -126).all() and (w != 0).mean() > 0.99 and sh['cb_flushed'] >= 0.99, sh
        elif s == -120:
            assert sh['cb_scale'] == 2.0 ** 100 and sh['cb_flushed'] >= 0.99, sh      # the clamp leaves the image empty
        elif s == 55:
            e2 = (w.astype(np.float64) ** 2).sum(1)
            assert e2.max() < F32_MAX and e2.max() >= 1e30 and sh['x_inf_rows'] == 0, sh   # only the magnitude guard is left
        elif s == -90:
            assert sh['cb_scale'] == 2.0 ** 100 and sh['cb_flushed'] <= 0.01 and sh['x_zero_rows'] == N, sh
        else:
            # |e|^2 overflows fp32: non-finite statistics (scale 1, no bound); the latents, scaled alike, overflow fp16
            with np.errstate(over='ignore'):
                assert np.isinf((w ** 2).sum(1, dtype=np.float32)).all() and np.isfinite(w).all()
            assert sh['cb_scale'] == 1.0 and sh['x_inf_rows'] == N, sh
    elif kind == 'ulp_pairs':
        assert hostile.count_ulp_pairs(w) == K // 2
    elif kind == 'mixed' and metric == 'L2':
        assert sh['cb_flushed'] >= 0.98 and sh['x_inf_rows'] >= N // 8 and sh['x_zero_rows'] >= N // 8, sh


@pytest.mark.parametrize('D', DIMS)
@pytest.mark.parametrize('case', list(hostile.CASES))
def test_determinism(case, D):
    x, w = _inputs(case, D)
    assert x.dtype == np.float32 and w.dtype == np.float32 and x.shape == (N, D) and w.shape == (K, D)
    assert np.isfinite(x).all() and np.isfinite(w).all()        # hostile, but every INPUT is a finite fp32 number
    assert f'{synth.sha(x)[:16]}:{synth.sha(w)[:16]}' == SHA[case, D]


@pytest.mark.parametrize('D', DIMS)
@pytest.mark.parametrize('metric', ['L2', 'Cosine'])
@pytest.mark.parametrize('case', list(hostile.CASES))
def test_family_bites(case, metric, D):
    r = report(case, metric, D)
    ref = r['ref']
    assert ref.shape == (N,) and ref.min() >= 0 and ref.max() < K
    print(f"{case}/{metric}/D={D}: inside the slop {r['inside']} of {N}, bare fp16 proposal wrong on {r['mutation']:.3f}, "
          + ' '.join(f'{k}={v:.4g}' for k, v in r['shares'].items()))
    assert r['wrong_decided'] == 0, f"the oracle disagrees with float64 on {r['wrong_decided']} rows outside the fp32 slop"
    check_property(case, metric, r, D)
    required = MUTATION_L2 if metric == 'L2' else MUTATION_COS
    if case in required:
        assert r['mutation'] >= 0.1, f"the bare proposal is wrong on only {r['mutation']:.3f} of the rows"
    elif metric == 'Cosine' and case in NORMALISED_AWAY_COS:
        assert r['mutation'] < 0.1, r['mutation']


SHA.update({
    ('channel_scale', 8): 'b851288bfec54c53:5eab4dd7c128619e',
    ('channel_scale', 32): '051368c1bfc77ff0:2063460848887e3b',
    ('channel_scale', 256): '47cde47885336cb1:176344f480be855a',
    ('channel_scale', 768): '48e01bfdc5811bd9:31886b372cdb0cc9',
    ('channel_scale_two', 8): 'd022e2a4b44c676c:29a6afe345939d21',
    ('channel_scale_two', 32): 'ed17331216c0ad5e:ccfc4bcc0a45fc19',
    ('channel_scale_two', 256): '05689d7ff15e3601:7e70e774f33f4054',
    ('channel_scale_two', 768): '98dbf0085943c9bb:fd13cf2adf64048c',
    ('channel_offset', 8): 'c09fbb6e223d39bb:ab940b79201ba8d2',
    ('channel_offset', 32): '6723ea7ee37f89f9:2462341009b490d2',
    ('channel_offset', 256): '12a6b2a2ba7d98f8:3291d8d608374571',
    ('channel_offset', 768): '33175bc0cf8e69c6:507bca0d0cb1ec8a',
    ('channel_offset_2p28', 8): '01b5a106bd8e96e1:781c0a0963817de2',
    ('channel_offset_2p28', 32): '11f926e0ccef3ccc:1abbb6b8bcf678f7',
    ('channel_offset_2p28', 256): 'c4d4c1006414b257:24079dff7dfb49df',
    ('channel_offset_2p28', 768): '61e96984a9ce704f:c42a16d18e720d47',
    ('code_outliers_s12', 8): '8507f78240c0fa3e:18fbf526e10ea3e4',
    ('code_outliers_s12', 32): '0d4baf74432bef4b:97a48b5642702244',
    ('code_outliers_s12', 256): 'ea73595d3d73d601:866ced8ba6130f75',
    ('code_outliers_s12', 768): '2da298d2e4b130ff:c38e0cc326768965',
    ('code_outliers_s28', 8): '08629458376a67e1:69a286502e1683ec',
    ('code_outliers_s28', 32): '085dec471dcb6176:a45057f73e149bb2',
    ('code_outliers_s28', 256): '5772d567ca388a6e:ed4f77c26b16e620',
    ('code_outliers_s28', 768): 'a151d2b348326a9e:a2a84fcd119649cb',
    ('row_scales', 8): '56183ef1b1f396fe:efa8050c9b4f124f',
    ('row_scales', 32): '1d0f059193764029:e033e6b51bb1fada',
    ('row_scales', 256): '431f1d4d60aef967:87e52093dded044f',
    ('row_scales', 768): 'fe72038cf9722578:0eeedacf8704491e',
    ('huge_rows', 8): 'b0fa2ec1a540af08:efa8050c9b4f124f',
    ('huge_rows', 32): '0cb82d8d16a0222f:e033e6b51bb1fada',
    ('huge_rows', 256): '2a8f7b38a0a9b801:87e52093dded044f',
    ('huge_rows', 768): '85a3e1179bf62aaa:0eeedacf8704491e',
    ('huge_rows_1e16', 8): '22d025cd62af34b4:efa8050c9b4f124f',
    ('huge_rows_1e16', 32): 'dd864659ba27c300:e033e6b51bb1fada',
    ('huge_rows_1e16', 256): '8134fba7fb216b99:87e52093dded044f',
    ('huge_rows_1e16', 768): 'e0c45b32f0c9d1a4:0eeedacf8704491e',
    ('huge_rows_3e19', 8): '75793b3fb9d6e25a:efa8050c9b4f124f',
    ('huge_rows_3e19', 32): 'baf5e1d68c2d5917:e033e6b51bb1fada',
    ('huge_rows_3e19', 256): '39ed3e213b52f616:87e52093dded044f',
    ('huge_rows_3e19', 768): '9b19a2144343def0:0eeedacf8704491e',
    ('tiny_rows', 8): '8cb823801c258992:efa8050c9b4f124f',
    ('tiny_rows', 32): 'ec616656e2e06785:e033e6b51bb1fada',
    ('tiny_rows', 256): 'f86b3524d08e06c5:87e52093dded044f',
    ('tiny_rows', 768): 'b778c4e31971b925:0eeedacf8704491e',
    ('tiny_rows_all', 8): '4b505506de85ff2c:efa8050c9b4f124f',
    ('tiny_rows_all', 32): 'dde7f23c863c1d10:e033e6b51bb1fada',
    ('tiny_rows_all', 256): '5b2642acc5e57349:87e52093dded044f',
    ('tiny_rows_all', 768): '68e7ad56edb9d390:0eeedacf8704491e',
    ('codebook_scale_m120', 8): '52d5a9e4cf621650:2ae47199a5122980',
    ('codebook_scale_m120', 32): 'b0d5377f774dcadc:0606043ebf29f857',
    ('codebook_scale_m120', 256): '97c0042b67806029:56e1394e04e5dc27',
    ('codebook_scale_m120', 768): 'b51e34240e8632fa:6f2f9583e4a8aa40',
    ('codebook_scale_m90', 8): '4ee16a3d9e88f340:4cd9ed9eaee5b232',
    ('codebook_scale_m90', 32): 'ad899ec65a1d04e4:a230af85d4cc1634',
    ('codebook_scale_m90', 256): 'd4c878060c5cb217:1a23f76751d8e217',
    ('codebook_scale_m90', 768): '36715b5a70975a18:4e263ee6ea507d87',
    ('codebook_scale_p90', 8): '9d7abbdf35998cf2:4ccce2327ace97a7',
    ('codebook_scale_p90', 32): '23e1bf144b748e91:0f1ff8ef6eb7a52a',
    ('codebook_scale_p90', 256): 'af916f26d8794e5f:236331756e40f926',
    ('codebook_scale_p90', 768): 'ae2dcf7cb9d73bfc:a93625cf29c0d344',
    ('codebook_scale_p110', 8): '1df9290975fe85a0:f1dba7b2a837dd00',
    ('codebook_scale_p110', 32): '3b1e401cd9495170:4a744fb8792b7b3c',
    ('codebook_scale_p110', 256): '1441c8fc620bf507:ce4d31d26c73c62d',
    ('codebook_scale_p110', 768): '161b1bcf2f708ed6:f02f0fc31f41bf23',
    ('codebook_scale_subnormal', 8): '719ae50d207c6e9b:c268d306229c81fe',
    ('codebook_scale_subnormal', 32): '72b0b96040dbc2db:5b6646efd87466e9',
    ('codebook_scale_subnormal', 256): '627cfa4c833cd166:aa0579317e6e0fd3',
    ('codebook_scale_subnormal', 768): '1dd19ef4b9003fc5:61d26905c764bc12',
    ('codebook_scale_p55_w', 8): '719ae50d207c6e9b:0b52cfe0b22fbc30',
    ('codebook_scale_p55_w', 32): '72b0b96040dbc2db:c0450b5253ea017f',
    ('codebook_scale_p55_w', 256): '627cfa4c833cd166:d8c7891b4f89d334',
    ('codebook_scale_p55_w', 768): '1dd19ef4b9003fc5:d3a47376555db926',
    ('ulp_pairs', 8): '78e33ca35996d268:b9bc4fbd94771237',
    ('ulp_pairs', 32): 'ea20e9c4dbbe2296:d0cd88bbb5dffd3c',
    ('ulp_pairs', 256): '13dd5550c9847dcc:fdac3e8b965bfb39',
    ('ulp_pairs', 768): '1e35cca38ce3f33e:17b4f70f157a4c45',
    ('mixed', 8): 'd7337553c53dcc3a:69a286502e1683ec',
    ('mixed', 32): '13328cdfa1392485:a45057f73e149bb2',
    ('mixed', 256): 'a02228d4a9ce25a0:ed4f77c26b16e620',
    ('mixed', 768): '2098b1a1df273058:a2a84fcd119649cb',
})
