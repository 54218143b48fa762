"""The dtype, layout and row-view rules the activation op families share (``ops.dense_layouts``, ``ops.row_view``) and every
family's verdict on ONE table of small tensors.  The expectations are literals: they were recorded from the helpers each family
kept for itself before these rules had one owner, so a family's verdict on a row of the table is what it always was.  Two rows
are findings of that recording - the families did not agree on them:

  * a channels-last map and a transposed map fail two clauses of the row view at once; the sampler's and the cross-entropy's
    op reported 'do not flatten' first, the cosine embedding 'stride 1'.  Both refuse; the one owner reports 'stride 1' (the
    route decisions of the sampler and the cross-entropy always did).
  * an empty tensor: the cosine embedding's helper refused it as a row view, the sampler's let R = 0 through to the library.
    The row view lets it through and ``cosine_embedding_refusal`` keeps its own 'empty tensor' clause.
"""
import pytest
import torch

from vector_quantization_amd import ops, samplers
from vector_quantization_amd.quantizers import routes

NEITHER = 'neither NCHW-contiguous nor channels-last'
FAMILIES = ('cosine', 'lpips', 'stylegan2', 'group_norm', 'image_metrics', 'sampler_why', 'token_ce_why', 'group_norm_why')


def _tensors():
    base = torch.arange(120.).reshape(2, 3, 4, 5)
    return {
        'nchw': base,
        'nhwc': base.contiguous(memory_format=torch.channels_last),
        'c1': torch.zeros(2, 1, 4, 5),                                   # C == 1: dense both ways
        'bc': torch.zeros(4, 6),
        'every_other': base[:, :, ::2],
        'transposed': base.transpose(2, 3),
        'expanded': torch.ones(()).expand(2, 3, 4, 5),                   # the gradient of .sum(): every stride 0
        'one_row': torch.zeros(8).as_strided((1, 6), (2, 1)),            # a single row whose stride is below C
        'wide_rows': torch.zeros(4, 10)[:, :6],                          # rows cut from a wider buffer
        'last_stride2': torch.zeros(4, 12)[:, ::2],
        'empty': torch.zeros(0, 3, 4, 5),
        'one_d': torch.zeros(6),
        'f64': base.double(),
    }


def _all(why):
    return dict.fromkeys(FAMILIES, why)


# name: (dense_layouts, row view: its row stride or a piece of the reason, {family: '' or a piece of the reason})
EXPECTED = {
    'nchw': (('map',), 5, _all('')),
    'nhwc': (('rows',), 'stride 1', {**_all(''), 'cosine': 'stride 1', 'sampler_why': 'stride 1', 'token_ce_why': 'stride 1'}),
    'c1': (('map', 'rows'), 5, _all('')),
    'bc': (('map',), 6, {**_all(''), 'lpips': 'one shape', 'image_metrics': 'must both be [B, C, H, W]'}),
    'every_other': ((), 10, {**_all(NEITHER), 'cosine': '', 'sampler_why': '', 'token_ce_why': ''}),
    'transposed': ((), 'stride 1', {**_all(NEITHER), 'cosine': 'stride 1', 'sampler_why': 'stride 1', 'token_ce_why': 'stride 1'}),
    'expanded': ((), 'stride 1', {**_all(NEITHER), 'cosine': 'stride 1', 'sampler_why': 'stride 1', 'token_ce_why': 'stride 1'}),
    'one_row': (('map',), 6, {**_all(''), 'lpips': 'one shape', 'image_metrics': 'must both be [B, C, H, W]'}),
    'wide_rows': ((), 10, {**_all(''), 'lpips': 'one shape', 'stylegan2': NEITHER, 'group_norm': NEITHER,
                           'image_metrics': 'must both be [B, C, H, W]', 'group_norm_why': NEITHER}),
    'last_stride2': ((), 'stride 1', {**_all('stride 1'), 'lpips': 'one shape', 'stylegan2': NEITHER, 'group_norm': NEITHER,
                                      'image_metrics': 'must both be [B, C, H, W]', 'group_norm_why': NEITHER}),
    'empty': (('map',), 5, {'cosine': 'empty tensor', 'lpips': 'empty features', 'stylegan2': 'empty activation',
                            'group_norm': 'empty activation', 'image_metrics': 'empty images', 'sampler_why': '',
                            'token_ce_why': '0 rows', 'group_norm_why': ''}),
    'one_d': (('map',), 6, {**_all(''), 'lpips': 'one shape', 'stylegan2': '1-D', 'group_norm': '1-D',
                            'image_metrics': 'must both be [B, C, H, W]'}),
    'f64': (('map',), 'float64', _all('float64')),
}


class Fake:
    """A CPU tensor as a route decision sees a device tensor (no GPU here): the decision goes on past its device clause."""
    def __init__(self, t):
        self.t, self.is_cuda = t, True

    def __getattr__(self, n):
        return getattr(self.t, n)


def _verdicts(t):
    targets = torch.zeros(t.shape[:-1], dtype=torch.int64)
    return {
        'cosine': ops.cosine_embedding_refusal(t, t),
        'lpips': ops.lpips_refusal(t, t),
        'stylegan2': ops.stylegan2_refusal(t),
        'group_norm': ops.group_norm_refusal(t, 1),
        'image_metrics': ops.image_metrics_refusal(t, t, False),
        'sampler_why': routes.sampler_why(samplers.BaseSampler(), Fake(t)).why,
        'token_ce_why': routes.token_ce_why(Fake(t), targets).why,
        'group_norm_why': routes.group_norm_why(None, Fake(t)).why,
    }


def test_the_table_is_the_one_the_expectations_were_recorded_on():
    assert set(_tensors()) == set(EXPECTED) and all(set(want) == set(FAMILIES) for _, _, want in EXPECTED.values())


@pytest.mark.parametrize('name', list(EXPECTED))
def test_dense_layouts(name):
    t, want = _tensors()[name], EXPECTED[name][0]
    assert ops.dense_layouts(t) == want
    assert ops.dense_layout(t) == (want[0] if want else None)
    assert ops.lpips_layout(t, t) == (want[0] if want else None)
    assert (ops.dense_refusal('x', t) == '') == bool(want) and (want or NEITHER in ops.dense_refusal('x', t))
    assert (ops.dense(t) is t) == bool(want) and ops.dense_layouts(ops.dense(t))


@pytest.mark.parametrize('name', list(EXPECTED))
def test_row_view(name):
    t, want = _tensors()[name], EXPECTED[name][1]
    got = ops.row_view(t, 'the logits')
    if isinstance(want, str):
        assert isinstance(got, str) and want in got
        with pytest.raises(ValueError, match=want):
            ops._logit_rows('op', t, 0, t.shape[-1])
        return
    rows, stride = got
    C = t.shape[-1]
    assert stride == want and stride >= C and rows.shape == (t.numel() // C, C)
    assert rows.data_ptr() == t.data_ptr() and (rows is t or rows._is_view())      # a view, never a copy
    if rows.shape[0] > 1:
        assert rows.stride() == (stride, 1) and torch.equal(rows, t.reshape(-1, C))
    assert ops._logit_rows('op', t, 0, C)[1:] == (rows.shape[0], stride)
    with pytest.raises(ValueError, match='need 0 <= start < end'):
        ops._logit_rows('op', t, 0, C + 1)


def test_overlapping_rows_are_refused_with_the_name_of_the_tensor():
    why = ops.row_view(torch.zeros(1, 6).expand(4, 6), 'the logits')
    assert 'rows of the logits overlap' in why and 'row stride 0 < 6' in why
    assert 'flatten' in ops.row_view(torch.zeros(2, 3, 6).transpose(0, 1), 'the logits')
    assert 'at least one dimension' in ops.row_view(torch.zeros(()), 'the logits')


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('name', list(EXPECTED))
def test_family_verdicts(name, family):
    got, want = _verdicts(_tensors()[name])[family], EXPECTED[name][2][family]
    assert (got == '') if want == '' else (want in got), (name, family, got)


@pytest.mark.parametrize('name', list(EXPECTED))
def test_the_route_decisions_stop_at_the_device_clause_on_cpu_tensors(name):
    t = _tensors()[name]
    targets = torch.zeros(t.shape[:-1], dtype=torch.int64)
    for why in (routes.sampler_why(samplers.BaseSampler(), t).why, routes.token_ce_why(t, targets).why, routes.group_norm_why(None, t).why):
        assert 'is on device cpu, not on a GPU' in why or 'are on device cpu, not on a GPU' in why


def test_the_dtype_sentence_and_the_tables():
    assert ops.float_dtype_refusal('pred is', torch.zeros(1, dtype=torch.float16)) == ''
    assert ops.float_dtype_refusal('pred is', torch.zeros(1, dtype=torch.int32)) == 'pred is torch.int32, not float32, bfloat16 or float16'
    assert set(ops.IMAGE_DTYPES) == set(ops.FLOAT_DTYPES) | {torch.uint8} and not hasattr(ops, 'SAMPLE_DTYPES')
    assert all(ops.IMAGE_DTYPES[d] == code for d, code in ops.FLOAT_DTYPES.items())
    # the two layout enums of include/vqhip.h number the same two arrangements in opposite orders
    L = ops._lib
    assert ops.LAYOUTS == {'rows': L.LAYOUT_ROWS, 'map': L.LAYOUT_MAP} and ops.IMAGE_LAYOUTS == {'rows': L.IMAGE_NHWC, 'map': L.IMAGE_NCHW}
    assert (L.LAYOUT_ROWS, L.LAYOUT_MAP) == (0, 1) and (L.IMAGE_NHWC, L.IMAGE_NCHW) == (1, 0)
