"""FiniteScalarQuantizer without a GPU: construction from the shipped configs, the codebook against the reference's fixture,
the refusals, and the argument checks of the four C entry points (all before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from vector_quantization_amd import _lib, build_quantizer, integration
from vector_quantization_amd.registries import VQITQuantizerRegistry

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fsq')
SHIPPED = {8000: [8, 8, 5, 5, 5], 64000: [8, 8, 8, 5, 5, 5]}                     # configs/fsq/model.py:13-16


def _fsq(levels, **kw):
    return build_quantizer(dict(type='FiniteScalarQuantizer', num_scalars_per_channel=levels, **kw))


@pytest.mark.parametrize('K', sorted(SHIPPED))
def test_shipped_configs_build(K):
    from vector_quantization_amd.quantizers import FiniteScalarQuantizer, ScalarQuantizer
    q = _fsq(SHIPPED[K])
    assert isinstance(q, FiniteScalarQuantizer) and isinstance(q, ScalarQuantizer)
    assert q.codebook_size == K and q.embedding_dim == len(SHIPPED[K])
    assert set(q.state_dict()) == {'_embeddings'}
    assert q.embeddings.shape == (K, len(SHIPPED[K])) and q.embeddings.dtype == torch.float32


@pytest.mark.parametrize('K', sorted(SHIPPED))
def test_embeddings_are_the_reference_codebook(K):
    z = np.load(os.path.join(GOLD, f'fsq_{K}.npz'))
    q = _fsq(SHIPPED[K])
    assert q.embeddings.numpy().tobytes() == z['embeddings'].tobytes()
    assert list(z['state_dict_keys']) == list(q.state_dict())
    # a state dict as the reference writes it loads
    other = _fsq(SHIPPED[K])
    other.load_state_dict({'_embeddings': torch.from_numpy(z['embeddings'])})
    assert torch.equal(other.embeddings, q.embeddings)


def test_non_persistent_converter_buffers():
    q = _fsq([8, 8, 5, 5, 5])
    conv = q._base_converter
    assert conv.cumprod.tolist() == [1, 8, 64, 320, 1600] and conv.cumprod.dtype == torch.int64
    assert conv.max_per_digit.tolist() == [8, 8, 5, 5, 5] and conv.max_per_digit.dtype == torch.int32
    assert len(conv) == 8000


@pytest.mark.parametrize('levels', [[8, 2, 5], [1, 5], [2], [4097, 4097], [3] * 17, []])
def test_unsupported_levels_are_refused(levels):
    with pytest.raises(ValueError):
        _fsq(levels)


def test_registered_and_replaced_in_the_reference_registry():
    from vector_quantization_amd.quantizers import FiniteScalarQuantizer, ScalarQuantizer
    assert VQITQuantizerRegistry.resolve('FiniteScalarQuantizer') is FiniteScalarQuantizer
    assert VQITQuantizerRegistry.resolve('ScalarQuantizer') is ScalarQuantizer
    assert {'ScalarQuantizer', 'FiniteScalarQuantizer'} <= set(integration.REPLACED['VQITQuantizerRegistry'])


def test_map_route_needs_a_device_map():
    q = _fsq([8, 8, 5, 5, 5])
    assert not q.map_fusable(torch.zeros(2, 5, 4, 4))                               # CPU tensor
    assert q._fusable()


@pytest.fixture(scope='module')
def lib():
    return _lib.lib()


def _consts(levels, C=None):
    from vector_quantization_amd import ops
    q = ops.fsq_constants([8, 8, 5, 5, 5])
    q.C = len(levels) if C is None else C
    for i, v in enumerate(levels[:16]):
        q.levels[i] = v
    return q


def test_c_entry_points_refuse_bad_arguments(lib):
    """Every check precedes the first HIP call: fake (non-null) pointers never reach a kernel."""
    fake = ctypes.c_void_p(0x1000)
    good = _consts([8, 8, 5, 5, 5])
    N = 1024

    def enc(q, x=fake, dt=0, layout=0, n=N, hw=0, quant=fake):
        return lib.vqhip_fsq_encode(ctypes.byref(q), x, dt, layout, n, hw, quant, fake, 0, None, None, None)

    def bwd(q, dt=0, layout=0, n=N, hw=0, g=fake):
        return lib.vqhip_fsq_backward(ctypes.byref(q), fake, dt, layout, n, hw, g, fake, None)

    def dec(q, qdt=2, layout=0, n=N, hw=0, quant=fake):
        return lib.vqhip_fsq_decode(ctypes.byref(q), quant, qdt, layout, n, hw, fake, None)

    cases = [
        (lambda f: f(_consts([8, 8, 5, 5, 5], C=0)), b'C = 0'),
        (lambda f: f(_consts([3] * 17, C=17)), b'C = 17'),
        (lambda f: f(_consts([8, 2, 5])), b'level 2'),
        (lambda f: f(_consts([8, 1, 5])), b'level 1'),
        (lambda f: f(_consts([4097, 4097])), b'2^24'),
        (lambda f: f(good, layout=7), b'layout'),
        (lambda f: f(good, n=-1), b'N'),
        (lambda f: f(good, layout=1, hw=0), b'HW'),
        (lambda f: f(good, layout=1, n=1000, hw=3), b'HW'),
    ]
    for name, fn in (('vqhip_fsq_encode', enc), ('vqhip_fsq_backward', bwd), ('vqhip_fsq_decode', dec)):
        for call, what in cases:
            assert call(fn) == -22, (name, what)
            err = lib.vqhip_last_error()
            assert name.encode() in err and what in err, (name, err)
    assert enc(good, quant=None) == -22 and b'vqhip_fsq_encode' in lib.vqhip_last_error()
    assert enc(good, x=None) == -22
    assert enc(good, dt=9) == -22 and b'x_dtype' in lib.vqhip_last_error()
    assert bwd(good, dt=9) == -22 and b'vqhip_fsq_backward: x_dtype' in lib.vqhip_last_error()
    assert bwd(good, g=None) == -22 and b'vqhip_fsq_backward' in lib.vqhip_last_error()
    assert dec(good, qdt=0) == -22 and b'vqhip_fsq_decode: quant_dtype' in lib.vqhip_last_error()
    assert dec(good, quant=None) == -22 and b'vqhip_fsq_decode' in lib.vqhip_last_error()
    assert lib.vqhip_fsq_encode(None, fake, 0, 0, N, 0, fake, None, 0, None, None, None) == -22
    bad_size = _consts([8, 8, 5, 5, 5])
    bad_size.struct_bytes = 8
    assert enc(bad_size) == -22 and b'struct_bytes' in lib.vqhip_last_error()
    # x_rows is a by-product of the map layout only
    assert lib.vqhip_fsq_encode(ctypes.byref(good), fake, 0, 0, N, 0, fake, None, 0, fake, None, None) == -22
    # int32 histogram
    assert lib.vqhip_hist_i32(None, N, 10, fake, None) == -22 and b'vqhip_hist_i32' in lib.vqhip_last_error()
    assert lib.vqhip_hist_i32(fake, N, 0, fake, None) == -22 and b'vqhip_hist_i32' in lib.vqhip_last_error()
    assert lib.vqhip_hist_i32(fake, -1, 10, fake, None) == -22
    # zero tokens: valid, nothing launched
    assert enc(good, n=0) == 0 and dec(good, n=0) == 0 and bwd(good, n=0) == 0
