"""routes.py without a device: the configuration part of every decision reproduces the table recorded from the commit before
it (tests/golden/routes.json, variants and inputs in route_variants.py), CPU inputs are refused by naming the device, and the
reasons tell the refusals apart.

One thing the table says differently from what one might expect: 2-D rows on the CPU leave the one-call routes for
``fused_tail`` where decode + loss can be fused, not for ``hooks`` — that is what the code before routes.py decided (the library
then refuses the CPU tensor: test_host_cpu.test_no_cpu_fallback), and no decision changes here."""
import pytest

import route_variants as RV
from vector_quantization_amd.quantizers import routes

TABLE = RV.load_table()


def test_table_covers_every_variant():
    assert set(TABLE) == set(RV.VARIANTS)


@pytest.mark.parametrize('variant', RV.VARIANTS)
def test_configuration_part_and_cpu_inputs(variant):
    q = RV.build(variant)
    RV.check_config(variant, TABLE[variant], q)
    RV.check_inputs(variant, TABLE[variant], q, None)
    for x in RV.row_inputs(q, None).values():
        assert routes.step(q, x).name in ('hooks', 'fused_tail')
    for x in RV.map_inputs(q, None).values():
        assert routes.map_entry(q, x, True).name == routes.map_entry(q, x, False).name == 'tokens'


DECISIONS = {
    'step': lambda q: routes.step_config(q).why,
    'quantize': lambda q: routes.map_config(q, decode=True),
    'encode_to_quant': lambda q: routes.map_config(q, decode=False),
    'decode_from_quant': routes.decode_config,
    'update': lambda q: routes.cvq_update_config(q._callbacks.callbacks[0]).why,
}


@pytest.mark.parametrize('decision', DECISIONS)
def test_refusal_reasons_are_there_and_differ(decision):
    """Where a shipped configuration takes the fastest route of a decision and one change to it does not, the reason is not empty,
    and two different changes to the same configuration never share a reason."""
    fast = ('map', 'sparse') + RV.ONE_CALL
    seen = 0
    for base in RV.SHIPPED:
        if TABLE[base]['config'].get(decision) not in fast:
            continue
        reasons = {}
        for change, bases in RV.CHANGES.items():
            variant = f'{base}+{change}'
            if base in bases and TABLE[variant]['config'][decision] not in fast:
                reasons[change] = DECISIONS[decision](RV.build(variant))
        assert all(reasons.values()), (decision, base, reasons)
        assert len(set(reasons.values())) == len(reasons), (decision, base, reasons)
        seen += len(reasons)
    assert seen >= 2, decision
