"""The table of tests/contract_cases.py against include/vqhip.h (no GPU): every entry point that takes a ``stream`` is reached by a
table entry or exempted with a reason, so a new entry point cannot skip the placement / stream / capture properties of
tests/test_gpu_op_contracts.py; and every clause an entry quotes still stands in the header."""
import re

import pytest

from vector_quantization_amd import _lib

import contract_cases as table


def stream_entry_points(text: str) -> set:
    """The names of the prototypes of a C header that have a parameter called ``stream`` (comments and macros removed as
    ``_lib.parse_header`` removes them)."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text.replace('\\\n', ' '), flags=re.S)
    text = re.sub(r'(?m)^[ \t]*#.*$', '', text)
    return {name for _, name, params in re.findall(r'([A-Za-z_][\w\s*]*?)\b(vqhip_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
            if re.search(r'\bstream\b', params)}


def uncovered(text: str, cases=None) -> set:
    cases = table.CASES if cases is None else cases
    reached = {name for case in cases for name in case.abi}
    return stream_entry_points(text) - reached - set(table.EXEMPT)


def header_text() -> str:
    with open(_lib.HEADER_PATH) as f:
        return f.read()


def header_words() -> str:
    """The header as one line of words: comment borders and line breaks do not split a quotation."""
    return ' '.join(re.sub(r'(?m)^\s*/?\*+/?', ' ', header_text()).split())


def test_every_entry_point_with_a_stream_is_in_the_table_or_exempt():
    names = stream_entry_points(header_text())
    assert len(names) > 70 and names <= set(_lib.SIGNATURES)
    assert not uncovered(header_text()), f'neither in tests/contract_cases.py nor exempt there: {sorted(uncovered(header_text()))}'


def test_the_table_and_the_exemptions_name_only_entry_points_that_exist():
    names = stream_entry_points(header_text())
    for case in table.CASES:
        assert case.abi and set(case.abi) <= names, f'{case.id}: {sorted(set(case.abi) - names)} take no stream in include/vqhip.h'
    assert set(table.EXEMPT) <= names, sorted(set(table.EXEMPT) - names)
    reached = {name for case in table.CASES for name in case.abi}
    assert not reached & set(table.EXEMPT), f'both in the table and exempt: {sorted(reached & set(table.EXEMPT))}'
    for name, reason in table.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.split()) >= 3, f'{name}: an exemption needs a reason'


def test_a_new_entry_point_cannot_skip_the_table():
    text = header_text().replace('#ifdef __cplusplus\n}', 'int vqhip_dummy_op(const void *x, int64_t n, void *stream);\n#ifdef __cplusplus\n}', 1)
    assert uncovered(text) == {'vqhip_dummy_op'}


@pytest.mark.parametrize('family', sorted({c.family for c in table.CASES}))
def test_a_family_taken_from_the_table_leaves_its_entry_points_uncovered(family):
    rest = [c for c in table.CASES if c.family != family]
    lost = {name for c in table.CASES if c.family == family for name in c.abi} - {name for c in rest for name in c.abi}
    assert lost and uncovered(header_text(), rest) == lost


def test_every_quoted_clause_stands_in_the_header():
    words = header_words()
    for case in table.CASES:
        assert case.clause and ' '.join(case.clause.split()) in words, f'{case.id}: include/vqhip.h no longer says "{case.clause}"'
    for name, clause in table.CLAUSE.items():                                  # the ones no single entry quotes (small vectors, outputs)
        assert ' '.join(clause.split()) in words, f'{name}: include/vqhip.h no longer says "{clause}"'


def test_placed_entries_are_complete():
    """Every family whose clause frees alignment has entries with the direct call, and those name what they free."""
    freed = {'sampler', 'token_ce', 'cosine', 'lpips', 'stylegan2', 'group_norm', 'vit_rows', 'image_metrics'}
    assert {c.family for c in table.PLACED} == freed
    for case in table.CASES:
        if case.family in freed:
            assert case.call_abi is not None and case.outs is not None, case.id
            assert case.free or case.id == 'lpips_keep_mask', case.id
        else:
            assert case.call_abi is None and not case.free, case.id
