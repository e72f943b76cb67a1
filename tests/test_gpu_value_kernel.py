"""k_value_map driven at the C ABI (zhip_value_map) against the independent
reference of value_cases.py, over the cases test_value_codecs.py proves against
the CPU hook: whole buffers compared, b between sentinel bytes, the error word
and the per-item non-empty words."""

import pytest

import value_driver as D

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", D.value_case_names())
def test_values_match_the_reference(name, device):
    desc, items, a, want, err, ne = D.value_case(name)
    got, gerr, gne = D.run_device(desc, items, a, len(want), device)
    assert gerr == err, name
    assert got == want, name
    if desc["encode"]:
        assert gne == ne, name


@pytest.mark.parametrize("dn,sn", D.shape_case_ids())
def test_item_shapes_match_the_reference(dn, sn, device):
    desc, items, status, a, want, err, ne = D.shape_case(dn, sn)
    got, gerr, gne = D.run_device(desc, items, a, len(want), device, status)
    assert gerr == err
    assert got == want
    if desc["encode"]:
        assert gne == ne
