"""The HARP_ENG parser takes names of the engine's switch table only (no GPU: a stub object stands in for the engine)."""
from types import SimpleNamespace

import pytest

from harp_amd.engine import SWITCH_NAMES, SWITCHES, apply_env_switches


def _stub():
    return SimpleNamespace(mesh_third=False, wide_front=False, hybrid_front=False, front_auto=True, vgg_streams=2, B=3)


def test_table_names_are_unique_and_documented():
    assert len(set(SWITCH_NAMES)) == len(SWITCHES)
    assert all(sw.doc for sw in SWITCHES)


def test_parser_sets_a_switch_with_the_type_of_its_value():
    eng = _stub()
    apply_env_switches(eng, "mesh_third=1,vgg_streams=3")
    assert eng.mesh_third is True and eng.vgg_streams == 3
    apply_env_switches(eng, "")
    assert eng.front_auto is True


@pytest.mark.parametrize("text", ["B=1", "nope=1", "mesh_third=1,B=0"])
def test_parser_refuses_what_is_not_a_switch(text):
    eng = _stub()
    with pytest.raises(ValueError, match="no engine switch"):
        apply_env_switches(eng, text)
    assert eng.B == 3


@pytest.mark.parametrize("name", ["wide_front", "hybrid_front"])
def test_an_explicit_front_form_clears_front_auto(name):
    eng = _stub()
    apply_env_switches(eng, name + "=1")
    assert getattr(eng, name) is True and eng.front_auto is False
