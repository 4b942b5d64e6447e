"""CPU-only checks of the interface of screening under an obstacle horizon: include/omds.h declares the switch and the binding, the
engine and the facade carry it; the test hook of include/omds_test_horizon.h lives in the test library only."""
import ctypes as C
import inspect
import os
import re

import pytest

from helpers import ROOT


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"OMDS_API\s+[\w\s\*]+?\b(omds_\w+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from optimalmodulationds_amd import _lib
    return _lib.load()


def test_switch_is_declared_exported_and_bound(lib):
    from optimalmodulationds_amd import _lib
    names = {"omds_set_screening_horizon", "omds_get_screening_horizon"}
    assert names <= set(_declared("omds.h")) and names <= set(_lib.SIGNATURES)
    for nme in names:
        assert hasattr(lib, nme)
    # no context: the library refuses, it does not crash
    assert lib.omds_set_screening_horizon(None, 1) != 0 and lib.omds_get_screening_horizon(None, None, None) != 0


def test_horizon_hook_lives_in_the_test_library_only(lib):
    from optimalmodulationds_amd import _lib
    hooks = _declared("omds_test_horizon.h")
    assert hooks == sorted(_lib.HORIZON_HOOK_SIGNATURES) == ["omds_test_screen_corrupt_slab"]
    raw, raw_test = C.CDLL(_lib.LIB_PATH), C.CDLL(_lib.TEST_LIB_PATH)
    for nme in hooks:
        assert not hasattr(raw, nme), f"{nme} is a test hook and must not be exported by the product library"
        assert hasattr(raw_test, nme)
    bound = _lib.load_test_hooks()
    assert bound.omds_test_screen_corrupt_slab.argtypes == _lib.HORIZON_HOOK_SIGNATURES["omds_test_screen_corrupt_slab"][1]
    assert bound.omds_test_screen_corrupt_slab(None, 0, 0, 0.0) != 0


def test_engine_and_facade_carry_the_switch():
    from optimalmodulationds_amd import MPPI
    from optimalmodulationds_amd.engine import Engine
    assert list(inspect.signature(Engine.set_screening_horizon).parameters) == ["self", "on"]
    assert inspect.signature(Engine.set_screening_horizon).parameters["on"].default is True
    assert callable(Engine.get_screening_horizon) and callable(Engine.test_screen_corrupt_slab)
    sig = inspect.signature(MPPI.set_screening)
    assert list(sig.parameters) == ["self", "mode", "eps", "over_horizon"]
    assert sig.parameters["eps"].default == 0.0 and sig.parameters["over_horizon"].default is False


def test_header_states_the_rule():
    src = open(os.path.join(ROOT, "include", "omds.h")).read()
    assert "while a horizon is set omds_propagate runs the all-fp32 step whatever mode" not in src
    for phrase in ("omds_set_screening_horizon", "slabs 0, (H-1)/2 and H-1", "clearing the horizon does not recalibrate"):
        assert phrase in src, phrase
