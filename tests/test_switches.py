"""tests/util.py: switches() -- the scoped form of the NOPE_* switches the conv tests steer the planner with.  The GPU tests import the
run() functions of the *_emu_case modules in-process, so a switch that outlives a failed assertion would send every later test of the
session to other kernels than it claims to run."""
import importlib
import os

import pytest

from tests.util import switches

CASE_MODULES = ["pp_emu_case", "x2_emu_case", "up2p_emu_case", "small_emu_case", "stream_emu_case", "lean_emu_case"]


def nope_env():
    return {k: v for k, v in os.environ.items() if k.startswith("NOPE_")}


def test_switches_scope(monkeypatch):
    monkeypatch.setenv("NOPE_CONV_PP", "7")
    monkeypatch.delenv("NOPE_SMALL_TILE", raising=False)
    monkeypatch.delenv("NOPE_XCD_GN", raising=False)
    before = nope_env()
    with switches(NOPE_CONV_PP=13, NOPE_SMALL_TILE="2"):
        assert (os.environ["NOPE_CONV_PP"], os.environ["NOPE_SMALL_TILE"]) == ("13", "2")      # values through str()
        with switches(NOPE_CONV_PP=None, NOPE_XCD_GN=1):                                        # None unsets; nests
            assert "NOPE_CONV_PP" not in os.environ and os.environ["NOPE_XCD_GN"] == "1" and os.environ["NOPE_SMALL_TILE"] == "2"
        assert os.environ["NOPE_CONV_PP"] == "13" and "NOPE_XCD_GN" not in os.environ
    assert nope_env() == before and os.environ["NOPE_CONV_PP"] == "7"       # a value that was set comes back, not merely goes away
    with pytest.raises(ZeroDivisionError):
        with switches(NOPE_CONV_PP=29, NOPE_SMALL_TILE=0):
            with switches(NOPE_SMALL_TILE=None):
                1 / 0
    assert nope_env() == before


class Refused(Exception):
    pass


class RaisingHip:
    """Stands for nope_amd.hip: every attribute access fails, as a kernel fault or a failed assertion inside a case would."""
    def __getattr__(self, name):
        raise Refused(name)


@pytest.mark.parametrize("module", CASE_MODULES)
def test_case_modules_leave_no_switch_behind(module, monkeypatch):
    monkeypatch.setenv("NOPE_CONV_PP", "7")
    before = nope_env()
    run = importlib.import_module("tests." + module).run
    with pytest.raises(Refused):
        run(RaisingHip(), "cpu")
    assert nope_env() == before
