"""Host side of femo_newton_rhs_linear: declared in the public header, its launcher in the internal one, bound in
`_lib.PROTOTYPES` with the handle signature of femo_newton_rhs, wrapped in `engine`, and exported by the library."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def test_symbol_is_declared_bound_and_exported():
    from femo_amd import _lib, engine
    public = re.sub(r"/\*.*?\*/", "", _read("include", "femo_hip.h"), flags=re.S)
    assert re.search(r"\bint\s+femo_newton_rhs_linear\s*\(\s*const femo_mat\*", public)
    internal = _read("femo_amd", "csrc", "femo_internal.h")
    assert re.search(r"\bint\s+femo_launch_newton_rhs_linear\s*\(", internal)
    assert _lib.PROTOTYPES["femo_newton_rhs_linear"] == _lib.PROTOTYPES["femo_newton_rhs"]
    assert hasattr(_lib.load(), "femo_newton_rhs_linear")
    assert callable(engine.newton_rhs_linear)


def test_newton_has_the_switch_and_the_linear_form_the_flag():
    from femo_amd.fea import utils_hip
    from femo_amd.fea.forms import NonlinearPoissonResidual, PoissonResidual
    assert utils_hip._NewtonBase.linear_reuse is True
    assert PoissonResidual.constant_partials is True
    assert not getattr(NonlinearPoissonResidual, "constant_partials", False)
