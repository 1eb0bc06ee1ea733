"""Mirror of the reference's ``femo.fea`` package on the HIP engine.

``femo.fea.fea_dolfinx``  -> ``femo_amd.fea.fea_hip``   (class FEA)
``femo.fea.utils_dolfinx`` -> ``femo_amd.fea.utils_hip`` (assemble*, update, solve*, ...)
"""

# The damped harmonic response of the SIMP elasticity, by name from the package (resolved on first use: importing the
# package stays as light as before).
_ELASTICITY_NAMES = ("DampedHarmonicElasticityResidual", "DampedDynamicCompliance", "pdeRes_harmonic_damped",
                     "dynamic_compliance_damped")
__all__ = list(_ELASTICITY_NAMES)


def __getattr__(name):
    if name in _ELASTICITY_NAMES:
        from . import elasticity
        return getattr(elasticity, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
