"""GPU tests of the thermoelastic chain rho -> T(rho) -> u(rho, T) -> J through FEAModel + Simulator: two FEA objects in one
model, the thermal one with the state ``temperature`` (ConductionResidual), the elastic one with an input of that name that
is an argument of its state and of its output (ThermalExpansion); the reverse sweep runs two adjoint solves.  Against
tests/thermal_ref.py, reference_cycle_thermoelastic, with the bounds of test_gpu_elast_body.py::test_body_cycle.  And the
heat-sink problem of scripts/run_topopt.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import thermal_ref as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


def _maxrel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def build_cycle(device, objective, nelx=16, nely=8):
    """The 16 x 8 cantilever, filtered: uniform heating with the sink on the clamped edge, the tip traction plus the thermal
    load of the computed temperature."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, Measure, TestFunction, ThermalExpansion,
                                      VectorFunctionSpace, displacement, locate_dofs_geometrical, mean_displacement, meshtags,
                                      pdeRes_conduction)
    from femo_amd.fea.elasticity import compliance, pdeRes
    mesh, facets, h_avg, sink = tr.cycle_case(nelx, nely)
    ds = Measure('ds', domain=mesh, subdomain_data=meshtags(mesh, 1, facets, np.full(len(facets), 100, dtype=np.int32)))(100)
    Q, P, V = FunctionSpace(mesh, ('DG', 0)), FunctionSpace(mesh, ('CG', 1)), VectorFunctionSpace(mesh, ('CG', 1))
    on_clamp = lambda x: np.isclose(x[0], 0., atol=1e-6)

    thermal = FEA(mesh)
    thermal.REPORT = False
    thermal.consistent_bc_partials = True
    rho_t, T = Function(Q), Function(P)
    res_t = pdeRes_conduction(T, TestFunction(P), rho_t, source=tr.SOURCE, k0=1.0, k_min=1e-3)
    thermal.add_input('density', rho_t)
    thermal.add_state(name='temperature', function=T, residual_form=res_t, arguments=['density'])
    Tbc = Function(P)
    Tbc.vector.set(0.0)
    thermal.add_strong_bc(Tbc, [locate_dofs_geometrical((P, P), on_clamp)], P)

    elastic = FEA(mesh)
    elastic.REPORT = False
    elastic.consistent_bc_partials = True      # F(rho, T) is non-zero on the clamped vertices, and so is the multiplier
    rho_e, T_in, u = Function(Q), Function(P), Function(V)
    f = Constant(mesh, tr.TRACTION)
    th = ThermalExpansion(tr.ALPHA, T_in)
    res_e = pdeRes(u, TestFunction(V), rho_e, f, dss=ds, thermal=th)
    elastic.add_input('density', rho_e)
    elastic.add_input('temperature', T_in)
    elastic.add_state(name='displacements', function=u, residual_form=res_e, arguments=['density', 'temperature'])
    ell = None
    if objective == "compliance":
        elastic.add_output(name='objective', type='scalar', form=compliance(u, f, dss=ds, rho_e=rho_e, thermal=th),
                           arguments=['displacements', 'density', 'temperature'])
    else:
        ell = mean_displacement(V, (0.0, -1.0), ds)
        elastic.add_output(name='objective', type='scalar', form=displacement(u, ell), arguments=['displacements'])
    ubc = Function(V)
    ubc.vector.set(0.0)
    elastic.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), on_clamp)], V)

    model = FEAModel(fea=[thermal, elastic])
    model.add(GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=h_avg),
              name='general_filter_model')
    model.create_input('density_unfiltered', shape=mesh.n_cell, val=np.random.default_rng(0).random(mesh.n_cell) * 0.86)
    model.add_design_variable('density_unfiltered', upper=1.0, lower=1e-4)
    model.add_objective('objective')
    aux = dict(facets=facets, h_avg=h_avg, sink=sink, res_t=res_t, res_e=res_e, ell=ell)
    return Simulator(model, device=device), mesh, aux


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("objective", ["compliance", "displacement"])
def test_thermoelastic_cycle(gpu, objective, device):
    sim, mesh, aux = build_cycle(device, objective)
    sim.run()
    x0 = np.array(sim['density_unfiltered'])
    R = tr.reference_cycle_thermoelastic(mesh, aux['facets'], tr.TRACTION, aux['h_avg'], x0, tr.ALPHA, tr.SOURCE, aux['sink'],
                                         objective=objective, ell=aux['ell'])
    ratio = np.abs(R['u_th']).max() / np.abs(R['u_mech']).max()
    assert 0.2 <= ratio <= 5.0                                        # neither part of u hides below the tolerance
    assert np.abs(np.asarray(sim['density']) - R['rho']).max() <= 1e-14
    err_T = _maxrel(np.asarray(sim['temperature']), R['T'])
    err_u = _maxrel(np.asarray(sim['displacements']), R['u'])
    err_J = abs(float(sim['objective'][0]) - R['J']) / abs(R['J'])
    g = np.asarray(sim.compute_totals('objective', 'density_unfiltered'))
    err_g = _maxrel(g, R['grad'])
    it, ie = aux['res_t'].last_info, aux['res_e'].last_info
    print(f"thermoelastic 16x8 cantilever, J = {objective}, device={device}: |u_th|/|u_mech| {ratio:.2f}, T {err_T:.1e}, "
          f"u {err_u:.1e}, J {err_J:.1e}, total {err_g:.1e}; conduction PCG {it['state']['iterations']} + "
          f"{it['adjoint']['iterations']} it, elasticity PCG {ie['state']['iterations']} + {ie['adjoint']['iterations']} it")
    assert err_T <= 1e-9
    assert err_u <= 1e-9
    assert err_J <= 1e-9
    assert err_g <= 1e-8
    if not device:
        chk = sim.check_totals('objective', 'density_unfiltered', step=1e-4, n_dir=3, seed=0)
        print(f"central differences: {chk['rel_error']}")
        assert max(chk['rel_error']) <= 1e-6, chk


def test_heatsink_design_loop(tmp_path):
    """scripts/run_topopt.py --problem heatsink as its users start it: one JSON line, a falling thermal compliance, the
    volume bound held."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "run_topopt.py"), "--out", str(tmp_path / "density.xdmf"),
                        "--problem", "heatsink", "--nelx", "32", "--nely", "16", "--iters", "8"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["metric"] == "topopt_mma_heatsink"
    obj = out["objective"]
    print(f"heat sink 32x16: thermal compliance {obj[0]:.4f} -> {obj[-1]:.4f} in {out['steps']} steps, "
          f"avg density {out['avg_density']:.4f}, PCG {out['pcg_iterations']}")
    assert obj[1] < obj[0] and obj[-1] < obj[0]
    assert out["avg_density"] <= out["volume"] + 1e-3
