"""GPU tests of the Heaviside projection (csrc/project.hip; DeviceProjection, ProjectedFilterModel, BetaContinuation) against
the extended-precision restatement of tests/projection_ref.py.

Bounds (eps = 2^-52; none of them is fitted to the kernels; tests/projection_ref.py derives the per-entry ones from the
operation count: three tanh within 2.45 eps each, argument rounding included -- z sech^2 z <= 0.448 --, the sum, the quotient
by D >= tanh(beta / 2)):

  rho      |rho_i - H^(xt_i)| <= bound_H = 1.05 eps (11.8 / D + 0.5) on active cells; passive entries exact; beta = 0 exact
  H_x      |(J^T a)_i - a_i H^_x,i| <= |a_i| bound_Hx + eps |a_i H^_x,i| (the product's rounding), zero rows exact
  eta      |eta - eta^| <= 2^-52 + E_g / |S^_v|, E_g = g_error: the rounding of the two sums of depth fold_depth (the thread's
           stride loop, 6 shuffle levels, 3 waves, then the fold's loop, 6 levels, 3 waves) plus twice sum v bound_H -- the
           bisection decides on entries that carry bound_H, and the density written at the root carries it again
  volume   |sum v rho - sum v xt| <= E_g + 2^-52 |S^_v|, both sums taken in extended precision from the device's arrays
  products volume mode, against the restatement AT THE DEVICE'S eta: volume_product_bounds, the entry bounds carried to first
           order through S_a (or the tangent's sum), S_v, their quotient and the final expression; the test asserts that the
           bound on S_v is below a hundredth of |S_v|, so first order is enough
  adjoint  |<J^T a, d> - <a, J d>| <= sum |d_j| r_j + sum |a_i| t_i with r, t the two products' entry bounds
  fused    xt of femo_filter_project equals femo_filter_apply's bit for bit; rho and eta equal femo_project_forward's on that xt
           bit for bit (ASSERTED AS EQUALITY: both kernels call the one __device__ function p_rho with the same coefficients
           and sum v xt in the same order)

Model level and design loop: the 24 x 12 cantilever of tests/test_gpu_mma.py, built locally with ProjectedFilterModel.  The
loop's bounds on x and J are ten times what a relative 1e-8 in the gradients moves the restatement's own 32 steps (measured
on the CPU: x 2.8e-8, J 3.6e-9), never looser than 1e-4 / 1e-5; the bound on M_nd is the one the bound
on x implies: |dM| <= 4 max|d rho| <= 4 (beta / D) max|dx| (W's rows sum to one, |1 - 2 rho| <= 1)."""
import functools

import numpy as np
import pytest

import projection_ref as P

pytestmark = pytest.mark.gpu

EPS = P.EPS
LD = np.longdouble
SIZES = (1, 63, 64, 65, 255, 256, 257, 1025, 100003)
BETAS = (0.0, 1.0, 8.0, 64.0, 512.0)
ETAS = (0.0, 0.3, 0.5, 1.0)


@pytest.fixture
def gpu(ctx):
    from femo_amd.fea import utils_hip
    utils_hip.set_context(ctx)
    return ctx


def _vec(ctx, a):
    from femo_amd.engine import Vec
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    return Vec(ctx, a.size).set(a)


def _passive(n, on):
    """Solid and void sets straddling the wave (64) and block (256) edges, cut to 0..n-1."""
    if not on:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    solid = np.array([i for i in (0, 254, 255, 256, 257, 1024) if i < n], dtype=np.int64)
    void = np.array([i for i in (62, 63, 64, 65, 510, 511, 512, 513, n - 1) if 0 < i < n and i not in solid], dtype=np.int64)
    return solid, np.unique(void)


# ---- element-wise stage --------------------------------------------------------------------------------------------------
def _xt_elementwise(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.random(n)
    x[::7] = 0.0
    x[3::7] = 1.0
    if n > 5:
        x[5] = 0.3                                              # an entry on the threshold eta = 0.3
    return x, rng


def check_forward(xt, rho, beta, eta, flag, void_value):
    """Assertions on one projected field; returns the worst error / bound."""
    act = flag == 0
    assert np.all(rho[flag > 0] == 1.0) and np.all(rho[flag < 0] == void_value)
    if beta == 0.0:
        assert np.array_equal(rho[act], xt[act])
        return 0.0
    err = np.abs(rho.astype(LD) - P.H(xt, beta, eta, LD))[act]
    b = P.bound_H(beta, eta)
    assert np.all(err <= b), (beta, eta, float(err.max()) / EPS, b / EPS)
    return float(err.max() / b) if err.size else 0.0


def check_diagonal_product(a, out, beta, eta, flag, hx, bhx):
    """hx, bhx: H_x in extended precision and its entry bound at (beta, eta), computed once per setting."""
    act = flag == 0
    assert np.all(out[~act] == 0.0)
    if beta == 0.0:
        assert np.array_equal(out[act], a[act])
        return 0.0
    err = np.abs(out.astype(LD) - a * hx)[act]
    b = (np.abs(a) * bhx + EPS * np.abs(a * np.asarray(hx, dtype=float)))[act]
    assert np.all(err <= b), (beta, eta, float((err / np.maximum(b, 1e-300)).max()))
    assert np.all(out[act][a[act] == 0.0] == 0.0)
    nz = b > 0
    return float((err[nz] / b[nz]).max()) if nz.any() else 0.0


@pytest.mark.parametrize("passive", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_elementwise_stage(gpu, n, passive):
    """rho, and H_x through the reverse product with unit patterns (every third entry one, the rest zero; all ones) and a
    random a, for every beta and eta of the grid on one handle (femo_project_set between them); the tangent product of the
    fixed mode is the same diagonal and must give the same bits; a second forward call gives the same bits."""
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceProjection
    xt, rng = _xt_elementwise(n, 13 * n + passive)
    solid, void = _passive(n, passive)
    flag = P.flags(n, solid, void)
    proj = DeviceProjection(gpu, n, 0.0, 0.5, None, solid, void, 1e-4)
    d_xt, d_rho, d_out = _vec(gpu, xt), Vec(gpu, n), Vec(gpu, n)
    third = np.where(np.arange(n) % 3 == 0, 1.0, 0.0)
    pats = [(third, _vec(gpu, third)), (np.ones(n), _vec(gpu, np.ones(n)))]
    a = rng.standard_normal(n) * rng.choice([1e-3, 1.0, 1e3], n)
    pats.append((a, _vec(gpu, a)))
    worst = [0.0, 0.0]
    for beta in BETAS:
        for eta in ETAS:
            proj.set(beta, eta)
            info = proj.forward(d_xt, d_rho)
            rho = np.array(d_rho.get())
            worst[0] = max(worst[0], check_forward(xt, rho, beta, eta, flag, 1e-4))
            assert info["eta"] == eta and info["flat"] == 0 and info["launches"] == 2
            act = flag == 0
            vin, vout = float(xt[act].sum()), float(rho[act].sum())
            tol = 0.5 * EPS * (P.fold_depth(n) + 1) * max(vin, vout, 1.0)
            assert abs(info["vol_in"] - vin) <= tol + 1e-15 * vin and abs(info["vol_out"] - vout) <= tol + 1e-15 * vout
            hx, bhx = P.H_x(xt, beta, eta, LD), P.bound_Hx(xt, beta, eta)
            for host, dev in pats:
                out = np.array(proj.reverse(d_xt, dev, d_out).get())
                worst[1] = max(worst[1], check_diagonal_product(host, out, beta, eta, flag, hx, bhx))
                assert np.array_equal(np.array(proj.tangent(d_xt, dev, d_out).get()), out)
            proj.forward(d_xt, d_out, info=False)
            assert np.array_equal(np.array(d_out.get()), rho)
    print(f"n={n} passive={passive}: worst error / bound: rho {worst[0]:.3f}, H_x {worst[1]:.3f}")


def test_in_place_product_and_grayness(gpu):
    """out may be a itself; M_nd against the restatement to the sums' rounding."""
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceProjection
    n = 1025
    rng = np.random.default_rng(4)
    xt, v, a = rng.random(n), rng.uniform(0.5, 1.5, n), rng.standard_normal(n)
    proj = DeviceProjection(gpu, n, 8.0, 0.4, v, [256], [255])
    d_xt, d_a, d_out, d_rho = _vec(gpu, xt), _vec(gpu, a), Vec(gpu, n), Vec(gpu, n)
    ref = np.array(proj.reverse(d_xt, d_a, d_out).get())
    assert np.array_equal(np.array(proj.reverse(d_xt, d_a, d_a).get()), ref)
    proj.forward(d_xt, d_rho)
    rho = np.array(d_rho.get())
    m, mref = proj.grayness(d_rho), float(P.grayness(rho, v, LD))
    assert abs(m - mref) <= EPS * (P.fold_depth(n) + 4) * 4.0            # 4 sum v rho (1 - rho) / sum v <= 1, summands positive
    assert 0.0 < m < 1.0


# ---- refusals through the library's error path -------------------------------------------------------------------------------
def test_library_refusals(gpu):
    import ctypes as C
    from femo_amd import _lib
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceFilter, DeviceProjection
    n = 70
    lib = gpu.lib

    def create(v=None, solid=(), void=(), void_value=1e-4, beta=1.0, eta=0.5, mode=0):
        s, w = np.asarray(solid, dtype=np.int64), np.asarray(void, dtype=np.int64)
        h = _lib.H()
        rc = lib.femo_project_create(gpu.handle, n, None if v is None else v.ctypes.data, s.size, s.ctypes.data if s.size else None,
                                     w.size, w.ctypes.data if w.size else None, void_value, beta, eta, mode, C.byref(h))
        if rc == 0:
            lib.femo_project_destroy(h)
        return rc
    assert create() == 0
    bad_v = [np.where(np.arange(n) == 64, q, 1.0) for q in (0.0, -1.0, np.nan, np.inf)]
    for kw in ([dict(beta=-1.0), dict(beta=np.nan), dict(beta=np.inf), dict(eta=-0.1), dict(eta=1.5), dict(eta=np.nan), dict(mode=2),
                dict(mode=-1), dict(solid=[n]), dict(void=[-1]), dict(solid=[3, 65], void=[65]), dict(void_value=0.0),
                dict(void_value=1.5), dict(void_value=np.nan), dict(mode=1, solid=np.arange(40), void=np.arange(40, n))]
               + [dict(v=q) for q in bad_v]):
        assert create(**kw) == 2, kw
    proj = DeviceProjection(gpu, n, 1.0, 0.5)
    for kw in (dict(beta=-1.0), dict(eta=2.0), dict(beta=np.nan)):
        with pytest.raises(ValueError):
            proj.set(**kw)
    assert proj.beta == 1.0 and proj.eta == 0.5
    x, y, z, short = Vec(gpu, n).fill(0.5), Vec(gpu, n), Vec(gpu, n), Vec(gpu, n - 1)
    alias = Vec(gpu, n - 8, device_ptr=x.device_ptr + 64)                        # overlaps x without being it
    filt = DeviceFilter(gpu, np.random.default_rng(0).random((n, 2)), 0.3)
    for args in ((x, x), (x, short), (short, y), (x, alias)):
        with pytest.raises(ValueError):
            proj.forward(*args)
    for args in ((x, x, y), (x, y, y), (x, y, x), (x, y, short), (x, alias, y)):
        with pytest.raises(ValueError):
            proj.filter_forward(filt, *args)
    for fn in (proj.reverse, proj.tangent):
        for args in ((x, y, x), (x, y, short), (x, y, alias)):
            with pytest.raises(ValueError):
                fn(*args)
    with pytest.raises(ValueError):
        proj.grayness(short)
    with pytest.raises(ValueError):
        DeviceProjection(gpu, n, 1.0, "volume", solid=np.arange(n))
    proj.set(eta="volume")
    with pytest.raises(ValueError):
        proj.reverse(x, y, z)                                                    # no forward call yet: no threshold
    info = proj.forward(x, y)                                                    # the refused calls left no trace
    # a constant field keeps its volume only as itself: eta = 1/2 to the bisection's resolution, rho = 1/2 to the entry bound
    assert info["mode"] == 1 and np.abs(np.array(y.get()) - 0.5).max() <= P.bound_H(1.0, 0.5) + EPS


# ---- fused path ------------------------------------------------------------------------------------------------------------------
def _cloud(name):
    rng = np.random.default_rng(11)
    if name == "cells2d":
        return rng.random((2000, 2)), 0.02
    gx, gy = np.meshgrid(np.arange(12) * 0.1, np.arange(9) * 0.1, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], axis=1), 0.2


@pytest.mark.parametrize("name", ["cells2d", "lattice"])
def test_fused_filter_projection(gpu, name):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceFilter, DeviceProjection
    c, r = _cloud(name)
    n = c.shape[0]
    rng = np.random.default_rng(3)
    x, v = rng.random(n), rng.uniform(0.5, 1.5, n)
    solid, void = _passive(n, True)
    flag = P.flags(n, solid, void)
    filt = DeviceFilter(gpu, c, r)
    proj = DeviceProjection(gpu, n, 0.0, 0.5, v, solid, void, 1e-4)
    d_x, d_xt0, d_xt1, d_rho1, d_rho2 = _vec(gpu, x), Vec(gpu, n), Vec(gpu, n), Vec(gpu, n), Vec(gpu, n)
    xt0 = np.array(filt.apply(d_x, d_xt0).get())
    for beta, eta in ((0.0, 0.5), (4.0, 0.5), (64.0, 0.3), (8.0, "volume"), (512.0, "volume")):
        proj.set(beta, eta)
        d_xt1.fill(-1.0)
        i1 = proj.filter_forward(filt, d_x, d_xt1, d_rho1)
        assert np.array_equal(np.array(d_xt1.get()), xt0)
        i2 = proj.forward(d_xt0, d_rho2)
        rho1, rho2 = np.array(d_rho1.get()), np.array(d_rho2.get())
        assert i1["eta"] == i2["eta"] and i1["vol_in"] == i2["vol_in"] and i1["vol_out"] == i2["vol_out"] and i1["flat"] == i2["flat"]
        assert np.array_equal(rho1, rho2)
        if eta == "volume":
            assert i1["launches"] == 1 + 107 + 1 + 1 and i2["launches"] == i1["launches"]
        else:
            assert i1["launches"] == 2 and i2["launches"] == 2               # the gather (or the element-wise launch), the fold
            check_forward(xt0, rho1, beta, eta, flag, 1e-4)
    proj.set(4.0, 0.5)
    proj.filter_forward(filt, d_x, d_xt1, d_rho1, info=False)               # one launch, nothing copied back
    assert np.array_equal(np.array(d_xt1.get()), xt0)


# ---- volume mode -----------------------------------------------------------------------------------------------------------------
def _volume_case(n):
    rng = np.random.default_rng(17 * n)
    return rng.uniform(0.02, 0.92, n), rng.uniform(0.5, 1.5, n), rng.standard_normal(n), rng.standard_normal(n)


@functools.lru_cache(maxsize=None)
def _eta_reference(n, beta, passive):
    xt, v, _, _ = _volume_case(n)
    flag = P.flags(n, *_passive(n, passive))
    return P.bisect_eta(xt, v, beta, flag, LD)


def check_volume(xt, v, a, d, flag, beta, eta_ref, eta, rho, rev, tan, info):
    """Every assertion on one volume-mode case; the device enters only through its arrays and its record."""
    act = flag == 0
    Sv = abs(float((v * P.H_eta(xt, beta, eta_ref, LD))[act].sum()))
    Eg = P.g_error(xt, v, beta, eta_ref, flag)
    assert 0.0 <= eta <= 1.0 and abs(eta - eta_ref) <= EPS + Eg / Sv, (eta, eta_ref, Eg / Sv)
    assert np.all(rho[flag > 0] == 1.0) and np.all(rho[flag < 0] == 1e-4)
    dv = abs(float((v.astype(LD) * rho.astype(LD))[act].sum() - (v.astype(LD) * xt.astype(LD))[act].sum()))
    assert dv <= Eg + EPS * Sv, (dv, Eg, Sv)
    vin = float((v * xt)[act].sum())
    assert abs(info["vol_in"] - vin) <= 1e-13 * vin and abs(info["vol_out"] - vin) <= 1e-13 * vin + Eg + EPS * Sv
    assert info["flat"] == 0 and abs(info["s_v"]) > 0.0
    # the density is H at the device's own eta
    err = np.abs(rho.astype(LD) - P.H(xt, beta, eta, LD))[act]
    assert np.all(err <= P.bound_H(beta, eta))
    out = {}
    for name, dev, vec, fn in (("reverse", rev, a, P.jac_reverse), ("tangent", tan, d, P.jac_forward)):
        ref, _, _ = fn(xt, vec, beta, eta, flag, v, True, LD)
        bound, dSv, aSv = P.volume_product_bounds(xt, vec, beta, eta, flag, v, name == "tangent")
        assert dSv <= 0.01 * aSv, (name, dSv, aSv)
        e = np.abs(dev.astype(LD) - ref)
        assert np.all(dev[~act] == 0.0) and np.all(e <= bound), (name, float((e[act] / bound[act]).max()))
        out[name] = bound
    lhs, rhs = float((rev.astype(LD) * d).sum()), float((a * tan.astype(LD)).sum())
    assert abs(lhs - rhs) <= float((np.abs(d) * out["reverse"]).sum() + (np.abs(a) * out["tangent"]).sum()), (lhs, rhs)
    return abs(eta - eta_ref) / (EPS + Eg / Sv)


@pytest.mark.parametrize("passive", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_volume_mode(gpu, n, passive):
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceProjection
    xt, v, a, d = _volume_case(n)
    solid, void = _passive(n, passive)
    flag = P.flags(n, solid, void)
    if not (flag == 0).any():
        with pytest.raises(ValueError):
            DeviceProjection(gpu, n, 1.0, "volume", v, solid, void)
        return
    proj = DeviceProjection(gpu, n, 1.0, "volume", v, solid, void, 1e-4)
    d_xt, d_a, d_d, d_rho, d_rev, d_tan = _vec(gpu, xt), _vec(gpu, a), _vec(gpu, d), Vec(gpu, n), Vec(gpu, n), Vec(gpu, n)
    worst = 0.0
    for beta in BETAS[1:]:
        proj.set(beta=beta)
        info = proj.forward(d_xt, d_rho)
        rho = np.array(d_rho.get())
        rev, tan = np.array(proj.reverse(d_xt, d_a, d_rev).get()), np.array(proj.tangent(d_xt, d_d, d_tan).get())
        worst = max(worst, check_volume(xt, v, a, d, flag, beta, _eta_reference(n, beta, passive), info["eta"], rho, rev, tan, info))
        again = proj.forward(d_xt, d_rev)
        assert again["eta"] == info["eta"] and again["vol_out"] == info["vol_out"] and np.array_equal(np.array(d_rev.get()), rho)
        assert info["launches"] == 1 + 107 + 1 + 1                     # sum v xt; the target's fold and 53 x 2; rho; the last fold
    print(f"n={n} passive={passive}: worst |eta - eta_ref| / bound {worst:.3f}")


def test_volume_mode_flat(gpu):
    """Every active cell saturated (xt in {0, 1}, beta = 512): H_eta = 0 exactly in every cell, so S_v = 0, flat = 1, the
    rank-one term is dropped and both products are the finite diagonal ones.  (g = 0 at every eta here, so the bisection ends
    at its left end, eta = 2^-54: the cells with xt = 0 then sit on the threshold and have H_x = beta / D.)"""
    from femo_amd.engine import Vec
    from femo_amd.fea.elasticity import DeviceProjection
    n = 1025
    rng = np.random.default_rng(2)
    xt = (rng.random(n) < 0.4).astype(float)
    proj = DeviceProjection(gpu, n, 512.0, "volume", rng.uniform(0.5, 1.5, n))
    a = rng.standard_normal(n)
    d_xt, d_a, d_rho, d_out = _vec(gpu, xt), _vec(gpu, a), Vec(gpu, n), Vec(gpu, n)
    info = proj.forward(d_xt, d_rho)
    assert info["flat"] == 1 and info["s_v"] == 0.0 and 0.0 <= info["eta"] <= 1.0
    assert np.array_equal(np.array(d_rho.get()), xt)
    eta = info["eta"]
    hx, bhx = P.H_x(xt, 512.0, eta, LD), P.bound_Hx(xt, 512.0, eta)
    for fn in (proj.reverse, proj.tangent):
        out = np.array(fn(d_xt, d_a, d_out).get())
        assert np.all(np.isfinite(out))
        check_diagonal_product(a, out, 512.0, eta, np.zeros(n, np.int8), hx, bhx)
    proj.set(beta=0.0)                                                          # the identity is flat too: g = 0 everywhere
    info = proj.forward(d_xt, d_rho)
    assert info["flat"] == 1 and np.array_equal(np.array(d_rho.get()), xt)
    assert np.array_equal(np.array(proj.reverse(d_xt, d_a, d_out).get()), np.array(d_a.get()))


# ---- model level --------------------------------------------------------------------------------------------------------------------
NELX, NELY, L_X, L_Y = 24, 12, 160.0, 80.0


def build_projected_cantilever(device=False, projected=True, seed=0, **projection):
    """tests/test_gpu_topopt.build_cantilever at 24 x 12 with ProjectedFilterModel (projected=False: GeneralFilterModel)."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel, ProjectedFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.elasticity import averageFunc, compliance, pdeRes
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, Measure, TestFunction, VectorFunctionSpace,
                                      createRectangleMesh, locate_dofs_geometrical, locate_entities_boundary, meshSize,
                                      meshtags)
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([L_X, L_Y]), NELX, NELY)
    traction_facets = locate_entities_boundary(
        mesh, 1, lambda x: np.logical_and(abs(x[1] - L_Y / 2) < L_Y / NELY + 3e-6, abs(x[0] - L_X) < 3e-6))
    facet_tag = meshtags(mesh, 1, traction_facets, np.full(len(traction_facets), 100, dtype=np.int32))
    ds_ = Measure('ds', domain=mesh, subdomain_data=facet_tag, metadata={"quadrature_degree": 4})
    fea = FEA(mesh)
    fea.REPORT = False
    Q, V = FunctionSpace(mesh, ('DG', 0)), VectorFunctionSpace(mesh, ('CG', 1))
    rho_fn, u_fn = Function(Q), Function(V)
    f = Constant(mesh, (0, -1 / 4))
    res = pdeRes(u_fn, TestFunction(V), rho_fn, f, dss=ds_(100), method="SIMP")
    fea.add_input('density', rho_fn)
    fea.add_state(name='displacements', function=u_fn, residual_form=res, arguments=['density'])
    fea.add_output(name='avg_density', type='scalar', form=averageFunc(rho_fn), arguments=['density'])
    fea.add_output(name='compliance', type='scalar', form=compliance(u_fn, f, dss=ds_(100)), arguments=['displacements'])
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0., atol=1e-6))], V)
    fea_model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    h_avg = (h.max() + h.min()) / 2
    nel = mesh.n_cell
    if projected:
        filt = ProjectedFilterModel(nel=nel, coordinates=Q.tabulate_dof_coordinates(), h_avg=h_avg, **projection)
    else:
        filt = GeneralFilterModel(nel=nel, coordinates=Q.tabulate_dof_coordinates(), h_avg=h_avg)
    fea_model.add(filt, name='general_filter_model')
    fea_model.create_input('density_unfiltered', shape=nel, val=np.random.default_rng(seed).random(nel) * 0.86)
    fea_model.add_design_variable('density_unfiltered', upper=1.0, lower=1e-4)
    fea_model.add_objective('compliance')
    fea_model.add_constraint('avg_density', upper=0.40)
    sim = Simulator(fea_model, device=device)
    return sim, filt, mesh, dict(facets=traction_facets, h_avg=h_avg)


def _cell_sets(mesh):
    """A solid strip along the loaded edge (x >= 150) and a void block in the interior."""
    c = mesh.centroids()
    solid = np.nonzero(c[:, 0] >= 150.0)[0]
    void = np.nonzero((np.abs(c[:, 0] - 60.0) <= 12.0) & (np.abs(c[:, 1] - 40.0) <= 12.0))[0]
    assert solid.size and void.size and not np.intersect1d(solid, void).size
    return solid, void


@pytest.mark.parametrize("device", [True, False])
def test_beta_zero_is_the_general_filter(gpu, device):
    sim0, _, mesh, _ = build_projected_cantilever(device, projected=False)
    sim1, filt, _, _ = build_projected_cantilever(device, projection_beta=0.0)
    sim0.run()
    sim1.run()
    assert np.array_equal(np.asarray(sim0['density']), np.asarray(sim1['density']))
    # the same density through the same solver: the totals agree to the solves' tolerance (two separately built models)
    g0 = np.asarray(sim0.compute_totals('compliance', 'density_unfiltered'))
    g1 = np.asarray(sim1.compute_totals('compliance', 'density_unfiltered'))
    assert np.abs(g0 - g1).max() <= 1e-9 * np.abs(g0).max()
    assert filt.operation.last["eta"] == 0.5 and filt.operation.last["flat"] == 0


@pytest.mark.parametrize("eta", [0.5, "volume"])
def test_totals_with_passive_cells(gpu, eta):
    """check_totals at step 1e-4 under the existing bound 1e-6, beta = 4, a solid strip and a void block."""
    import elasticity_ref as eref
    _, _, mesh, _ = build_projected_cantilever(False, projected=False)
    solid, void = _cell_sets(mesh)
    vol = eref.cell_volumes(mesh.x, mesh.conn)
    sim, filt, mesh, _ = build_projected_cantilever(False, projection_beta=4.0, eta=eta, volumes=vol, solid=solid, void=void)
    sim.run()
    rho = np.asarray(sim['density'])
    assert np.all(rho[solid] == 1.0) and np.all(rho[void] == 1e-4)
    for of in ('compliance', 'avg_density'):
        chk = sim.check_totals(of, 'density_unfiltered', step=1e-4, n_dir=3, seed=0)
        print(eta, of, chk['rel_error'])
        assert max(chk['rel_error']) <= 1e-6, chk
    op = filt.operation
    assert op.last["mode"] == (1 if eta == "volume" else 0)
    assert abs(op.grayness() - float(P.grayness(rho, vol, LD))) <= 1e-13


@pytest.mark.parametrize("device", [True, False])
def test_volume_mode_keeps_the_average_density(gpu, device):
    """eta = 'volume' without passive cells: avg_density = v . xt / sum v within the volume bound; in device mode no array of
    n entries crosses the link during run() and compute_totals()."""
    import elasticity_ref as eref
    from femo_amd import engine
    _, _, mesh, aux = build_projected_cantilever(False, projected=False)
    vol = eref.cell_volumes(mesh.x, mesh.conn)
    n = mesh.n_cell
    sim, filt, mesh, _ = build_projected_cantilever(device, projection_beta=8.0, eta="volume", volumes=vol)
    x = np.array(sim['density_unfiltered'])
    sim.run()                                                     # first run: set-up traffic
    gpu.sync()
    engine.host_stats(reset=True)
    sim.run()
    g = sim.compute_totals('compliance', 'density_unfiltered')
    ga = sim.compute_totals('avg_density', 'density_unfiltered')
    gpu.sync()
    stats = engine.host_stats()
    if device:
        moved = {k: v for k, v in stats.items() if v and not k.startswith("h2d_skipped")}
        print("host traffic:", moved)
        assert sum(v for k, v in moved.items() if k.endswith("_bytes")) < 8 * n // 2, moved
    xt = eref.filter_matrix(mesh.centroids(), 2.0 * aux["h_avg"]) @ x
    op = filt.operation
    eta = op.last["eta"]
    Sv = abs(float((vol * P.H_eta(xt, 8.0, eta, LD)).sum()))
    # xt is the host filter's here: its own rounding (a row sum of <= 30 products) enters through sum v |d xt| <= 32 eps sum v xt
    bound = (P.g_error(xt, vol, 8.0, eta) + EPS * Sv + 32 * EPS * float(vol @ xt)) / vol.sum() + 64 * EPS       # and the output's own sum
    avg = float(np.asarray(sim['avg_density'])[0])
    assert abs(avg - float(vol @ xt / vol.sum())) <= bound, (avg, float(vol @ xt / vol.sum()), bound)
    assert np.all(np.isfinite(np.asarray(g))) and np.all(np.isfinite(np.asarray(ga)))
    # the volume is preserved along every direction: d avg_density / dx = W^T v / sum v, the projection drops out
    W = eref.filter_matrix(mesh.centroids(), 2.0 * aux["h_avg"])
    assert np.abs(np.asarray(ga) - W.T @ (vol / vol.sum())).max() <= 1e-10 * np.abs(np.asarray(ga)).max()


# ---- the design loop ----------------------------------------------------------------------------------------------------------------
STEPS, STAGE_BETAS, EVERY = 32, (1.0, 2.0, 4.0, 8.0), 8
_LOOP = {}


def _loop_reference():
    """Computed once for both modes: the restated loop and how far a relative 1e-8 in the gradients moves it."""
    if not _LOOP:
        import elasticity_ref as eref
        _, _, mesh, aux = build_projected_cantilever(False, projected=False)
        clean = P.continuation_loop(mesh, aux["facets"], aux["h_avg"], STAGE_BETAS, EVERY, STEPS)
        noisy = P.continuation_loop(mesh, aux["facets"], aux["h_avg"], STAGE_BETAS, EVERY, STEPS, noise=1e-8)
        dx = max(np.abs(a[2] - b[2]).max() for a, b in zip(clean, noisy))
        dJ = max(abs(a[0] - b[0]) / abs(a[0]) for a, b in zip(clean, noisy))
        _LOOP.update(clean=clean, dx=dx, dJ=dJ, vol=eref.cell_volumes(mesh.x, mesh.conn))
    return _LOOP


@pytest.mark.parametrize("device", [True, False])
def test_design_loop_with_continuation(gpu, device):
    """betas (1, 2, 4, 8), 8 steps each, 32 steps, avg_density <= 0.40 from x = 0.4, eta = 0.5, step by step against the
    restated loop.  The Newton-step counts are printed, not asserted."""
    from femo_amd.opt import MMA, BetaContinuation, CSDLProblem
    ref = _loop_reference()
    sim, filt, mesh, _ = build_projected_cantilever(device, projection_beta=STAGE_BETAS[0], volumes=ref["vol"])
    n = mesh.n_cell
    assert n == 576
    sim['density_unfiltered'] = np.full(n, 0.4)
    prob = CSDLProblem(problem_name='beam_topo_opt', simulator=sim)
    op = filt.operation
    optimizer = MMA(prob, max_iter=STEPS, move=0.5, tol=0.0, sub_tol=1e-7, normalize=True,
                    continuation=BetaContinuation(op, STAGE_BETAS, EVERY)).setup()
    xs, run = [], sim.run
    resets, reset = [], optimizer.handle.reset

    def recording_run():
        xs.append(np.array(sim['density_unfiltered']))
        run()

    def recording_reset():
        resets.append(len(xs) + 1)                               # the step the fresh history begins with
        reset()
    sim.run = recording_run
    optimizer.handle.reset = recording_reset
    res = optimizer.solve()
    clean = ref["clean"]
    bx, bJ = min(10.0 * ref["dx"], 1e-4), min(10.0 * ref["dJ"], 1e-5)
    ex = max(np.abs(x - r[2]).max() for x, r in zip(xs, clean))
    eJ = max(abs(J - r[0]) / abs(r[0]) for J, r in zip(res["objective"], clean))
    bM = 4.0 * (STAGE_BETAS[-1] / float(P.denominator(STAGE_BETAS[-1], 0.5))) * bx + 64 * EPS
    eM = abs(res["grayness"][-1] - clean[-1][5])
    print(f"device={device}: J {res['objective'][0]:.2f} -> {res['objective'][-1]:.2f}, M_nd {res['grayness'][0]:.4f} -> "
          f"{res['grayness'][-1]:.4f}; sensitivity of the restatement to 1e-8: x {ref['dx']:.2e}, J {ref['dJ']:.2e}; against the "
          f"restatement: x {ex:.2e} (bound {bx:.2e}), J {eJ:.2e} (bound {bJ:.2e}), M_nd {eM:.2e} (bound {bM:.2e}); Newton steps "
          f"{res['inner']} (restatement {[r[3] for r in clean]})")
    assert len(res["objective"]) == STEPS == len(xs)
    assert res["beta"] == [r[4] for r in clean] == P.stage_plan(STAGE_BETAS, EVERY, STEPS)[0]
    assert res["reset"] == [1, 9, 17, 25] == resets
    assert res["eta"] == [0.5] * STEPS
    assert ex <= bx and eJ <= bJ
    assert eM <= bM
    assert all(c == 1 for c in res["converged"])
    assert res["grayness"][-1] < res["grayness"][0]
