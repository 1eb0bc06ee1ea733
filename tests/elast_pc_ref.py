"""NumPy / SciPy restatement of the multilevel preconditioner of the SIMP elasticity solves (csrc/elast_pc.hip), written
from the formulas alone:

  M^-1 = D_blk^-1 + sum_l P_l C_l P_l^T,      C_l = blockdiag_d(P_l^T A P_l)^-1

  A     K(rho) with identity rows / columns on the fixed dofs (tests/elasticity_ref.py supplies K)
  P_l   multilinear interpolation from lattice l over the bounding box to the vertices, the same scalar weights for all
        d components, zero rows on fixed dofs
  plan  coarsest lattice: spacing = the shortest extent of the bounding box (one bin along that axis), ceil(extent /
        spacing) bins along the others; every finer lattice halves the spacing; the number of lattices is
        1 + round(log2(shortest extent / (spacing_factor * mean edge length))), at least 1.  The mean edge length is the
        mean over the cells of all their d (d + 1) / 2 edges.

The Galerkin blocks are formed here by sparse products and the diagonal d x d blocks cut out of the result; the device
forms them cell by cell from the closed form (`cell_blocks` below restates that one as well, so the two derivations
check each other).  The device keeps bins as int32 and fractions as fp64, like `level_weights`.  One thing is quantised, and identically
here: a finest-lattice coordinate within SNAP of a lattice line is moved onto it (a vertex a round-off beyond a line would
otherwise reach the nodes behind it with a weight of 1e-17, and their blocks and corrections would be made of noise); the
coordinates on the coarser lattices are the finest ones divided by a power of two.
A component of a lattice node that no free dof touches has a zero Galerkin diagonal; its row and column of C are zero.
"""
from __future__ import annotations

import itertools
import math

import numpy as np
import scipy.sparse as sp

import elasticity_ref as ref

DEFAULT_SPACING_FACTOR = 2.0
MAX_LEVELS = 12
SNAP = 1e-9


def mean_edge_length(x, conn):
    p = x[conn]
    tot, cnt = 0.0, 0
    for a in range(conn.shape[1]):
        for b in range(a + 1, conn.shape[1]):
            tot += np.linalg.norm(p[:, a] - p[:, b], axis=1).sum()
            cnt += len(conn)
    return tot / cnt


def lattice_plan(x, conn, spacing_factor=0.0):
    """dict(lo, n_levels, n[l] = bins per axis (coarsest first), H[l], nodes[l])."""
    f = spacing_factor if spacing_factor > 0.0 else DEFAULT_SPACING_FACTOR
    d = x.shape[1]
    lo, hi = x.min(axis=0), x.max(axis=0)
    ext = hi - lo
    lmin = ext.min()
    h = mean_edge_length(x, conn)
    nl = 1 + int(math.floor(math.log2(lmin / (f * h)) + 0.5))
    nl = min(max(nl, 1), MAX_LEVELS)
    n0 = np.maximum(np.ceil(ext / lmin - 1e-9).astype(np.int64), 1)
    n = [n0 * (1 << l) for l in range(nl)]
    return dict(lo=lo, n_levels=nl, n=n, H=[lmin / (1 << l) for l in range(nl)],
                nodes=[int(np.prod(k + 1)) for k in n], dim=d)


def level_weights(plan, x, level):
    """(bin[n_vert, d], frac[n_vert, d]) of the vertices on lattice `level`."""
    last = plan["n_levels"] - 1
    t = (x - plan["lo"]) * (1.0 / plan["H"][last])
    tr = np.rint(t)
    t = np.where(np.abs(t - tr) < SNAP, tr, t)
    t = np.clip(t, 0.0, plan["n"][last]) / (1 << (last - level))
    n = plan["n"][level]
    b = np.clip(np.floor(t).astype(np.int64), 0, n - 1)
    return b, np.clip(t - b, 0.0, 1.0)


def node_index(n, ijk):
    """x fastest: i0 + (n0 + 1) (i1 + (n1 + 1) i2)"""
    idx = ijk[..., -1]
    for k in range(ijk.shape[-1] - 2, -1, -1):
        idx = idx * (n[k] + 1) + ijk[..., k]
    return idx


def scalar_interpolation(plan, x, level):
    """n_vert x nodes[level]: multilinear weights."""
    d = x.shape[1]
    b, f = level_weights(plan, x, level)
    n = plan["n"][level]
    rows, cols, vals = [], [], []
    for corner in itertools.product((0, 1), repeat=d):
        c = np.array(corner)
        w = np.prod(np.where(c == 1, f, 1.0 - f), axis=1)
        rows.append(np.arange(x.shape[0])); cols.append(node_index(n, b + c)); vals.append(w)
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                         shape=(x.shape[0], plan["nodes"][level]))


def interpolation(plan, x, level, fixed_mask=None):
    """P_l: n_dof x d nodes[level], blocked dofs on both sides, zero rows on fixed dofs."""
    d = x.shape[1]
    P = sp.kron(scalar_interpolation(plan, x, level), sp.identity(d), format="csr")
    if fixed_mask is not None:
        P = sp.diags((np.asarray(fixed_mask) == 0).astype(np.float64)) @ P
    return P.tocsr()


def lattice_transfer(plan, fine, coarse):
    """T: d nodes[fine] x d nodes[coarse], multilinear interpolation between nested lattices (P_coarse = P_fine T)."""
    d = plan["dim"]
    nf = plan["n"][fine]
    grid = np.stack(np.meshgrid(*[np.arange(k + 1) for k in nf], indexing="ij"), axis=-1).reshape(-1, d)
    pos = grid * plan["H"][fine] + plan["lo"]
    T = scalar_interpolation(plan, pos, coarse)
    perm = node_index(nf, grid)
    S = sp.csr_matrix((np.ones(len(perm)), (perm, np.arange(len(perm)))), shape=(len(perm),) * 2)
    return sp.kron(S @ T, sp.identity(d), format="csr")


def masked_operator(K, fixed_mask):
    if fixed_mask is None:
        return K.tocsr()
    free = sp.diags((np.asarray(fixed_mask) == 0).astype(np.float64))
    return (free @ K @ free + sp.diags(np.asarray(fixed_mask).astype(np.float64))).tocsr()


def block_diagonal(G, d):
    """(n, d, d) diagonal blocks of a sparse matrix of size n d."""
    G = G.tocsr()
    n = G.shape[0] // d
    B = np.zeros((n, d, d))
    for r in range(d):
        for c in range(d):
            B[:, r, c] = G[r::d][:, c::d].diagonal()
    return B


def galerkin_blocks(P, A, d):
    return block_diagonal((P.T @ A @ P).tocsr(), d)


def invert_blocks(B):
    """Inverse of every block; components with a zero diagonal entry get a zero row and column."""
    d = B.shape[1]
    dead = np.stack([B[:, r, r] == 0.0 for r in range(d)], axis=1)
    W = B.copy()
    for r in range(d):
        W[dead[:, r], r, :] = 0.0
        W[dead[:, r], :, r] = 0.0
        W[dead[:, r], r, r] = 1.0
    Ci = np.linalg.inv(W)
    for r in range(d):
        Ci[dead[:, r], r, :] = 0.0
        Ci[dead[:, r], :, r] = 0.0
    return Ci


def cell_blocks(plan, x, conn, coef, level, fixed_mask=None, E=1.0, nu=0.3):
    """The closed form, cell by cell: with g_r = sum_a w_aI m_ar grad(lambda_a) (m_ar = 0 on a fixed dof), cell e adds
    coef_e |T_e| (lam0 g_r[r] g_c[c] + mu0 (g_r[c] g_c[r] + delta_rc g_r . g_c)) to entry (r, c) of the block of node I."""
    d = x.shape[1]
    lam, mu = ref.lame(E, nu)
    S = scalar_interpolation(plan, x, level).tocsr()
    free = np.ones((x.shape[0], d)) if fixed_mask is None else (np.asarray(fixed_mask).reshape(-1, d) == 0).astype(np.float64)
    B = np.zeros((plan["nodes"][level], d, d))
    for e, cv in enumerate(conn):
        g, vol = ref.grads_and_volume(x[cv])
        Se = S[cv].tocoo()
        for I in np.unique(Se.col):
            w = np.zeros(len(cv))
            w[Se.row[Se.col == I]] = Se.data[Se.col == I]
            G = np.stack([(w * free[cv, r]) @ g for r in range(d)])       # G[r] = g_r
            for r in range(d):
                for c in range(d):
                    t = lam * G[r, r] * G[c, c] + mu * G[r, c] * G[c, r]
                    if r == c:
                        t += mu * (G[r] @ G[c])
                    B[I, r, c] += coef[e] * vol * t
    return B


class Multilevel:
    """M^-1 of the module docstring for one mesh, density and fixed set."""

    def __init__(self, x, conn, rho, method="SIMP", fixed_mask=None, spacing_factor=0.0, E=1.0, nu=0.3, K=None):
        self.d = d = x.shape[1]
        self._x = x
        self.plan = lattice_plan(x, conn, spacing_factor)
        self.mask = None if fixed_mask is None else np.asarray(fixed_mask, dtype=np.uint8)
        K = ref.stiffness(x, conn, rho, method, E, nu) if K is None else K
        self.A = masked_operator(K, self.mask)
        self.Dinv = invert_blocks(block_diagonal(self.A, d))
        self.P = [interpolation(self.plan, x, l, self.mask) for l in range(self.plan["n_levels"])]
        self.G = [galerkin_blocks(P, self.A, d) for P in self.P]
        self.C = [invert_blocks(G) for G in self.G]

    def jacobi(self, r):
        return np.einsum("nij,nj->ni", self.Dinv, r.reshape(-1, self.d)).ravel()

    def apply(self, r):
        z = self.jacobi(r)
        for P, C in zip(self.P, self.C):
            z += P @ np.einsum("nij,nj->ni", C, (P.T @ r).reshape(-1, self.d)).ravel()
        return z

    def apply_abs(self, r):
        """a = |D^-1| |r| + sum_l |P_l| |C_l| |P_l^T| |r|: what the rounding errors of one application are measured in."""
        r = np.abs(r)
        a = np.einsum("nij,nj->ni", np.abs(self.Dinv), r.reshape(-1, self.d)).ravel()
        for P, C in zip(self.P, self.C):
            Pa = abs(P)
            a += Pa @ np.einsum("nij,nj->ni", np.abs(C), (Pa.T @ r).reshape(-1, self.d)).ravel()
        return a

    def apply_long(self, r):
        """`apply` with the same fp64 D^-1, P_l and C_l, every product and sum in np.longdouble."""
        ld, d = np.longdouble, self.d
        r = np.asarray(r, dtype=ld)
        z = np.einsum("nij,nj->ni", self.Dinv.astype(ld), r.reshape(-1, d)).ravel()
        for P, C in zip(self.P, self.C):
            P = P.tocoo()
            w = P.data.astype(ld)
            g = np.zeros(P.shape[1], dtype=ld)
            np.add.at(g, P.col, w * r[P.row])
            e = np.einsum("nij,nj->ni", C.astype(ld), g.reshape(-1, d)).ravel()
            np.add.at(z, P.row, w * e[P.col])
        return z

    def longest_restriction_list(self):
        """n_hat: the most vertices under the hat of one node of the finest lattice."""
        S = scalar_interpolation(self.plan, self._x, self.plan["n_levels"] - 1).tocsc()
        S.eliminate_zeros()
        return int(np.diff(S.indptr).max())


def pcg(A, b, precond, fixed_mask=None, rtol=1e-15, atol=0.0, max_it=100000):
    """PCG with the device's protocol: x = b on the fixed dofs, zero elsewhere; stop when r.M^-1 r <= max(rtol^2
    r0.M^-1 r0, atol^2), tested after every iteration.  Returns (x, iterations, converged)."""
    x = np.zeros_like(b)
    if fixed_mask is not None:
        x[np.asarray(fixed_mask) == 1] = b[np.asarray(fixed_mask) == 1]
    r = b - A @ x
    z = precond(r)
    p = z.copy()
    rz = r @ z
    tol2 = max(rtol * rtol * rz, atol * atol)
    if rz <= tol2:
        return x, 0, True
    for it in range(1, max_it + 1):
        q = A @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = precond(r)
        rz_new = r @ z
        if rz_new <= tol2:
            return x, it, True
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_it, False


# ------------------------------------------------------------------------------------- the cases of the count tests ----
def truss_density(centroids, height, void=1e-3):
    """Black / white truss in the unit-height 2:1 box: solid where y < 0.1, y > 0.9 or |((x +- y) mod 0.5) - 0.25| < 0.04."""
    xs, ys = centroids[:, 0] / height, centroids[:, 1] / height
    solid = (ys < 0.1) | (ys > 0.9)
    for s in (1.0, -1.0):
        solid |= np.abs(np.mod(xs + s * ys, 0.5) - 0.25) < 0.04
    return np.where(solid, 1.0, void)


def count_density(kind, centroids, height):
    if kind == "uniform":
        return np.full(len(centroids), 0.5)
    if kind == "truss":
        return truss_density(centroids, height)
    if kind == "noise":
        return np.random.default_rng(1).uniform(1e-3, 1.0, len(centroids))
    raise ValueError(kind)


def cantilever_case(x, conn, lx, ly, nely):
    """Fixed mask (clamped at x = 0) and the tip load of the cantilever: traction (0, -1/4) on the facets of the edge
    x = lx within one cell of mid-height."""
    n_vert = x.shape[0]
    mask = np.zeros(2 * n_vert, dtype=np.uint8)
    fv = np.nonzero(np.isclose(x[:, 0], 0.0))[0]
    mask[2 * fv] = 1
    mask[2 * fv + 1] = 1
    on = np.nonzero((np.abs(x[:, 0] - lx) < 3e-6) & (np.abs(x[:, 1] - ly / 2) < ly / nely + 3e-6))[0]
    on = on[np.argsort(x[on, 1])]
    facets = np.stack([on[:-1], on[1:]], axis=1)
    F = ref.traction_load(x, facets, (0.0, -0.25))
    F[mask == 1] = 0.0
    return mask, facets, F


# --------------------------------------------------------------------------------- shared inputs of the two test files ----
L_X, L_Y = 160.0, 80.0


def small_meshes():
    from femo_amd.fea.mesh import createRectangleMesh, createUnitCubeMesh, createUnitSquareMesh
    return {"rect8x4": lambda: createRectangleMesh([0.0, 0.0], [2.0, 1.0], 8, 4),
            "square9j": lambda: createUnitSquareMesh(9, 0.25),
            "cube4j": lambda: createUnitCubeMesh(4, 0.2)}


LDS_DOUBLES = 2048          # a level of more than LDS_DOUBLES / d^2 nodes adds its blocks with global atomics
COARSE_THREADS = 1024       # a lattice below the finest with more nodes takes the one-workgroup sweep more than one trip


def path_meshes():
    """name -> (mesh factory, spacing factor): the cases on which the other paths of csrc/elast_pc.hip engage.  What each
    is for stands in PATH_PLANS below and is asserted from the plan by the tests that use it."""
    import wide_meshes as W
    from femo_amd.fea.mesh import Mesh, createRectangleMesh, createUnitCubeMesh

    def box8j():
        m = createUnitCubeMesh(8, 0.2)
        return Mesh(m.x * np.array([1.0, 1.0, 2.0]), m.conn)

    return {"rect52x26": (lambda: createRectangleMesh([0.0, 0.0], [2.0, 1.0], 52, 26), 0.0),
            "rect30x20_wide": (lambda: createRectangleMesh([0.0, 0.0], [1.5, 1.0], 30, 20), 1.0),
            "rect64x32_fine": (lambda: createRectangleMesh([0.0, 0.0], [2.0, 1.0], 64, 32), 0.5),
            "fan64x24_random": (lambda: Mesh(*W.renumber(*W.fan(64, 24), W.random_numbering(1537, 11))), 1.0),
            "cube8j": (lambda: createUnitCubeMesh(8, 0.2), 1.0),
            "cube5_8": (lambda: Mesh(*W.cube5(8)), 1.0),
            "box8j_fine": (box8j, 0.25),
            "fan40x8": (lambda: Mesh(*W.fan(40, 8)), 1.0)}                  # host tests only: small enough for cell_blocks


# vertices, cells, nodes per level (coarsest first) of path_meshes(), as lattice_plan gave them when the cases were chosen
PATH_PLANS = {"rect52x26": (1431, 2704, [6, 15, 45, 153, 561]),
              "rect30x20_wide": (651, 1200, [6, 15, 45, 153, 561]),
              "rect64x32_fine": (2145, 4096, [6, 15, 45, 153, 561, 2145, 8385]),
              "fan64x24_random": (1537, 3008, [4, 9, 25, 81, 289, 1089]),
              "cube8j": (729, 3072, [8, 27, 125, 729]),
              "cube5_8": (729, 2560, [8, 27, 125, 729]),
              "box8j_fine": (729, 3072, [12, 45, 225, 1377, 9537]),
              "fan40x8": (321, 600, [4, 9, 25, 81, 289])}
# levels on the global-atomic block path, levels below the finest that the one-workgroup sweep takes in several trips
PATH_LEVELS = {"rect52x26": ([4], []), "rect30x20_wide": ([4], []), "rect64x32_fine": ([4, 5, 6], [5]),
               "fan64x24_random": ([5], []), "cube8j": ([3], []), "cube5_8": ([3], []), "box8j_fine": ([3, 4], [3]),
               "fan40x8": ([], [])}
# per level under path_mask: nodes with an all-zero block, nodes with some but not all diagonal entries zero (the
# restatement's counts; the lattice nodes no vertex reaches are 0, 3, 10, 36, 136 on rect30x20_wide, 6240 of the finest on
# rect64x32_fine, 4, 32, 184 on the fan, 132 and 6764 on the stretched box)
PATH_DEAD = {"rect52x26": ([0, 0, 0, 0, 0], [0, 3, 10, 36, 136]),
             "rect30x20_wide": ([0, 3, 10, 36, 136], [0, 0, 5, 27, 102]),
             "rect64x32_fine": ([0, 0, 0, 0, 0, 33, 6273], [0, 3, 10, 36, 136, 528, 528]),
             "fan64x24_random": ([0, 0, 0, 4, 32, 184], [0, 0, 5, 16, 52, 178]),
             "cube8j": ([0, 0, 0, 29], [0, 0, 25, 165]),
             "cube5_8": ([0, 0, 0, 81], [0, 0, 25, 162]),
             "box8j_fine": ([0, 0, 0, 180, 6845], [0, 0, 45, 291, 666]),
             "fan40x8": ([0, 0, 0, 4, 41], [0, 0, 5, 16, 48])}
PATH_GPU_CASES = ["rect52x26", "rect30x20_wide", "rect64x32_fine", "fan64x24_random", "cube8j", "cube5_8", "box8j_fine"]


def path_mask(mesh):
    """The fixed set of the path cases: the clamped face x = 0 (where the mesh has no such face, as the fan, all dofs of
    the vertex with the smallest x), then component 1 of every vertex in the quarter x > x_min + 0.75 (x_max - x_min): a
    region of rollers, under which lattice nodes keep some components and lose the others."""
    d, xs = mesh.tdim, mesh.x[:, 0]
    if np.isclose(xs.min(), 0.0):
        mask = clamped_face(mesh)
    else:
        mask = np.zeros(d * mesh.n_vert, dtype=np.uint8)
        mask[d * int(np.argmin(xs)):d * (int(np.argmin(xs)) + 1)] = 1
    mask[d * np.nonzero(xs > xs.min() + 0.75 * (xs.max() - xs.min()))[0] + 1] = 1
    return mask


_PATH_CASES = {}


def path_case(name, method="SIMP"):
    """(mesh, spacing factor, rho, mask, Multilevel) of one path case, built once per process and shared: read only."""
    if (name, method) not in _PATH_CASES:
        make, f = path_meshes()[name]
        mesh = make()
        rho = np.random.default_rng(7).uniform(1e-3, 1.0, mesh.n_cell)
        mask = path_mask(mesh)
        _PATH_CASES[name, method] = (mesh, f, rho, mask, Multilevel(mesh.x, mesh.conn, rho, method, mask, spacing_factor=f))
    return _PATH_CASES[name, method]


def path_levels(nodes, d):
    """(levels on the atomic block path, levels below the finest above COARSE_THREADS nodes) of a list of node counts."""
    return ([l for l, n in enumerate(nodes) if n * d * d > LDS_DOUBLES],
            [l for l, n in enumerate(nodes[:-1]) if n > COARSE_THREADS])


def max_valence(conn):
    """(vertex, its number of distinct neighbours) of the longest row."""
    nv = conn.shape[1]
    e = np.concatenate([conn[:, [a, b]] for a in range(nv) for b in range(nv) if a != b])
    e = np.unique(e, axis=0)
    cnt = np.bincount(e[:, 0])
    return int(cnt.argmax()), int(cnt.max())


def is_lexicographic(x):
    """Vertices numbered by ascending (z, y, x), x fastest, as the structured constructors number them."""
    return bool(np.array_equal(np.lexsort(x.T), np.arange(len(x))))


def dead_counts(G):
    """(nodes with an all-zero diagonal, nodes with some but not all diagonal entries zero) of one level's blocks."""
    z = (np.diagonal(G, axis1=1, axis2=2) == 0.0).sum(axis=1)
    return int((z == G.shape[1]).sum()), int(((z > 0) & (z < G.shape[1])).sum())


def lame_ratio(E=1.0, nu=0.3):
    lam, mu = ref.lame(E, nu)
    return (lam + mu) / mu


def block_bound(G, n_cell, E=1.0, nu=0.3):
    """(nodes,): the most an entry of a node's block may differ between two fp64 evaluations.  An entry is a sum of at
    most n_cell cell terms (plus the flushes of the workgroups that accumulate in LDS, 64 covers them with the roundings of
    a term); the diagonal terms are non-negative with t_rr >= mu0 |g_r|^2, so |t_rc| <= (lam0 + mu0) |g_r| |g_c| <=
    ((lam0 + mu0) / mu0) max(t_rr, t_cc); the leading 2 covers the sparse products of this file."""
    return 2.0 * (n_cell + 64) * 2.0 ** -53 * lame_ratio(E, nu) * np.diagonal(G, axis1=1, axis2=2).max(axis=1)


def block_entry_bound(G, n_cell, E=1.0, nu=0.3):
    """(nodes, d, d): block_bound entry by entry.  |t_rc| <= ((lam0 + mu0) / mu0) sqrt(t_rr t_cc) cell by cell, and
    sum_e sqrt(t_rr t_cc) <= sqrt(G_rr G_cc) by Cauchy-Schwarz, so entry (r, c) carries sqrt(G_rr G_cc) where block_bound
    has the node's largest diagonal entry: never more, and far less on a component that only weakly weighted free
    vertices reach beside one that is reached in full."""
    dg = np.diagonal(G, axis1=1, axis2=2)
    return 2.0 * (n_cell + 64) * 2.0 ** -53 * lame_ratio(E, nu) * np.sqrt(dg[:, :, None] * dg[:, None, :])


def block_conditions(G):
    """Condition number of the live part of every block after scaling it to a unit diagonal (nan for an all-zero block).
    This is the number that carries block_entry_bound to the inverse: with S = diag(G)^-1/2 the error of S G S is at most
    the relative bound in every entry, C = S (S G S)^-1 S, and the scaling cancels from error and inverse alike.  (The
    unscaled condition number reaches 5e6 where rollers leave a node one strongly and one weakly reached component.)"""
    d = G.shape[1]
    dg = np.diagonal(G, axis1=1, axis2=2)
    live = dg != 0.0
    s = np.where(live, 1.0 / np.sqrt(np.where(live, dg, 1.0)), 0.0)
    Gs = G * s[:, :, None] * s[:, None, :]
    out = np.full(G.shape[0], np.nan)
    for pat in itertools.product((False, True), repeat=d):
        k = np.nonzero(pat)[0]
        sel = np.nonzero((live == np.array(pat)).all(axis=1))[0]
        if len(k) and len(sel):
            out[sel] = np.linalg.cond(Gs[sel][:, k][:, :, k])
    return out


def apply_gamma(M):
    """gamma_s of one application: unit round-off times the length of its longest chain of sums, n_hat terms of the mesh
    restriction, 3^d down and 2^d <= 3^d up per level, d-term block products and the two gathers of the last kernel."""
    d = M.d
    return 2.0 ** -53 * (M.longest_restriction_list() + 2 * 3 ** d * M.plan["n_levels"] + 8 * d)


def apply_bound(M, n_cell, r, E=1.0, nu=0.3):
    """Per entry: (gamma_s + 4 beta) a, beta the relative block error of block_bound without its leading 2, times 4 for the
    condition number of a live block (block_conditions <= 4 is asserted beside every use)."""
    beta = (n_cell + 64) * 2.0 ** -53 * lame_ratio(E, nu)
    return (apply_gamma(M) + 4.0 * beta) * M.apply_abs(r)



def clamped_face(mesh):
    """uint8 mask of the dofs of the vertices on x = 0."""
    d = mesh.tdim
    mask = np.zeros(d * mesh.n_vert, dtype=np.uint8)
    fv = np.nonzero(np.isclose(mesh.x[:, 0], 0.0))[0]
    mask[(fv[:, None] * d + np.arange(d)).ravel()] = 1
    return mask


def count_case(nelx, nely, kind):
    """(mesh, rho, mask, facets, F) of the count tests: the L_X x L_Y cantilever with the fixed density ``kind``."""
    from femo_amd.fea.mesh import createRectangleMesh
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([L_X, L_Y]), nelx, nely)
    mask, facets, F = cantilever_case(mesh.x, mesh.conn, L_X, L_Y, nely)
    rho = count_density(kind, mesh.centroids(), L_Y)
    return mesh, rho, mask, facets, F


def build_cantilever(preconditioner, nelx=80, nely=40, device=False, seed=0):
    """The cantilever of run_topo_opt_cantilever_beam.py through FEAModel + GeneralFilterModel + Simulator, as in
    tests/test_gpu_topopt.py, with the preconditioner of the state and adjoint solves chosen."""
    from femo_amd.csdl_opt.fea_model import FEAModel
    from femo_amd.csdl_opt.filter_model import GeneralFilterModel
    from femo_amd.csdl_opt.simulator import Simulator
    from femo_amd.fea.elasticity import averageFunc, compliance, pdeRes
    from femo_amd.fea.fea_hip import (FEA, Constant, Function, FunctionSpace, Measure, TestFunction, VectorFunctionSpace,
                                      createRectangleMesh, locate_dofs_geometrical, locate_entities_boundary, meshSize,
                                      meshtags)
    mesh = createRectangleMesh(np.array([0.0, 0.0]), np.array([L_X, L_Y]), nelx, nely)
    eps = 3e-6
    marker = lambda x: np.logical_and(abs(x[1] - L_Y / 2) < L_Y / nely + eps, abs(x[0] - L_X) < eps)
    facets = locate_entities_boundary(mesh, mesh.tdim - 1, marker)
    tags = meshtags(mesh, mesh.tdim - 1, facets, np.full(len(facets), 100, dtype=np.int32))
    ds_ = Measure('ds', domain=mesh, subdomain_data=tags)
    fea = FEA(mesh)
    fea.REPORT = False
    Q, V = FunctionSpace(mesh, ('DG', 0)), VectorFunctionSpace(mesh, ('CG', 1))
    rho_fn, u_fn = Function(Q), Function(V)
    f = Constant(mesh, (0, -1 / 4))
    res = pdeRes(u_fn, TestFunction(V), rho_fn, f, dss=ds_(100), preconditioner=preconditioner)
    fea.add_input('density', rho_fn)
    fea.add_state(name='displacements', function=u_fn, residual_form=res, arguments=['density'])
    fea.add_output(name='compliance', type='scalar', form=compliance(u_fn, f, dss=ds_(100)), arguments=['displacements'])
    ubc = Function(V)
    ubc.vector.set(0.0)
    fea.add_strong_bc(ubc, [locate_dofs_geometrical((V, V), lambda x: np.isclose(x[0], 0., atol=1e-6))], V)
    model = FEAModel(fea=[fea])
    h = meshSize(mesh)
    h_avg = (h.max() + h.min()) / 2
    model.add(GeneralFilterModel(nel=mesh.n_cell, coordinates=Q.tabulate_dof_coordinates(), h_avg=h_avg),
              name='general_filter_model')
    model.create_input('density_unfiltered', shape=mesh.n_cell, val=np.random.default_rng(seed).random(mesh.n_cell) * 0.86)
    model.add_design_variable('density_unfiltered', upper=1.0, lower=1e-4)
    model.add_objective('compliance')
    return Simulator(model, device=device), mesh, dict(facets=facets, h_avg=h_avg, res=res)


def reference_cycle(mesh, facets, h_avg, x0, method="SIMP"):
    """filter -> K(rho) u = F -> compliance -> gradient with SciPy's direct solver."""
    W = ref.filter_matrix(mesh.centroids(), 2.0 * h_avg)
    rho = W @ x0
    K0 = ref.element_matrices(mesh.x, mesh.conn)
    K = ref.stiffness(mesh.x, mesh.conn, rho, method, K0=K0)
    F = ref.traction_load(mesh.x, facets, (0.0, -0.25))
    fixed_v = np.nonzero(np.isclose(mesh.x[:, 0], 0.0))[0]
    fixed = np.concatenate([2 * fixed_v, 2 * fixed_v + 1])
    u = ref.solve_fixed(K, F, fixed)
    dJ = -ref.compliance_gradient(mesh.x, mesh.conn, rho, u, u, method, K0=K0)
    return dict(rho=rho, u=u, J=F @ u, grad=W.T @ dJ, K=K, F=F, fixed=fixed)
