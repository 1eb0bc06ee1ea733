"""Meshes with rows of more than 14 off-diagonal entries (test infrastructure).

Every construction is valid geometry (no degenerate cell, every cell positively oriented) and returns ``(x, conn)`` with
``conn`` int32.  Row lengths are the numbers of distinct neighbours of a vertex: what ``max_rowlen`` counts."""
import numpy as np


def fan(k: int, rings: int):
    """2-D: a hub at the origin (vertex 0) and ``rings`` concentric rings of ``k`` points (ring r, point i is vertex
    1 + r k + i, radius r + 1).  k hub triangles plus 2 k per annulus.  The hub's row has k entries, every other row at
    most 6."""
    t = 2.0 * np.pi * np.arange(k) / k
    x = [np.zeros((1, 2))]
    for r in range(rings):
        x.append((r + 1.0) * np.stack([np.cos(t), np.sin(t)], axis=1))
    i = np.arange(k)
    j = (i + 1) % k
    cells = [np.stack([np.zeros(k, np.int64), 1 + i, 1 + j], axis=1)]
    for r in range(rings - 1):
        a, b = 1 + r * k, 1 + (r + 1) * k
        cells.append(np.stack([a + i, b + i, b + j], axis=1))
        cells.append(np.stack([a + i, b + j, a + j], axis=1))
    return np.concatenate(x), np.concatenate(cells).astype(np.int32)


def bipyramid(k: int):
    """3-D: hub (vertex 0) at the origin, poles (1, 2) at z = +-1, ``k`` points (3 ...) on the unit circle of z = 0; the
    2 k tetrahedra (hub, r_i, r_i+1, pole).  The hub's row has k + 2 entries, a pole's k + 1, an equator point's 5."""
    t = 2.0 * np.pi * np.arange(k) / k
    x = np.concatenate([[[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]],
                        np.stack([np.cos(t), np.sin(t), np.zeros(k)], axis=1)])
    i = 3 + np.arange(k)
    j = 3 + (np.arange(k) + 1) % k
    hub = np.zeros(k, np.int64)
    top = np.stack([hub, i, j, hub + 1], axis=1)
    bottom = np.stack([hub, j, i, hub + 2], axis=1)          # mirrored: swapped to stay positively oriented
    return x, np.concatenate([top, bottom]).astype(np.int32)


def cube5(n: int):
    """3-D: the unit cube in n^3 boxes of 5 tetrahedra each (four corner tetrahedra and the central one), mirrored by
    the parity of i + j + k so that the face diagonals of neighbouring boxes coincide.  Lexicographic numbering, x
    fastest.  A vertex with even i + j + k has up to 18 neighbours (6 along the axes, 12 across face diagonals), an odd
    one up to 6."""
    g = np.linspace(0.0, 1.0, n + 1)
    Z, Y, X = np.meshgrid(g, g, g, indexing="ij")
    x = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    np1 = n + 1
    kk, jj, ii = (a.ravel() for a in np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"))
    base = kk * np1 * np1 + jj * np1 + ii
    c = lambda dx, dy, dz: base + dx + dy * np1 + dz * np1 * np1
    even = [[c(0, 0, 0), c(1, 1, 0), c(0, 1, 1), c(1, 0, 1)],               # the central tetrahedron: the box's even corners
            [c(1, 0, 0), c(0, 0, 0), c(1, 0, 1), c(1, 1, 0)],
            [c(0, 1, 0), c(0, 0, 0), c(1, 1, 0), c(0, 1, 1)],
            [c(0, 0, 1), c(0, 0, 0), c(0, 1, 1), c(1, 0, 1)],
            [c(1, 1, 1), c(1, 1, 0), c(1, 0, 1), c(0, 1, 1)]]
    m = lambda dx, dy, dz: c(1 - dx, dy, dz)                                # odd boxes: the same split mirrored in x
    odd = [[m(0, 0, 0), m(1, 1, 0), m(0, 1, 1), m(1, 0, 1)],
           [m(1, 0, 0), m(0, 0, 0), m(1, 0, 1), m(1, 1, 0)],
           [m(0, 1, 0), m(0, 0, 0), m(1, 1, 0), m(0, 1, 1)],
           [m(0, 0, 1), m(0, 0, 0), m(0, 1, 1), m(1, 0, 1)],
           [m(1, 1, 1), m(1, 1, 0), m(1, 0, 1), m(0, 1, 1)]]
    is_odd = ((ii + jj + kk) % 2 == 1)[:, None]
    conn = np.concatenate([np.where(is_odd, np.stack(o, axis=1), np.stack(e, axis=1)) for e, o in zip(even, odd)])
    return x, _oriented(x, conn).astype(np.int32)


def _oriented(x, conn):
    """Swap the last two vertices of the cells with a negative determinant."""
    p = x[conn]
    neg = np.linalg.det(p[:, 1:] - p[:, :1]) < 0.0
    conn = conn.copy()
    conn[neg, -2], conn[neg, -1] = conn[neg, -1].copy(), conn[neg, -2].copy()
    return conn


def union(a, b, shift):
    """Disjoint union: the vertices of ``a``, then those of ``b`` moved by ``shift`` (far enough not to touch ``a``)."""
    (xa, ca), (xb, cb) = a, b
    x = np.concatenate([xa, xb + np.asarray(shift, dtype=np.float64)])
    return x, np.concatenate([ca, cb + len(xa)]).astype(np.int32)


def strip(N: int, window: int, seed: int):
    """2-D: a 2 x N strip of unit squares' corners, bottom row numbered 0 ... N-1 before the top row N ... 2N-1, right
    diagonals -- every vertex couples to one N or N +- 1 away.  The numbers are then shuffled inside consecutive windows
    of ``window`` by ``default_rng(seed)``, which moves each end of a coupling by up to window - 1."""
    i = np.arange(N - 1)
    x = np.concatenate([np.stack([np.arange(N), np.zeros(N)], axis=1), np.stack([np.arange(N), np.ones(N)], axis=1)])
    conn = np.concatenate([np.stack([i, i + 1, N + i + 1], axis=1), np.stack([i, N + i + 1, N + i], axis=1)])
    rng = np.random.default_rng(seed)
    n = 2 * N
    perm = np.arange(n)
    for lo in range(0, n, window):
        hi = min(lo + window, n)
        perm[lo:hi] = lo + rng.permutation(hi - lo)
    return renumber(x, conn, perm)


def renumber(x, conn, perm):
    """The same mesh with vertex v renamed ``perm[v]``."""
    perm = np.asarray(perm, dtype=np.int64)
    x2 = np.empty_like(x)
    x2[perm] = x
    return x2, perm[conn].astype(np.int32)


def move_vertex(n: int, v: int, to: int):
    """Permutation for ``renumber`` that puts vertex ``v`` at position ``to`` and keeps the order of all others."""
    order = [w for w in range(n) if w != v]
    order.insert(to, v)
    perm = np.empty(n, np.int64)
    perm[np.asarray(order)] = np.arange(n)
    return perm


def random_numbering(n: int, seed: int):
    return np.random.default_rng(seed).permutation(n)
