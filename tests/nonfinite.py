"""Plain helpers of tests/test_gpu_nonfinite.py: poisoning one entry of a floating-point input, the topological dependent
sets of a mesh, and the two-sided check of the contract "no output hides a non-finite state" ("Non-finite
inputs").  No fixtures, no device code.

The contract for one output array of one call with one poisoned input entry:

  never hides      the output is non-finite wherever the float64 restatement, evaluated on the poisoned input, is;
  does not spray   outside the dependent set the output is finite and is the device's own clean result (bit for bit, or
                   to the kernel's parity tolerance where it sums with float atomics);
  finite decides   where the restatement is finite inside the dependent set, the output equals it to the parity tolerance.
"""
import numpy as np

VALUES = (np.nan, np.inf, -np.inf)


def poison(v, i, value):
    """A float64 copy of ``v`` with the flat entry ``i`` set to ``value``; same shape."""
    out = np.array(v, dtype=np.float64, copy=True)
    out.reshape(-1)[i] = value
    return out


# ---- dependent sets from the connectivity --------------------------------------------------------------------------------
def cells_of_vertex(conn, vertex):
    """Mask over the cells that touch ``vertex``."""
    return np.any(np.asarray(conn) == vertex, axis=1)


def cells_of_entry(cell_entries, entry):
    """Mask over the cells whose row of ``cell_entries`` (n_cell, k: vertices, or dofs) holds ``entry``."""
    return np.any(np.asarray(cell_entries) == entry, axis=1)


def one_cell(n_cell, cell):
    m = np.zeros(n_cell, dtype=bool)
    m[cell] = True
    return m


def entries_of_cells(cell_entries, cells, n):
    """Mask over 0..n-1 of the entries (vertices, or dofs) in the rows ``cells`` of ``cell_entries``."""
    m = np.zeros(n, dtype=bool)
    m[np.unique(np.asarray(cell_entries)[cells])] = True
    return m


def vertex_dofs(vertex_mask, d):
    """Blocked dofs (d * vertex + component) of a vertex mask."""
    return np.repeat(vertex_mask, d)


def in_column(mask, n_cols, column):
    """(n_cols, len(mask)) mask that is ``mask`` in ``column`` (None: in every column) and empty elsewhere."""
    out = np.zeros((n_cols, mask.size), dtype=bool)
    out[slice(None) if column is None else column] = mask
    return out


def positions(conn, n_entries_per_vertex, block=256):
    """Three vertices to poison: one in the first wave of the first block, one of a cell in the last, partly filled block
    of cells, and the last vertex.  Returned as flat entries with the component varied."""
    conn = np.asarray(conn)
    n_cell, n_vert, k = len(conn), int(conn.max()) + 1, n_entries_per_vertex
    tail = (n_cell - 1) // block * block                      # first cell of the last block
    assert n_cell > block and n_cell % block != 0, "the mesh must end in a partly filled block of cells"
    mid_vertex = int(conn[tail + (n_cell - tail) // 2][1])
    return [3 * k, mid_vertex * k + (k - 1), n_vert * k - 1]


def cell_positions(n_cell, block=256):
    """Three cells to poison: first wave of the first block, inside the last, partly filled block, the last one."""
    tail = (n_cell - 1) // block * block
    assert n_cell > block and n_cell % block != 0
    return [5, tail + (n_cell - tail) // 2, n_cell - 1]


# ---- the two-sided check ----------------------------------------------------------------------------------------------------
def violations(got, want, clean, dependent, tol=None, decide_tol=1e-12, scale=None, label=""):
    """The contract above for one output; returns a list of messages, empty when it holds.

    got        device output on the poisoned input         want       restatement on the poisoned input
    clean      device output on the clean input            dependent  mask of the entries that may differ from ``clean``
    tol        outside the dependent set: None for bit for bit, else relative to ``scale`` (default max |clean|)
    decide_tol ``got`` against a finite ``want`` inside the dependent set, relative to ``scale``; an array: absolute, per entry"""
    got, want, clean = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (got, want, clean))
    dependent = np.broadcast_to(np.atleast_1d(np.asarray(dependent, dtype=bool)), got.shape)
    assert got.shape == want.shape == clean.shape, (label, got.shape, want.shape, clean.shape)
    assert np.all(np.isfinite(clean)), f"{label}: the clean result is not finite"
    scale = float(np.abs(clean).max()) if scale is None else float(scale)
    out = []
    hidden = ~np.isfinite(want) & np.isfinite(got)
    if hidden.any():
        i = np.flatnonzero(hidden)
        out.append(f"{label}: hides {i.size} non-finite entries of the restatement (first {i[0]}: got {got.flat[i[0]]!r}, "
                   f"want {want.flat[i[0]]!r})")
    outside = ~dependent
    sprayed = outside & ~np.isfinite(got)
    if sprayed.any():
        i = np.flatnonzero(sprayed)
        out.append(f"{label}: {i.size} non-finite entries outside the dependent set (first {i[0]})")
    same = outside & np.isfinite(got)
    if tol is None:
        moved = same & (got != clean)
    else:
        moved = same & (np.abs(got - clean) > tol * scale)
    if moved.any():
        i = np.flatnonzero(moved)
        out.append(f"{label}: {i.size} entries outside the dependent set differ from the clean call (first {i[0]}: "
                   f"{got.flat[i[0]]!r} against {clean.flat[i[0]]!r})")
    decided = dependent & np.isfinite(want)
    bound = decide_tol * scale if np.ndim(decide_tol) == 0 else np.broadcast_to(np.asarray(decide_tol, dtype=np.float64), got.shape)
    with np.errstate(invalid="ignore"):
        wrong = decided & ~(np.abs(got - want) <= bound)
    if wrong.any():
        i = np.flatnonzero(wrong)
        out.append(f"{label}: {i.size} entries differ from a finite restatement (first {i[0]}: got {got.flat[i[0]]!r}, "
                   f"want {want.flat[i[0]]!r})")
    return out
