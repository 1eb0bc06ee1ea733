"""Host topology of meshes with rows of more than 14 off-diagonal entries (tests/wide_meshes.py): the slice classes the
GPU tests of tests/test_gpu_wide_rows.py rely on, the CSR export on both sides of the 32-bit structural-zero mask, the
+-32767 edge of the 16-bit column class and the 254-entry limit of the slot map.  No GPU."""
import numpy as np
import pytest

import wide_meshes as W
from oracle import femo_oracle as fo


def _cube6():
    m = fo.unit_cube_mesh(6)
    return m.x, m.conn


def _fan_random(rings):
    x, conn = W.fan(40, rings)
    return W.renumber(x, conn, W.random_numbering(len(x), 5))


# name -> (mesh, expected info values; n_vert is checked as the number of vertices of the construction)
MESHES = {
    "fan16": (lambda: W.fan(16, 6), dict(n_vert=97, n_slices=2, max_rowlen=16, regular_slices=0, short_slices=2)),
    "fan40": (lambda: W.fan(40, 6), dict(n_vert=241, n_slices=4, max_rowlen=40, regular_slices=2, short_slices=2)),
    "fan62": (lambda: W.fan(62, 6), dict(n_vert=373, n_slices=6, max_rowlen=62, regular_slices=3, short_slices=3)),
    "fan63": (lambda: W.fan(63, 6), dict(max_rowlen=63)),
    "fan84": (lambda: W.fan(84, 6), dict(max_rowlen=84)),
    "fan85": (lambda: W.fan(85, 6), dict(max_rowlen=85)),
    "fan254": (lambda: W.fan(254, 6), dict(max_rowlen=254)),
    "fan40x8_random": (lambda: _fan_random(8), dict(n_vert=321, n_slices=6, max_rowlen=40, regular_slices=0, short_slices=6)),
    "fan40x900_random": (lambda: _fan_random(900), dict(n_vert=36001, n_slices=563, max_rowlen=40, regular_slices=0, short_slices=463)),
    "fan40x900_rings": (lambda: W.fan(40, 900), dict(n_vert=36001, n_slices=563, regular_slices=560)),
    "bipyramid13": (lambda: W.bipyramid(13), dict(max_rowlen=15)),
    "bipyramid14": (lambda: W.bipyramid(14), dict(max_rowlen=16)),
    "bipyramid30": (lambda: W.bipyramid(30), dict(max_rowlen=32)),
    "bipyramid31": (lambda: W.bipyramid(31), dict(max_rowlen=33)),
    "bipyramid61": (lambda: W.bipyramid(61), dict(n_vert=64, n_slices=1, max_rowlen=63)),
    "bipyramid62": (lambda: W.bipyramid(62), dict(max_rowlen=64)),
    "bipyramid63": (lambda: W.bipyramid(63), dict(max_rowlen=65)),
    "cube6_bipyramid13": (lambda: W.union(_cube6(), W.bipyramid(13), (3.0, 0.0, 0.0)),
                          dict(n_vert=359, n_slices=6, max_rowlen=15, regular_slices=3, short_slices=3)),
    "cube6_bipyramid14": (lambda: W.union(_cube6(), W.bipyramid(14), (3.0, 0.0, 0.0)),
                          dict(n_vert=360, n_slices=6, max_rowlen=16, regular_slices=3, short_slices=3)),
    "cube5_8": (lambda: W.cube5(8), dict(n_vert=729, n_slices=12, max_rowlen=18, regular_slices=7, short_slices=5)),
    "strip32760": (lambda: W.strip(32760, 4, 1), dict(n_vert=65520, n_slices=1024, regular_slices=0, short_slices=1024)),
    "strip32764": (lambda: W.strip(32764, 4, 1), dict(n_vert=65528, n_slices=1024, regular_slices=0, short_slices=0)),
}

_CACHE = {}


def _built(name):
    if name not in _CACHE:
        from femo_amd import engine as E
        x, conn = MESHES[name][0]()
        info, rowptr, col = E.topology_host(x.shape[1], len(x), len(x), conn)
        _CACHE[name] = (x, conn, info, rowptr, col)
    return _CACHE[name]


def _deltas(rowptr, col):
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return rows, col.astype(np.int64) - rows


@pytest.mark.parametrize("name", sorted(MESHES))
def test_info_and_pattern(name):
    x, conn, info, rowptr, col = _built(name)
    assert conn.dtype == np.int32
    p = x[conn]
    assert (np.linalg.det(p[:, 1:] - p[:, :1]) != 0.0).all()                     # no degenerate cell
    got = {k: info[k] for k in MESHES[name][1]}
    assert got == MESHES[name][1]
    assert info["n_vert"] == len(x)
    K = fo.stiffness(fo.OMesh(x.shape[1], x, conn))
    assert np.array_equal(rowptr, K.indptr) and np.array_equal(col, K.indices)
    assert info["max_rowlen"] == int(np.diff(K.indptr).max()) - 1                # the diagonal is not counted


@pytest.mark.parametrize("name", ["fan16", "fan40", "bipyramid14", "cube5_8"])
def test_constructions_are_positively_oriented(name):
    x, conn = _built(name)[:2]
    p = x[conn]
    assert (np.linalg.det(p[:, 1:] - p[:, :1]) > 0.0).all()


def test_row_lengths_of_the_constructions():
    """What the docstrings of tests/wide_meshes.py promise: hub and pole rows, and 18 / 6 in the 5-tetrahedra cube."""
    _, _, _, rowptr, _ = _built("fan40")
    rl = np.diff(rowptr) - 1
    assert rl[0] == 40 and rl[1:].max() == 6
    _, _, _, rowptr, _ = _built("bipyramid30")
    rl = np.diff(rowptr) - 1
    assert rl[0] == 32 and rl[1] == rl[2] == 31 and (rl[3:] == 5).all()
    x, conn, _, rowptr, _ = _built("cube5_8")
    rl = np.diff(rowptr) - 1
    ijk = np.rint(x * 8).astype(int)
    interior = ((ijk > 0) & (ijk < 8)).all(axis=1)
    even = ijk.sum(axis=1) % 2 == 0
    assert (rl[interior & even] == 18).all() and (rl[interior & ~even] == 6).all()
    p = x[conn]
    assert abs(np.abs(np.linalg.det(p[:, 1:] - p[:, :1])).sum() / 6.0 - 1.0) < 1e-13


def test_rows_past_the_structural_zero_mask_export_every_entry():
    """Rows of 32 and more entries: entries 32 ... of a row are never structural zeros (femo_topology_csr's k >= 32 arm)."""
    for name, hub_len in (("bipyramid30", 32), ("bipyramid31", 33), ("fan40", 40), ("fan254", 254)):
        x, conn, info, rowptr, col = _built(name)
        assert rowptr[1] - rowptr[0] == hub_len + 1
        assert np.array_equal(col[:hub_len + 1], np.arange(hub_len + 1))          # the hub couples to vertices 1 ... hub_len
        assert info["nnz"] == rowptr[-1]


def test_regular_slices_wider_than_14():
    """A completed regular slice of cube5(8) is 18 wide (each holds an interior even vertex): 9 pairs per row."""
    _, _, info, rowptr, _ = _built("cube5_8")
    assert info["regular_slices"] == 7
    # stored entries: the regular slices store 18 per row, structural zeros included, so more than the pattern holds
    assert info["sell_entries"] >= 7 * 64 * 18
    assert info["sell_entries"] > info["nnz"] - info["n_vert"]


def test_sixteen_bit_class_edge():
    """Computed from the exported pattern, so that a change to the generator cannot silently move the edge: at N = 32760
    the largest |col - row| is 32767 exactly, with both signs, and every slice is in the 16-bit class; at N = 32764 every
    slice holds a column further than 32767 away and none is."""
    _, _, info, rowptr, col = _built("strip32760")
    rows, d = _deltas(rowptr, col)
    assert d.max() == 32767 and d.min() == -32767
    assert len(np.unique(rows[np.abs(d) == 32767] // 64)) == 719
    assert info["short_slices"] == info["n_slices"] == 1024
    _, _, info, rowptr, col = _built("strip32764")
    rows, d = _deltas(rowptr, col)
    assert np.abs(d).max() == 32771
    far = np.unique(rows[np.abs(d) > 32767] // 64)
    assert len(far) == info["n_slices"] == 1024 and info["short_slices"] == 0


def test_random_fan_has_both_irregular_classes():
    _, _, info, rowptr, col = _built("fan40x900_random")
    rows, d = _deltas(rowptr, col)
    far = np.unique(rows[np.abs(d) > 32767] // 64)
    assert len(far) == 100 == info["n_slices"] - info["short_slices"]


def test_255_entries_are_rejected_and_the_next_build_succeeds():
    from femo_amd import engine as E
    x, conn = W.fan(255, 6)
    with pytest.raises(E.FemoError, match="exceeds the 8-bit slot map"):
        E.topology_host(2, len(x), len(x), conn)
    x, conn = W.fan(254, 6)
    info, rowptr, col = E.topology_host(2, len(x), len(x), conn)
    assert info["max_rowlen"] == 254
    K = fo.stiffness(fo.OMesh(2, x, conn))
    assert np.array_equal(rowptr, K.indptr) and np.array_equal(col, K.indices)
