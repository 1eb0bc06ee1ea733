"""Function spaces and functions (replaces dolfinx.fem.FunctionSpace / Function).

Only the two spaces on the hot path exist: ("CG", 1) on vertices and ("DG", 0)
on cells (run_poisson_opt.py:98-105).  A Function owns one device vector; its
``vector`` attribute offers the three PETSc idioms the reference uses
(utils_dolfinx.py:155-167, 308): ``getArray()``, ``[:] = array`` and ``set(x)``.
"""
from __future__ import annotations

import numpy as np

from ..engine import Vec


class FunctionSpace:
    def __init__(self, mesh, element=("CG", 1)):
        family, degree = element
        from .mesh import BeamMesh
        if (family, degree) == ("Hermite", 3):
            if not isinstance(mesh, BeamMesh):
                raise NotImplementedError("the cubic Hermite element is implemented on interval (beam) meshes only")
        elif (family, degree) not in (("CG", 1), ("Lagrange", 1), ("DG", 0)):
            raise NotImplementedError(
                f"function space {element}: the HIP engine implements CG1 / Hermite-3 states and DG0 inputs only")
        elif isinstance(mesh, BeamMesh) and family != "DG":
            raise NotImplementedError("on a beam mesh the state space is ('Hermite', 3)")
        self.mesh = mesh
        self.family = "DG" if family == "DG" else ("HERMITE" if family == "Hermite" else "CG")
        self.degree = degree
        self.num_sub_spaces = 0

    @property
    def dim(self) -> int:
        return self.mesh.n_cell if self.family == "DG" else self.mesh.n_vert

    def tabulate_dof_coordinates(self) -> np.ndarray:
        if self.family == "DG":
            return self.mesh.centroids()
        return self.mesh.x[:, :1] if self.family == "HERMITE" else self.mesh.x

    def __eq__(self, other):
        return (isinstance(other, FunctionSpace) and other.mesh is self.mesh
                and other.family == self.family and other.degree == self.degree)

    __hash__ = object.__hash__


class VectorFunctionSpace:
    """dolfinx ``VectorFunctionSpace(mesh, ("CG", 1))`` [ext] on a 2-D or 3-D simplex mesh: d = tdim components per vertex in
    the blocked layout dolfinx uses (bs = d): dof = d * vertex + component, which is also the order ``getFuncArray``
    hands to CSDL (run_topo_opt_cantilever_beam.py:108-110).  The scalar ``FunctionSpace`` is left as it is."""

    def __init__(self, mesh, element=("CG", 1)):
        family, degree = element
        if (family, degree) not in (("CG", 1), ("Lagrange", 1)):
            raise NotImplementedError(f"vector function space {element}: only ('CG', 1) is implemented")
        if getattr(mesh, "tdim", None) not in (2, 3) or getattr(mesh, "gdim", mesh.tdim) != mesh.tdim \
                or mesh.conn.shape[1] != mesh.tdim + 1:
            raise NotImplementedError("VectorFunctionSpace needs a 2-D or 3-D simplex Mesh")
        self.mesh = mesh
        self.family = "CGV"
        self.degree = 1
        self.bs = mesh.tdim
        self.num_sub_spaces = mesh.tdim

    @property
    def dim(self) -> int:
        return self.bs * self.mesh.n_vert

    def tabulate_dof_coordinates(self) -> np.ndarray:
        """One row per vertex (the block), as dolfinx tabulates a blocked space."""
        return self.mesh.x

    def sub(self, i: int) -> "_SubSpace":
        if not 0 <= i < self.bs:
            raise IndexError(f"component {i} of a {self.bs}-component space")
        return _SubSpace(self, i)

    def __eq__(self, other):
        return isinstance(other, VectorFunctionSpace) and other.mesh is self.mesh

    __hash__ = object.__hash__


class _SubSpace:
    """``V.sub(i)``: component i of a VectorFunctionSpace; ``dofs`` are its dofs in the parent's numbering."""

    def __init__(self, parent: VectorFunctionSpace, i: int):
        self.parent, self.component = parent, int(i)
        self.mesh = parent.mesh

    @property
    def dofs(self) -> np.ndarray:
        return (np.arange(self.mesh.n_vert, dtype=np.int32) * self.parent.bs + self.component).astype(np.int32)

    def tabulate_dof_coordinates(self) -> np.ndarray:
        return self.mesh.x


class LoadCaseSpace:
    """``n_cases`` copies of a VectorFunctionSpace in one vector, one per load case of the SIMP elasticity: column l holds the
    dofs of ``base`` in its blocked layout and starts at ``l * base.dim`` (the layout of femo_elast_solve_multi).  A
    ``Function(LoadCaseSpace(V, L))`` is an ordinary Function of dimension ``L * V.dim``."""

    def __init__(self, base: VectorFunctionSpace, n_cases: int):
        from .. import _lib
        if not isinstance(base, VectorFunctionSpace):
            raise NotImplementedError("LoadCaseSpace needs a VectorFunctionSpace(mesh, ('CG', 1)) base")
        if not 1 <= int(n_cases) <= _lib.ELAST_MAX_COLS:
            raise ValueError(f"LoadCaseSpace: {n_cases} load cases (1 to {_lib.ELAST_MAX_COLS})")
        self.base, self.n_cases, self.mesh = base, int(n_cases), base.mesh
        self.family = "CGV_CASES"
        self.degree = 1
        self.bs = base.bs
        self.num_sub_spaces = 0

    @property
    def dim(self) -> int:
        return self.n_cases * self.base.dim

    def column(self, l: int) -> slice:
        """The entries of load case ``l`` in a vector of this space."""
        if not 0 <= l < self.n_cases:
            raise IndexError(f"load case {l} of {self.n_cases}")
        return slice(l * self.base.dim, (l + 1) * self.base.dim)

    def tabulate_dof_coordinates(self) -> np.ndarray:
        """The base space's: one row per vertex, the same for every load case."""
        return self.base.tabulate_dof_coordinates()

    def __eq__(self, other):
        return isinstance(other, LoadCaseSpace) and other.base == self.base and other.n_cases == self.n_cases

    __hash__ = object.__hash__


class TimeHistorySpace:
    """``n_steps`` copies of a VectorFunctionSpace in one vector, one per time step of a transient response of the SIMP
    elasticity: step n + 1 of the march holds the dofs of ``base`` in its blocked layout and starts at ``n * base.dim`` (the
    layout of femo_elast_newmark_march).  Any number of steps: the 8-column limit of a `LoadCaseSpace` does not apply.  A
    ``Function(TimeHistorySpace(V, N))`` is an ordinary Function of dimension ``N * V.dim``."""

    def __init__(self, base: VectorFunctionSpace, n_steps: int):
        if not isinstance(base, VectorFunctionSpace):
            raise NotImplementedError("TimeHistorySpace needs a VectorFunctionSpace(mesh, ('CG', 1)) base")
        if int(n_steps) < 1:
            raise ValueError(f"TimeHistorySpace: {n_steps} steps (at least 1)")
        self.base, self.n_steps, self.mesh = base, int(n_steps), base.mesh
        self.family = "CGV_STEPS"
        self.degree = 1
        self.bs = base.bs
        self.num_sub_spaces = 0

    @property
    def dim(self) -> int:
        return self.n_steps * self.base.dim

    def step(self, n: int) -> slice:
        """The entries of u_{n+1} in a vector of this space."""
        if not 0 <= n < self.n_steps:
            raise IndexError(f"step {n} of {self.n_steps}")
        return slice(n * self.base.dim, (n + 1) * self.base.dim)

    def tabulate_dof_coordinates(self) -> np.ndarray:
        """The base space's: one row per vertex, the same for every step."""
        return self.base.tabulate_dof_coordinates()

    def __eq__(self, other):
        return isinstance(other, TimeHistorySpace) and other.base == self.base and other.n_steps == self.n_steps

    __hash__ = object.__hash__


class _VectorView:
    """PETSc-Vec-flavoured access to a Function's device vector."""

    def __init__(self, fn: "Function"):
        self._fn = fn

    def getArray(self) -> np.ndarray:
        # the reference refreshes ghosts before handing the array out (utils_dolfinx.py:155-159 -> 200, 205: ghostUpdate);
        # here it also means the host copy and the device vector agree INCLUDING the ghost tail, at one generation: later
        # operators find the ghosts fresh (no further exchange) and the host copy a valid mirror (no re-upload)
        self.ghostUpdate()
        return self._fn.vec.get()

    def set(self, value) -> None:
        """PETSc ``Vec.set(alpha)`` [ext]: one scalar for every entry (a length-1 array is accepted, as
        ``update`` passes one, utils_dolfinx.py:308-309); arrays go through ``setFuncArray`` / ``v[:] =``."""
        a = np.asarray(value)
        if a.size != 1:
            raise ValueError(f"Vec.set takes a scalar, got an array of size {a.size}; use setFuncArray")
        self._fn.version += 1
        self._fn.vec.fill(float(a.ravel()[0]))

    def __setitem__(self, key, value) -> None:
        if key != slice(None):
            raise NotImplementedError("only v.vector[:] = array is supported")
        arr = np.asarray(value, dtype=np.float64)
        self._fn.version += 1
        if arr.ndim == 0:
            self._fn.vec.fill(float(arr))
        else:
            self._fn.vec.set(arr)

    # no-ops kept so reference call sequences read the same (utils_dolfinx.py:166-167)
    def assemble(self) -> None:
        pass

    def ghostUpdate(self, *a, **k) -> None:
        """Ghost entries <- the owners' values on a partitioned mesh (PETSc ``Vec.ghostUpdate`` [ext]); a no-op on one rank, for
        cell-wise (DG0) functions, and when nothing has written the vector since its last refresh (femo_halo_exchange)."""
        fs = self._fn.function_space
        mesh = fs.mesh
        local = getattr(mesh, "local", None)
        dm = getattr(mesh, "_device", None)
        if local is None or local.nranks <= 1 or dm is None or fs.family != "CG" or len(local.nbr) == 0:
            return
        if self._fn.vec.n >= dm.n_vert:
            dm.halo_exchange(self._fn.vec)


class _XView:
    def __init__(self, fn):
        self._fn = fn

    @property
    def array(self):
        return _ArrayProxy(self._fn)


class _ArrayProxy:
    def __init__(self, fn):
        self._fn = fn

    def __setitem__(self, key, value):
        self._fn.vector[key] = value

    def __array__(self, dtype=None, copy=None):
        return self._fn.vector.getArray()


class Function:
    def __init__(self, function_space: FunctionSpace, name: str = "f"):
        from .utils_hip import get_context
        self.function_space = function_space
        self.name = name
        self.vec = Vec(get_context(), function_space.dim)
        self.version = 0          # bumped by every host-side write (cache key for Dirichlet values)
        self.vector = _VectorView(self)
        self.x = _XView(self)

    def interpolate(self, fn) -> None:
        """fn receives coordinates shaped (3, n_dofs) like dolfinx [ext] (fea_dolfinx.py:163-167)."""
        x = self.function_space.tabulate_dof_coordinates()
        xt = np.zeros((3, x.shape[0]))
        xt[:x.shape[1]] = x.T
        self.version += 1
        self.vec.set(np.asarray(fn(xt), dtype=np.float64))

    def rename(self, name, label=None) -> None:
        self.name = name
