"""The density filter of the SIMP example as a CSDL model (examples/beam_topo_opt/pre_processor/general_filter_model.py).

``GeneralFilterModel`` / ``GeneralFilterOperation`` keep the reference's parameters (``nel``, ``beta = 2.``,
``coordinates``, ``h_avg``) and variables (``density_unfiltered`` -> ``density``):

    density = W density_unfiltered,   W_ij = (r - d_ij) / sum_k (r - d_ik)  over d_ij <= r,  r = beta h_avg

W and W^T are built once on the device (csrc/elasticity.hip: hash grid, count / scan / fill); ``compute`` and both
Jacobian-vector products are gathers on the GPU.  Values may be NumPy arrays or ``DeviceArray``.  With the real
``csdl`` the sparse partials (rows, cols, val) are declared as a CSDL backend expects, exported once from the device.
"""
import numpy as np

from femo_amd import engine as E
from femo_amd.csdl_opt._csdl_compat import HAVE_CSDL, CustomExplicitOperation, Model, custom
from femo_amd.engine import DeviceArray, Vec
from femo_amd.fea.elasticity import DeviceFilter
from femo_amd.fea.utils_hip import get_context

_FILTER_PARAMS = (('nel', {}), ('beta', dict(default=2.)), ('coordinates', {}), ('h_avg', {}))


class GeneralFilterModel(Model):
    """Declares ``density_unfiltered`` and registers ``density`` as the output of a GeneralFilterOperation."""

    def initialize(self):
        for name, kw in _FILTER_PARAMS:
            self.parameters.declare(name, **kw)

    def define(self):
        P = self.parameters
        nel = P['nel']
        density_unfiltered = self.declare_variable('density_unfiltered', shape=(nel,), val=1.0)
        op = GeneralFilterOperation(nel=nel, beta=P['beta'], coordinates=P['coordinates'], h_avg=P['h_avg'])
        self.register_output('density', custom(density_unfiltered, op=op))


class GeneralFilterOperation(CustomExplicitOperation):
    """input: unfiltered density (DG0), output: filtered density."""

    def initialize(self):
        for name, kw in _FILTER_PARAMS:
            self.parameters.declare(name, **kw)

    def define(self):
        P = self.parameters
        self.nel = int(P['nel'])
        coords = np.asarray(P['coordinates'], dtype=np.float64)
        if coords.shape[0] != self.nel:
            raise ValueError(f"GeneralFilterOperation: {coords.shape[0]} coordinates for nel = {self.nel}")
        if coords.shape[1] == 3 and np.all(coords[:, 2] == 0.0):
            coords = coords[:, :2]                     # dolfinx tabulates 3 coordinates for a 2-D mesh
        self.radius = float(P['beta']) * float(P['h_avg'])
        self.add_input('density_unfiltered', shape=(self.nel,), val=0.0)
        self.add_output('density', shape=(self.nel,))
        self.filter = DeviceFilter(get_context(), coords, self.radius)
        self._x = self._y = None
        if HAVE_CSDL:
            rowptr, cols, val = self.filter.export_csr()
            rows = np.repeat(np.arange(self.nel), np.diff(rowptr))
            self.declare_derivatives('density', 'density_unfiltered', rows=rows, cols=cols, val=val)
        else:
            self.declare_derivatives('density', 'density_unfiltered')

    # -- helpers -----------------------------------------------------------------------------
    def _vec_in(self, value) -> Vec:
        if isinstance(value, DeviceArray):
            return value.vec
        if self._x is None:
            self._x = Vec(get_context(), self.nel)
        return self._x.set(np.ascontiguousarray(E.host_wait(np.asarray(value, dtype=np.float64))).ravel())

    def _product(self, value, transpose: bool) -> Vec:
        if self._y is None:
            self._y = Vec(get_context(), self.nel)
        return self.filter.apply(self._vec_in(value), self._y, transpose=transpose)

    @staticmethod
    def _add(target, y: Vec):
        """target += y with NumPy's in-place semantics (DeviceArray: on the device)."""
        if isinstance(target, DeviceArray):
            target.vec.axpy(1.0, y)
            return target
        if isinstance(target, np.ndarray) and target.dtype == np.float64 and target.flags.c_contiguous \
                and target.flags.writeable and target.size == y.n:
            y.add_to_host(target, y.n)
            return target
        return np.asarray(target, dtype=np.float64) + np.asarray(y.get())

    # -- protocol ----------------------------------------------------------------------------
    def compute(self, inputs, outputs):
        x = inputs['density_unfiltered']
        if isinstance(x, DeviceArray):
            out = Vec(get_context(), self.nel)
            self.filter.apply(x.vec, out)
            outputs['density'] = DeviceArray(out)
        else:
            outputs['density'] = self._product(x, False).get()

    def compute_jacvec_product(self, inputs, d_inputs, d_outputs, mode):
        """fwd: d_outputs[density] += W d_inputs[density_unfiltered];  rev: d_inputs[...] += W^T d_outputs[density]."""
        if mode == 'fwd':
            if 'density_unfiltered' in d_inputs and 'density' in d_outputs:
                d_outputs['density'] = self._add(d_outputs['density'], self._product(d_inputs['density_unfiltered'], False))
        elif mode == 'rev':
            if 'density_unfiltered' in d_inputs and 'density' in d_outputs:
                d_inputs['density_unfiltered'] = self._add(d_inputs['density_unfiltered'],
                                                           self._product(d_outputs['density'], True))
        else:
            raise ValueError(f"unknown mode {mode!r}")
