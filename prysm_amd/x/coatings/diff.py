"""Forward evaluations and the thickness gradient (prysm/x/coatings/diff.py) on pm_tf_stack and pm_tf_thickness_grad.

A ForwardEval evaluates r, t, R and T in one launch when it is made; the boundary fields and the absorptance come from a second
launch the first time one of E, H, A_value or Esq_value is asked for.  It keeps no matrices: thickness_gradient hands the
evaluation's operands to the gradient kernel, which sweeps the stack from the substrate (the unnormalised boundary vectors go to
its workspace) and scans the cotangent from the ambient side.  Complex cotangents use dF = Re(conj(c_z) dz); the gradient is summed
over the samples in double, in a fixed order: two runs give the same bits.

Seeds of the absorptance and of the field intensity (dA, dEsq) and the gradient with respect to the indices are not built.
"""
from ... import _ops
from .stack import operands

__all__ = ['ForwardEval', 'forward_eval', 'thickness_gradient', 'index_gradient', 'char_matrix_vjp', 'assembly_cotangent', 'layer_cotangents']


class ForwardEval:
    """A forward evaluation of a stack over wvl x theta0 (diff.py:63-154).  pol is 's' or 'p'; 'both' (what the merit terms use
    for pol='avg') carries the two polarisations through one sweep and gives every quantity a leading axis of 2, s first."""

    __slots__ = ('stack', 'wvl', 'theta0', 'pol', 'op', 'shape', 'r', 't', '_R', '_T', '_more')

    def __init__(self, stack, wvl, theta0, pol, op=None, shape=None):
        pol = pol.lower()
        if pol not in ('p', 's', 'both'):
            raise ValueError("unknown polarization, use 'p' or 's'")
        self.stack, self.wvl, self.theta0, self.pol = stack, wvl, theta0, pol
        if op is None:
            op, shape = operands(stack, wvl, theta0)
        self.op, self.shape = op, tuple(shape)
        out = _ops.tf_stack(op, pol, want=('R', 'T'))
        self.r, self.t, self._R, self._T = (self._shaped(out[k]) for k in ('r', 't', 'R', 'T'))
        self._more = None

    def _shaped(self, a, lead=()):
        a = a if self.pol == 'both' else a[0]
        return a.reshape(((2,) if self.pol == 'both' else ()) + tuple(lead) + self.shape)

    def _fields(self):
        if self._more is None:
            out = _ops.tf_stack(self.op, self.pol, want=('fields', 'A'))
            L = self.op.L
            self._more = (self._shaped(out['E'], (L + 1,)), self._shaped(out['H'], (L + 1,)), self._shaped(out['A'], (L,)))
        return self._more

    @property
    def E(self):
        """Tangential electric field at every boundary, the boundary axis first."""
        return self._fields()[0]

    @property
    def H(self):
        """Tangential magnetic field at every boundary."""
        return self._fields()[1]

    @property
    def R_value(self):
        """Reflectance abs(r)^2."""
        return self._R

    @property
    def T_value(self):
        """Transmittance with the tilted-admittance flux factor."""
        return self._T

    @property
    def A_value(self):
        """Per-layer absorptance, (N, calc)."""
        return self._fields()[2]

    @property
    def Esq_value(self):
        """Standing-wave intensity abs(E)^2 at each boundary, (N + 1, calc)."""
        E = self.E
        return E.real * E.real + E.imag * E.imag


def forward_eval(stack, wvl, theta0, pol):
    """Build a ForwardEval for one sample set (diff.py:157-159)."""
    return ForwardEval(stack, wvl, theta0, pol)


def thickness_gradient(fwd, dR=None, dT=None, dA=None, dEsq=None, out=None):
    """Gradient of a scalar merit with respect to every layer thickness (diff.py:294-308): an (N,) device tensor from the seeds
    dR = dF/dR and dT = dF/dT over the evaluation's samples.  `out`, when given, is added to (the s and p parts of one merit)."""
    if dA is not None or dEsq is not None:
        raise NotImplementedError('thickness_gradient: the dA and dEsq seeds are not implemented (dR and dT are)')
    return _ops.tf_thickness_grad(fwd.op, fwd.pol, dR, dT, grad=out)


def index_gradient(fwd, dR=None, dT=None, dA=None, dEsq=None):
    """Not built: the gradient with respect to the layer indices (diff.py:311-340)."""
    raise NotImplementedError('prysm_amd.x.coatings.index_gradient is not implemented')


def _missing(name):
    def missing(*args, **kwargs):
        raise NotImplementedError(f'prysm_amd.x.coatings.diff.{name} is not implemented: the gradient kernel keeps no matrix cotangents')
    missing.__name__ = name
    return missing


char_matrix_vjp = _missing('char_matrix_vjp')
assembly_cotangent = _missing('assembly_cotangent')
layer_cotangents = _missing('layer_cotangents')
