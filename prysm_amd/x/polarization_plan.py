"""What prysm_amd/x/polarization.py and csrc/jones.hip share, without a device: the records of the five entry points, the layout
logic, and the numpy model of every kernel -- the same products and sums in the same order and the same type, so that a test can
tell a wrong kernel from a rounding.

Layouts.  A Jones field has four complex components per pixel in the order (0,0), (0,1), (1,0), (1,1), a Jones vector two, (0,0),
(1,0).  'aos' is the reference's (..., 2, 2) / (..., 2, 1); 'planes' is (4, ...) / (2, ...), the stack propagation.focus and its
siblings take.  The leading dimensions of the pixel grid flatten to rows, the last one is cols.

The model writes a complex product as its four real products and two sums (numpy's own complex product may or may not fuse), works
in the dtype it is given, and takes the cosine and sine of a host scalar in double before rounding once, of a map in the map's type,
as the kernels do.
"""
import math

import numpy as np

AOS, PLANES = 0, 1
LAYOUTS = {'aos': AOS, 'planes': PLANES}
ROTATION, RETARDER, DIATTENUATOR, VORTEX, LINPOL_VECTOR = range(5)
FIELD_NONE, FIELD_REAL, FIELD_COMPLEX = 0, 1, 2
LEAKAGE_IDENTITY = 1
MAX_CHAIN = 6
NPARAM = {ROTATION: 1, RETARDER: 2, DIATTENUATOR: 2, VORTEX: 3, LINPOL_VECTOR: 1}

PAULI = (((1, 0), (0, 1)), ((1, 0), (0, -1)), ((0, 1), (1, 0)), ((0, -1j), (1j, 0)))


def layout_code(layout):
    try:
        return LAYOUTS[layout]
    except (KeyError, TypeError):
        raise ValueError(f"layout must be 'aos' or 'planes', got {layout!r}") from None


def tail_of(ncomp):
    """the trailing dimensions of an aos array of ncomp components per pixel"""
    return {4: (2, 2), 2: (2, 1), 16: (4, 4)}[ncomp]


def ncomp_of(shape, layout):
    """components per pixel (4 a matrix, 2 a vector) and the pixel grid of a Jones array of this shape"""
    shape = tuple(shape)
    if layout == AOS:
        if len(shape) >= 2 and shape[-2:] == (2, 2):
            return 4, shape[:-2]
        if len(shape) >= 2 and shape[-2:] == (2, 1):
            return 2, shape[:-2]
        raise ValueError(f'an aos Jones array ends in (2, 2) or (2, 1), got shape {shape}')
    if len(shape) >= 2 and shape[0] in (4, 2):
        return shape[0], shape[1:]
    raise ValueError(f'a planes Jones array starts with 4 or 2 planes, got shape {shape}')


def rows_cols(pix):
    """the leading dimensions flatten to rows, the last one is cols"""
    pix = tuple(int(n) for n in pix)
    if not pix:
        return 1, 1
    return int(np.prod(pix[:-1], dtype=np.int64)), pix[-1]


def window(pix, strides, unit):
    """(rows, cols, ld) of a pixel grid whose dimensions lie `strides` elements apart, ld in units of `unit` elements (the components
    per pixel of an aos array, 1 for a plane); None where the kernels cannot address it (the caller copies, or refuses an output)"""
    pix, strides = tuple(pix), tuple(strides)
    rows, cols = rows_cols(pix)
    if rows * cols == 0:
        return rows, cols, max(cols, 1)
    if not pix:
        return 1, 1, 1
    if cols > 1 and strides[-1] != unit:
        return None
    lead = [(n, s) for n, s in zip(pix[:-1], strides[:-1]) if n > 1]
    if not lead:
        return rows, cols, cols
    for (_, s0), (n1, s1) in zip(lead[:-1], lead[1:]):
        if s0 != s1 * n1:
            return None
    s = lead[-1][1]
    if s % unit or s // unit < cols:
        return None
    return rows, cols, s // unit


# ---------------------------------------------------------------- the model
def to_planes(a):
    """aos (..., 2, 2) / (..., 2, 1) / (..., 4, 4) -> planes"""
    a = np.asarray(a)
    n = a.shape[-2] * a.shape[-1]
    pix = a.shape[:-2]
    return np.ascontiguousarray(np.moveaxis(a.reshape(*pix, n), -1, 0))


def from_planes(p):
    """planes (4, ...) / (2, ...) / (16, ...) -> aos"""
    p = np.asarray(p)
    return np.ascontiguousarray(np.moveaxis(p, 0, -1)).reshape(*p.shape[1:], *tail_of(p.shape[0]))


def _cx(re, im, cdt):
    out = np.empty(np.broadcast(re, im).shape, dtype=cdt)
    out.real, out.imag = re, im
    return out


def _cmul(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return _cx(a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real, np.result_type(a, b))


def _cs(p, mul, rdt):
    """cos and sin of parameter p times mul: a map in its own type, a scalar in double and rounded once"""
    if isinstance(p, np.ndarray) and p.ndim:
        v = p.astype(rdt, copy=False) * rdt(mul)
        return np.cos(v), np.sin(v)
    v = float(p) * float(mul)
    return rdt(math.cos(v)), rdt(math.sin(v))


def optic(kind, params, shape, cdtype, charge=1.0, leak=False, field=None):
    """pm_jones_optic: the aos array (*shape, 2, 2), or (*shape, 2, 1) for LINPOL_VECTOR"""
    cdt = np.dtype(cdtype)
    rdt = np.float32 if cdt == np.complex64 else np.float64
    shape = tuple(shape)
    zero, one = rdt(0), rdt(1)
    full = lambda v: np.broadcast_to(np.asarray(v, dtype=rdt), shape)      # noqa: E731
    p = list(params) + [0.0] * (3 - len(params))
    if kind in (ROTATION, LINPOL_VECTOR):
        co, si = _cs(p[0], charge if kind == LINPOL_VECTOR else 1.0, rdt)
        comps = [(co, zero), (si, zero)] if kind == LINPOL_VECTOR else [(co, zero), (si, zero), (-si, zero), (co, zero)]
    elif kind in (RETARDER, DIATTENUATOR):
        if kind == RETARDER:
            pr, pi = _cs(p[0], 1.0, rdt)
        else:
            pr, pi = (p[0].astype(rdt, copy=False) if isinstance(p[0], np.ndarray) and p[0].ndim else rdt(p[0])), zero
        co, si = _cs(p[1], 1.0, rdt)
        c2, s2, sc = co * co, si * si, co * si
        off = (sc * (one - pr), -(sc * pi))
        comps = [(c2 + s2 * pr, s2 * pi), off, off, (s2 + c2 * pr, c2 * pi)]
    elif kind == VORTEX:
        ct, st = _cs(p[0], charge, rdt)
        cr, sr = _cs(p[1], 0.5, rdt)
        co, si = _cs(p[2], 1.0, rdt)
        a = (sr * ct, -cr)
        b = (sr * st, zero)
        d = (-(sr * ct), -cr if leak else zero)
        sub = lambda u, ku, v, kv: (u[0] * ku - v[0] * kv, u[1] * ku - v[1] * kv)      # noqa: E731
        add = lambda u, ku, v, kv: (u[0] * ku + v[0] * kv, u[1] * ku + v[1] * kv)      # noqa: E731
        x00, x01 = sub(a, co, b, si), sub(b, co, d, si)
        x10, x11 = add(a, si, b, co), add(b, si, d, co)
        comps = [sub(x00, co, x01, si), add(x00, si, x01, co), sub(x10, co, x11, si), add(x10, si, x11, co)]
    else:
        raise ValueError(f'unknown kind {kind}')
    out = np.empty((*shape, len(comps)), dtype=cdt)
    for k, (re, im) in enumerate(comps):
        e = _cx(full(re), full(im), cdt)
        out[..., k] = _cmul(e, np.asarray(field, dtype=cdt)) if field is not None else e
    return out.reshape(*shape, *tail_of(len(comps)))


def chain(operands, vector_tail=False):
    """pm_jones_chain on aos operands ((..., 2, 2) maps or (2, 2) constants; the last one (..., 2, 1) with vector_tail), from the left"""
    if not 1 <= len(operands) <= MAX_CHAIN:
        raise ValueError(f'between 1 and {MAX_CHAIN} operands are taken, got {len(operands)}')
    ops = [np.asarray(o) for o in operands]
    pix = np.broadcast_shapes(*[o.shape[:-2] for o in ops])
    nmat = len(ops) - 1 if vector_tail else len(ops)
    comp = lambda o, i, j: np.broadcast_to(o[..., i, j], pix)      # noqa: E731
    acc = None
    if nmat:
        acc = [[comp(ops[0], i, j) for j in (0, 1)] for i in (0, 1)]
        for o in ops[1:nmat]:
            b = [[comp(o, i, j) for j in (0, 1)] for i in (0, 1)]
            acc = [[_cmul(acc[i][0], b[0][j]) + _cmul(acc[i][1], b[1][j]) for j in (0, 1)] for i in (0, 1)]
    if vector_tail:
        v = [comp(ops[-1], i, 0) for i in (0, 1)]
        if acc is not None:
            v = [_cmul(acc[i][0], v[0]) + _cmul(acc[i][1], v[1]) for i in (0, 1)]
        out = np.empty((*pix, 2, 1), dtype=ops[-1].dtype)
        out[..., 0, 0], out[..., 1, 0] = v
        return out
    out = np.empty((*pix, 2, 2), dtype=ops[0].dtype)
    for i in (0, 1):
        for j in (0, 1):
            out[..., i, j] = acc[i][j]
    return out


def scale(jones, field=None):
    """pm_jones_scale on an aos array: field x J, the field complex, real or None"""
    jones = np.asarray(jones)
    if field is None:
        return jones.copy()
    f = np.asarray(field)[..., None, None]
    if np.iscomplexobj(f):
        return _cmul(jones, f.astype(jones.dtype, copy=False)).astype(jones.dtype, copy=False)
    f = f.astype(jones.real.dtype, copy=False)
    return _cx(jones.real * f, jones.imag * f, jones.dtype)


def mueller(jones):
    """pm_jones_to_mueller on an aos array (..., 2, 2): the real (..., 4, 4) of Re(U (J* (x) J) U^H)"""
    jones = np.asarray(jones)
    a, b, c, d = jones[..., 0, 0], jones[..., 0, 1], jones[..., 1, 0], jones[..., 1, 1]
    rec = lambda x, y: x.real * y.real + x.imag * y.imag      # noqa: E731  Re(x* y)
    imc = lambda x, y: x.real * y.imag - x.imag * y.real      # noqa: E731  Im(x* y)
    h = jones.real.dtype.type(0.5)
    na, nb, nc, nd = rec(a, a), rec(b, b), rec(c, c), rec(d, d)
    m = [h * ((na + nb) + (nc + nd)), h * ((na - nb) + (nc - nd)), rec(a, b) + rec(c, d), imc(a, b) + imc(c, d),
         h * ((na + nb) - (nc + nd)), h * ((na - nb) - (nc - nd)), rec(a, b) - rec(c, d), imc(a, b) - imc(c, d),
         rec(a, c) + rec(b, d), rec(a, c) - rec(b, d), rec(a, d) + rec(b, c), imc(a, d) - imc(b, c),
         -(imc(a, c) + imc(b, d)), -(imc(a, c) - imc(b, d)), -(imc(a, d) + imc(b, c)), rec(a, d) - rec(b, c)]
    return np.stack(m, axis=-1).reshape(*jones.shape[:-2], 4, 4)


def pauli(jones):
    """pm_pauli_coefficients on an aos array: the planes (4, ...) of c0 ... c3"""
    jones = np.asarray(jones)
    a, b, c, d = jones[..., 0, 0], jones[..., 0, 1], jones[..., 1, 0], jones[..., 1, 1]
    h = jones.real.dtype.type(0.5)
    df = b - c
    zero, one = h * 0, h * 2
    j = _cx(zero * df.real - one * df.imag, zero * df.imag + one * df.real, jones.dtype)
    half = lambda z: _cx(z.real * h, z.imag * h, jones.dtype)      # noqa: E731
    return np.stack([half(a + d), half(a - d), half(b + c), half(j)], axis=0)
