"""Host-side planning of aperture geometry (numpy only: no torch, no library).

A shape is a tree of Node objects: the primitives of prysm/geometry.py (each a signed-distance function, negative inside) under union
(min), intersect (max) and subtract (max(d1, -d2)).  plan() flattens a tree into a table of fixed-size steps that the kernel
(csrc/geometry.hip pm_sdf_render) walks per pixel, and evaluate() is a numpy walk of the SAME table with the SAME order of
operations -- what the CPU tests pin to the reference fixture and what the GPU tests compare the kernel against.

The flattening needs no stack at run time.  A step computes (part of) one primitive: a whole circle, rectangle or ellipse, one edge
of a polygon, one vane of a spider; the primitive's last step (flag END) combines its value into one of MAX_SLOTS accumulators by
`comb` (set, min, max, max(acc, -value)).  A composite's first child is evaluated into the composite's own slot, every other leaf
child is combined into it directly, and a child that is itself a composite is evaluated into the next slot and brought back by a
MERGE step.  A tree that would need more than MAX_SLOTS slots is refused here, with a ValueError.

Polygon edges are steps of their own (start, edge vector, 1 / |edge|^2, end y), not an index range into a vertex list: a step is read
once for all pixels either way, and one record kind keeps kernel and walk short.  The per-edge division of the reference is the
multiplication by that reciprocal, here and in the kernel.
"""
import math

import numpy as np

MAX_SLOTS = 4

OP_NOP, OP_CIRCLE, OP_ANNULUS, OP_RCIRCLE, OP_RANNULUS, OP_RECT, OP_ELLIPSE, OP_EDGE, OP_VANE, OP_GAUSS, OP_MERGE = range(11)
CB_SET, CB_MIN, CB_MAX, CB_MAXNEG = range(4)
FL_BEGIN, FL_END, FL_ROT, FL_UP = 1, 2, 4, 8

_COMPOSITES = ('union', 'intersect', 'subtract')
_COMB_OF = {'union': CB_MIN, 'intersect': CB_MAX, 'subtract': CB_MAXNEG}


def step_dtype(dtype):
    """the record of one step: struct pm::GStep in csrc/geometry.hip (48 bytes in float32, 80 in float64)"""
    return np.dtype([('op', np.int32), ('comb', np.int32), ('slot', np.int32), ('flags', np.int32), ('f', np.dtype(dtype), (8,))])


class Node:
    """One shape of a tree: `kind`, its parameters (a tuple of Python numbers / tuples, hashable) and, for composites, its children."""
    __slots__ = ('kind', 'params', 'children')

    def __init__(self, kind, params=(), children=()):
        self.kind, self.params, self.children = kind, tuple(params), tuple(children)

    @property
    def key(self):
        """a hashable value that identifies the program: what device tables are cached by"""
        return (self.kind, self.params, tuple(c.key for c in self.children))

    def __hash__(self):
        return hash(self.key)

    def __eq__(self, other):
        return isinstance(other, Node) and self.key == other.key

    def __repr__(self):
        inner = ', '.join([repr(p) for p in self.params] + [repr(c) for c in self.children])
        return f'{self.kind}({inner})'

    def union(self, *others):
        return union(self, *others)

    def intersect(self, *others):
        return intersect(self, *others)

    def subtract(self, other):
        return subtract(self, other)


def _num(v, what):
    if isinstance(v, complex) or (hasattr(v, 'dtype') and np.issubdtype(np.asarray(v).dtype, np.complexfloating)):
        raise TypeError(f'{what} must be real')
    return float(v)


def _pt(c, what='center'):
    c = tuple(c)
    if len(c) != 2:
        raise ValueError(f'{what} must be (x, y)')
    return (_num(c[0], what), _num(c[1], what))


def _nodes(nodes, least):
    if len(nodes) < least or not all(isinstance(n, Node) for n in nodes):
        raise TypeError(f'expected at least {least} shape node(s)')
    for n in nodes:
        if n.kind == 'gaussian':
            raise ValueError('a gaussian is not a distance: it cannot be combined with shapes')
    return nodes


# ---------------------------------------------------------------- node constructors (geometry.shape)
def circle(radius, center=(0, 0)):
    """hypot(x - x0, y - y0) - radius (circle_sdf on the radial coordinate about `center`; offset_circle)"""
    return Node('circle', (_num(radius, 'radius'), _pt(center)))


def offset_circle(radius, center):
    return circle(radius, center)


def annulus(rin, rout, center=(0, 0)):
    return Node('annulus', (_num(rin, 'rin'), _num(rout, 'rout'), _pt(center)))


def radial_circle(radius):
    """r - radius with r taken from the x coordinate as it is (circle_sdf(radius, r))"""
    return Node('rcircle', (_num(radius, 'radius'),))


def radial_annulus(rin, rout):
    return Node('rannulus', (_num(rin, 'rin'), _num(rout, 'rout')))


def rectangle(width, height=None, angle=0):
    """rectangle_sdf: half-width, half-height (None: a square), angle in degrees -- 90 swaps x and y, any other angle rotates the
    coordinates by +angle"""
    width = _num(width, 'width')
    height = width if height is None else _num(height, 'height')
    return Node('rectangle', (width, height, _num(angle, 'angle')))


def rectangle_with_corner_fillets(width, height, cradius, center=(0, 0), rotation=0):
    """rectangle_with_corner_fillets_sdf: the coordinates are rotated about the grid origin BEFORE the centre is subtracted"""
    return Node('fillet', (_num(width, 'width'), _num(height, 'height'), _num(cradius, 'cradius'), _pt(center), _num(rotation, 'rotation')))


def rotated_ellipse(width_major, width_minor, major_axis_angle=0):
    a, b = _num(width_major, 'width_major'), _num(width_minor, 'width_minor')
    if b > a:
        raise ValueError('By definition, major axis must be larger than minor.')
    return Node('ellipse', (a, b, _num(major_axis_angle, 'major_axis_angle')))


def polygon(vertices):
    """polygon_sdf: N x 2 vertices, either winding, no repeated closing vertex, concave allowed"""
    v = np.asarray(vertices)
    if np.issubdtype(v.dtype, np.complexfloating):
        raise TypeError('polygon vertices must be real')
    if v.ndim != 2 or v.shape[1] != 2:
        raise ValueError(f'vertices must be N x 2, got {v.shape}')
    if v.shape[0] < 3:
        raise ValueError(f'a polygon needs at least 3 vertices, got {v.shape[0]}')
    return Node('polygon', (tuple((float(a), float(b)) for a, b in v),))


def generate_vertices(sides, radius=1, center=(0, 0), rotation=0, dtype=np.float64):
    """the reference's _generate_vertices (geometry.py:521-547): x = R sin(k 2 pi / sides + rot) + x0, y = R cos(...) + y0, the index
    k held in `dtype` (config.precision)"""
    angle = 2 * np.pi / sides
    rotation = np.radians(rotation)
    x0, y0 = center
    points = np.arange(sides, dtype=dtype)
    x = radius * np.sin(points * angle + rotation) + x0
    y = radius * np.cos(points * angle + rotation) + y0
    return np.stack((x, y), axis=1)


def regular_polygon(sides, radius, center=(0, 0), rotation=0, dtype=np.float64):
    sides = int(sides)
    if sides < 3:
        raise ValueError(f'a polygon needs at least 3 vertices, got {sides}')
    return polygon(generate_vertices(sides, _num(radius, 'radius'), _pt(center), _num(rotation, 'rotation'), dtype))


def spider(vanes, width, rotation=0, center=(0, 0), rotation_is_rad=False):
    vanes = int(vanes)
    if vanes < 1:
        raise ValueError('a spider needs at least one vane')
    return Node('spider', (vanes, _num(width, 'width'), _num(rotation, 'rotation'), _pt(center), bool(rotation_is_rad)))


def gaussian(sigma, center=(0, 0)):
    """exp(-4 ln 2 ((x - x0)^2 + (y - y0)^2) / sigma^2): a value, not a distance -- only alone, only with output 'sdf'"""
    return Node('gaussian', (_num(sigma, 'sigma'), _pt(center)))


def union(*nodes):
    return Node('union', (), _nodes(nodes, 1))


def intersect(*nodes):
    return Node('intersect', (), _nodes(nodes, 1))


def subtract(a, b):
    return Node('subtract', (), _nodes((a, b), 2))


# ---------------------------------------------------------------- flattening
def depth(node):
    """accumulator slots the tree needs"""
    if node.kind not in _COMPOSITES:
        return 1
    need = depth(node.children[0])
    for c in node.children[1:]:
        if c.kind in _COMPOSITES:
            need = max(need, 1 + depth(c))
    return need


def _leaf_steps(node, comb, slot):
    """the steps of one primitive: (op, comb, slot, flags, f[8]) tuples, floats still in Python precision"""
    k, p = node.kind, node.params
    z = [0.0] * 8

    def one(op, flags, *f):
        return [(op, comb, slot, flags | FL_BEGIN | FL_END, list(f) + z[len(f):])]

    if k == 'circle':
        return one(OP_CIRCLE, 0, p[1][0], p[1][1], p[0])
    if k == 'annulus':
        return one(OP_ANNULUS, 0, p[2][0], p[2][1], (p[0] + p[1]) / 2, (p[1] - p[0]) / 2)
    if k == 'rcircle':
        return one(OP_RCIRCLE, 0, 0.0, 0.0, p[0])
    if k == 'rannulus':
        return one(OP_RANNULUS, 0, 0.0, 0.0, (p[0] + p[1]) / 2, (p[1] - p[0]) / 2)
    if k == 'rectangle':
        w, h, ang = p
        if ang == 0:
            return one(OP_RECT, 0, 1.0, 0.0, 0.0, 0.0, w, h, 0.0)
        if ang == 90:       # x and y swapped: the half-width bounds y
            return one(OP_RECT, 0, 1.0, 0.0, 0.0, 0.0, h, w, 0.0)
        a = math.radians(ang)
        return one(OP_RECT, FL_ROT, math.cos(a), math.sin(a), 0.0, 0.0, w, h, 0.0)
    if k == 'fillet':
        w, h, cr, c, rot = p
        a = math.radians(rot)
        return one(OP_RECT, FL_ROT if rot != 0 else 0, math.cos(a), math.sin(a), c[0], c[1], w - cr, h - cr, cr)
    if k == 'ellipse':
        a, b, ang = p
        A = math.radians(-ang)
        return one(OP_ELLIPSE, 0, math.cos(A), math.sin(A), a, b, a * a, b * b)
    if k == 'gaussian':
        s, c = p
        return one(OP_GAUSS, 0, c[0], c[1], -4 * math.log(2), s ** 2)
    if k == 'polygon':
        v = p[0]
        n = len(v)
        steps = []
        for i in range(n):
            (x0, y0), (x1, y1) = v[i], v[(i + 1) % n]
            ex, ey = x1 - x0, y1 - y0
            fl = (FL_BEGIN if i == 0 else 0) | (FL_END if i == n - 1 else 0) | (FL_UP if y1 > y0 else 0)
            steps.append((OP_EDGE, comb, slot, fl, [x0, y0, ex, ey, 1.0 / (ex * ex + ey * ey), y1, 0.0, 0.0]))
        return steps
    if k == 'spider':
        vanes, width, rot, c, is_rad = p
        if not is_rad:
            rot = math.radians(rot)
        step = 2 * math.pi / vanes
        steps = []
        for m in range(vanes):
            ang = step * m - rot
            fl = (FL_BEGIN if m == 0 else 0) | (FL_END if m == vanes - 1 else 0)
            steps.append((OP_VANE, comb, slot, fl, [math.cos(ang), math.sin(ang), c[0], c[1], width / 2, 0.0, 0.0, 0.0]))
        return steps
    raise ValueError(f'unknown shape {k!r}')


def _flatten(node, comb, slot, steps):
    if slot >= MAX_SLOTS:
        raise ValueError(f'the shape tree nests composites deeper than the {MAX_SLOTS} accumulators of the kernel')
    if node.kind not in _COMPOSITES:
        steps.extend(_leaf_steps(node, comb, slot))
        return
    inner = _COMB_OF[node.kind]
    if comb == CB_SET:
        # the composite's own result goes to `slot`: its first child is evaluated there, the others combined into it
        _flatten(node.children[0], CB_SET, slot, steps)
        for c in node.children[1:]:
            if c.kind in _COMPOSITES:
                _flatten(c, CB_SET, slot + 1, steps)
                if slot + 1 >= MAX_SLOTS:
                    raise ValueError(f'the shape tree nests composites deeper than the {MAX_SLOTS} accumulators of the kernel')
                steps.append((OP_MERGE, inner, slot, FL_BEGIN | FL_END, [0.0] * 8))
            else:
                _flatten(c, inner, slot, steps)
    else:
        raise AssertionError('composites are entered with CB_SET only')


def plan(programs, dtype):
    """The step table of one Node or of a sequence of them (a stack): a structured array of shape (B, nsteps) in step_dtype(dtype),
    shorter programs padded with NOP steps.  Scalars are rounded once to `dtype`."""
    if isinstance(programs, Node):
        programs = (programs,)
    programs = tuple(programs)
    if not programs or not all(isinstance(p, Node) for p in programs):
        raise TypeError('plan() takes a shape node or a non-empty sequence of them')
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError('step tables are float32 or float64')
    rows = []
    for p in programs:
        steps = []
        _flatten(p, CB_SET, 0, steps)
        rows.append(steps)
    n = max(len(r) for r in rows)
    tab = np.zeros((len(rows), n), dtype=step_dtype(dtype))
    for b, r in enumerate(rows):
        for s, (op, comb, slot, flags, f) in enumerate(r):
            tab[b, s] = (op, comb, slot, flags, np.asarray(f, dtype=np.float64).astype(dtype))
    return tab


# ---------------------------------------------------------------- the numpy walk
def evaluate(table, x, y):
    """Walk ONE program (a 1-D table of steps) at the points (x, y) -- any shapes that broadcast -- in the table's precision, with the
    kernel's order of operations.  Returns accumulator 0: the signed distance (or the gaussian's value)."""
    table = np.asarray(table)
    if table.ndim != 1:
        raise ValueError('evaluate() walks one program: give table[b] of a stack')
    T = table.dtype['f'].base.type
    x, y = np.asarray(x, dtype=T), np.asarray(y, dtype=T)
    shape = np.broadcast_shapes(x.shape, y.shape)
    acc = [np.zeros(shape, dtype=T) for _ in range(MAX_SLOTS)]
    run = par = None
    zero, one = T(0), T(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        for st in table:
            op, comb, slot, flags = int(st['op']), int(st['comb']), int(st['slot']), int(st['flags'])
            f = st['f']
            begin = bool(flags & FL_BEGIN)
            if op == OP_NOP:
                continue
            if op in (OP_CIRCLE, OP_ANNULUS):
                xx, yy = x - f[0], y - f[1]
                p = np.sqrt(xx * xx + yy * yy) - f[2]
                if op == OP_ANNULUS:
                    p = np.abs(p) - f[3]
            elif op in (OP_RCIRCLE, OP_RANNULUS):
                p = x - f[2]
                if op == OP_RANNULUS:
                    p = np.abs(p) - f[3]
            elif op == OP_RECT:
                xx, yy = x, y
                if flags & FL_ROT:
                    xx, yy = x * f[0] - y * f[1], x * f[1] + y * f[0]
                qx, qy = np.abs(xx - f[2]) - f[4], np.abs(yy - f[3]) - f[5]
                ox, oy = np.maximum(qx, zero), np.maximum(qy, zero)
                p = np.sqrt(ox * ox + oy * oy) + np.minimum(np.maximum(qx, qy), zero) - f[6]
            elif op == OP_ELLIPSE:
                xr, yr = x * f[0] + y * f[1], x * f[1] - y * f[0]
                u, v = xr / f[2], yr / f[3]
                F = u * u + v * v - one
                gx, gy = T(2) * xr / f[4], T(2) * yr / f[5]
                p = F / np.maximum(np.sqrt(gx * gx + gy * gy), T(1e-15))
            elif op == OP_EDGE:
                x0, y0, ex, ey, rinv, y1 = f[:6]
                up = bool(flags & FL_UP)
                wx, wy = x - x0, y - y0
                t = (wx * ex + wy * ey) * rinv
                t = np.minimum(np.maximum(t, zero), one)
                px, py = wx - t * ex, wy - t * ey
                seg = px * px + py * py
                crosses = ((y0 > y) != (y1 > y)) & ((wx * ey < ex * wy) == up)
                run = seg if begin else np.minimum(run, seg)
                par = crosses if begin else par ^ crosses
                if flags & FL_END:
                    d = np.sqrt(run)
                    p = np.where(par, -d, d)
            elif op == OP_VANE:
                xx, yy = x - f[2], y - f[3]
                al, ac = np.minimum(xx * f[0] - yy * f[1], zero), xx * f[1] + yy * f[0]
                vane = np.sqrt(al * al + ac * ac) - f[4]
                run = vane if begin else np.minimum(run, vane)
                p = run
            elif op == OP_GAUSS:
                xx, yy = x - f[0], y - f[1]
                p = np.exp(f[2] * (xx * xx + yy * yy) / f[3])
            elif op == OP_MERGE:
                p = acc[slot + 1]
            else:
                raise ValueError(f'unknown opcode {op}')
            if not flags & FL_END:
                continue
            p = np.broadcast_to(p, shape)
            if comb == CB_SET:
                acc[slot] = p
            elif comb == CB_MIN:
                acc[slot] = np.minimum(acc[slot], p)
            elif comb == CB_MAX:
                acc[slot] = np.maximum(acc[slot], p)
            else:
                acc[slot] = np.maximum(acc[slot], -p)
    return np.array(acc[0], dtype=T)


def coverage(d, dx):
    """antialias (geometry.py:11-34): the one-pixel ramp min(max(0.5 - d / dx, 0), 1) in d's precision"""
    d = np.asarray(d)
    T = d.dtype.type
    return np.minimum(np.maximum(T(0.5) - d / T(dx), T(0)), T(1))


def grid_axis(n, dx, dtype):
    """fftrange(n, dtype) * dx (fttools.py:13-15, coordinates.py:373): the index j - n // 2 in `dtype`, times dx rounded once to it"""
    T = np.dtype(dtype).type
    return np.arange(-(n // 2), -(n // 2) + n, dtype=T) * T(dx)


def grid_spacing(shape, dx=0, diameter=0):
    """((ny, nx), dx) of make_xy_grid's arguments: a scalar shape is square, a diameter overrides dx (dx = diameter / max(shape))"""
    if not isinstance(shape, tuple):
        shape = (shape, shape)
    if len(shape) != 2:
        raise ValueError(f'shape must be (rows, cols), got {shape}')
    ny, nx = int(shape[0]), int(shape[1])
    if ny < 0 or nx < 0:
        raise ValueError(f'shape must not be negative, got {shape}')
    if diameter != 0:
        dx = diameter / max(ny, nx)
    return (ny, nx), float(dx)
