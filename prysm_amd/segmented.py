"""Segmented apertures (prysm/segmented.py) on the device: CompositeHexagonalAperture, its per-segment OPD and the adjoint.

    from prysm_amd.segmented import CompositeHexagonalAperture
    from prysm_amd.polynomials import zernike_nm_seq, noll_to_nm
    ap = CompositeHexagonalAperture(x, y, 2, 1.32, 0.007, exclude=(0,))
    ap.prepare_opd_bases(zernike_nm_seq, [noll_to_nm(j) for j in range(1, 12)])
    opd = ap.compose_opd(coefs)                  # coefs (S, K) or (B, S, K), read on the device when the kernel runs
    coefs_bar = ap.compose_opd_adjoint(opd_bar)  # (S, K) or (B, S, K)

The geometry (windows, local coordinates, antialiased hexagon masks, the amplitude) is one-off host work in numpy, as in the
reference; the device copies are made once, on first use.  prepare_opd_bases builds the segment plan (csrc/segmented.hip): one record
per segment (window, grid source, mask offset, centre, normalisation radius), the packed masks and the cover planes (for every pixel,
the segments whose window covers it with a non-zero mask, in segment order).  compose_opd is then one launch (pm_segment_compose) and
compose_opd_adjoint two (pm_segment_project).  With basis_func = polynomials.zernike_nm_seq no basis is stored: the kernels walk the
Zernike step table per point.  Any other basis_func is evaluated per unique grid, as in the reference, and kept on the device.

Grid sharing (share_grids=True, the reference's behaviour): prepare_opd_bases caches a segment's grid under the key
(local_x[0, 0], *local_x.shape), so segments in one window column use the local coordinates of the first segment with the same key,
even where their local y differ.  share_grids=False evaluates every segment on its own local grid.

Dropping cover entries whose mask is 0 changes results only where a basis value is not finite (0 * inf).  CompositeKeystoneAperture is
not provided: its x/y-basis path and geometry have quirks of their own and are left for later.
"""
import inspect
from collections import namedtuple
from collections.abc import Sequence

import numpy as np
import torch

from . import _lib as L
from .conf import config

__all__ = ['FLAT_TO_FLAT_TO_VERTEX_TO_VERTEX', 'VERTEX_TO_VERTEX_TO_FLAT_TO_FLAT', 'Hex', 'add_hex', 'sub_hex', 'mul_hex', 'hex_dir',
           'hex_neighbor', 'hex_to_xy', 'scale_hex', 'hex_ring', 'CompositeHexagonalAperture', 'SegmentPlan', 'evaluate_compose',
           'evaluate_project']

FLAT_TO_FLAT_TO_VERTEX_TO_VERTEX = 1.1547005383792515  # 2 / sqrt(3)
VERTEX_TO_VERTEX_TO_FLAT_TO_FLAT = 1 / FLAT_TO_FLAT_TO_VERTEX_TO_VERTEX

# ------------------------------------------------------------------------------------------------ cube coordinates of a hex grid

Hex = namedtuple('Hex', ['q', 'r', 's'])

_DIRS = (Hex(1, 0, -1), Hex(1, -1, 0), Hex(0, -1, 1), Hex(-1, 0, 1), Hex(-1, 1, 0), Hex(0, 1, -1))


def add_hex(h1, h2):
    """Componentwise sum of two hex coordinates."""
    return Hex(h1.q + h2.q, h1.r + h2.r, h1.s + h2.s)


def sub_hex(h1, h2):
    """Componentwise difference of two hex coordinates."""
    return Hex(h1.q - h2.q, h1.r - h2.r, h1.s - h2.s)


def mul_hex(h1, h2):
    """Componentwise product of two hex coordinates."""
    return Hex(h1.q * h2.q, h1.r * h2.r, h1.s * h2.s)


def hex_dir(i):
    """The unit step in direction i, taken modulo 6."""
    return _DIRS[i % 6]


def hex_neighbor(h, direction):
    """The neighbour of h in `direction`."""
    return add_hex(h, hex_dir(direction))


def hex_to_xy(h, radius, rot=90):
    """(x, y) of the centre of hex h for cells of vertex radius `radius`, flat side up (rot=90) or vertex up (any other rot)."""
    if rot == 90:
        x, y = 1.5 * h.q, VERTEX_TO_VERTEX_TO_FLAT_TO_FLAT * h.q + np.sqrt(3) * h.r
    else:
        x, y = np.sqrt(3) * h.q + VERTEX_TO_VERTEX_TO_FLAT_TO_FLAT * h.r, 1.5 * h.r
    return x * radius, y * radius


def scale_hex(h, k):
    """h times the scalar k."""
    return Hex(h.q * k, h.r * k, h.s * k)


def hex_ring(radius):
    """The 6 * radius hexes of ring `radius`, starting from the 'north' one and going round."""
    tile, ring = Hex(-radius, radius, 0), []
    for side in range(6):
        for _ in range(radius):
            ring.append(tile)
            tile = hex_neighbor(tile, side)
    return ring[radius:] + ring[:radius]


def _local_window(cy, cx, center, dx, samples_per_seg, x, y):
    """(row slice, column slice) of the 2 samples_per_seg square about `center`, clipped to the array."""
    if isinstance(samples_per_seg, int):
        samples_per_seg = (samples_per_seg, samples_per_seg)
    lo_x = cx + int(center[0] / dx) - samples_per_seg[0]
    lo_y = cy + int(center[1] / dx) - samples_per_seg[1]
    hi_x, hi_y = lo_x + 2 * samples_per_seg[0], lo_y + 2 * samples_per_seg[1]
    nx, ny = x.shape[1], y.shape[0]
    clip = lambda v, n: min(max(v, 0), n)  # noqa: E731
    return slice(clip(lo_y, ny), clip(hi_y, ny)), slice(clip(lo_x, nx), clip(hi_x, nx))


# ------------------------------------------------------------------------------------------------ geometry (host, numpy)

def _hexagon_vertices(radius, center, rotation):
    k = np.arange(6, dtype=config.precision)
    a = k * (2 * np.pi / 6) + np.radians(rotation)
    return np.stack((radius * np.sin(a) + center[0], radius * np.cos(a) + center[1]), axis=1)


def _polygon_sdf(verts, x, y):
    """signed distance to a closed polygon, negative inside (even-odd rule for the sign)"""
    d2 = inside = None
    n = len(verts)
    for i in range(n):
        ax, ay = (float(v) for v in verts[i])
        bx, by = (float(v) for v in verts[(i + 1) % n])
        ex, ey = bx - ax, by - ay
        wx, wy = x - ax, y - ay
        t = np.clip((wx * ex + wy * ey) / (ex * ex + ey * ey), 0, 1)
        px, py = wx - t * ex, wy - t * ey
        e2 = px * px + py * py
        d2 = e2 if d2 is None else np.minimum(d2, e2)
        crosses = ((ay > y) != (by > y)) & ((wx * ey < ex * wy) == (by > ay))
        inside = crosses if inside is None else inside ^ crosses
    d = np.sqrt(d2)
    return np.where(inside, -d, d)


def _antialias(d, dx):
    """pixel coverage of a signed distance: 1 inside, 0 outside, a one-sample ramp across the edge"""
    return np.minimum(np.maximum(0.5 - d / dx, 0), 1)


def _host(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().numpy()
    return np.asarray(a)


def _geometry(rings, segment_diameter, segment_separation, x, y, segment_angle, exclude):
    """(vtov, all_centers, windows, local_coords, local_masks, segment_ids, amp) of the reference's _composite_hexagonal_aperture,
    in numpy"""
    if segment_angle not in {0, 90}:
        raise ValueError('can only synthesize composite apertures with hexagons along a cartesian axis')
    vtov = segment_diameter * FLAT_TO_FLAT_TO_VERTEX_TO_VERTEX
    gap = segment_separation * FLAT_TO_FLAT_TO_VERTEX_TO_VERTEX / 2
    rseg = vtov / 2
    dx = x[0, 1] - x[0, 0]
    spp = int(rseg / dx + 1)
    cx, cy = int(np.ceil(x.shape[1] / 2)), int(np.ceil(y.shape[0] / 2))
    amp = np.zeros(x.shape, dtype=config.precision)
    centers, windows, coords, masks, ids = [], [], [], [], []

    def add(sid, center, local):
        win = _local_window(cy, cx, center, dx, spp, x, y)
        xx, yy = x[win], y[win]
        m = _antialias(_polygon_sdf(_hexagon_vertices(rseg, center, segment_angle), xx, yy), dx)
        amp[win] = np.maximum(amp[win], m)
        ids.append(sid)
        windows.append(win)
        coords.append(local(xx, yy))
        masks.append(m)

    if 0 not in exclude:
        centers.append((0., 0.))
        add(0, (0, 0), lambda xx, yy: (xx, yy))
    last = 0
    for ring in range(1, rings + 1):
        cs = np.array([hex_to_xy(h, rseg + gap, rot=segment_angle) for h in hex_ring(ring)])
        rid = np.arange(last + 1, last + 1 + len(cs), dtype=int)
        keep = ~np.isin(rid, exclude, assume_unique=True)
        centers += cs[keep].tolist()
        for sid, c in zip(rid[keep], cs[keep]):
            add(sid, c, lambda xx, yy, c=c: (xx - c[0], yy - c[1]))
        last = rid[-1]
    return vtov, centers, windows, coords, masks, ids, amp


def _grid_sources(local_coords, share):
    """g(s): the segment whose local grid segment s uses -- the first one with the same (local_x[0, 0], *shape) key (the reference's
    grid cache), or s itself"""
    first, src = {}, []
    for s, (lx, _) in enumerate(local_coords):
        if not share or lx.size == 0:
            src.append(s)
        else:
            src.append(first.setdefault((float(lx[0, 0]), *lx.shape), s))
    return src


# ------------------------------------------------------------------------------------------------ the segment plan

# struct pm::SegDesc (csrc/segmented.hip), 80 bytes
_DESC_DTYPE = np.dtype([('y0', '<i4'), ('x0', '<i4'), ('h', '<i4'), ('w', '<i4'), ('gy0', '<i4'), ('gx0', '<i4'), ('pad0', '<i4'),
                        ('pad1', '<i4'), ('moff', '<i8'), ('boff', '<i8'), ('cx', '<f8'), ('cy', '<f8'), ('nr', '<f8'), ('pad2', '<f8')])
assert _DESC_DTYPE.itemsize == 80


class SegmentPlan:
    """What the kernels read, on the host: desc (S records of _DESC_DTYPE), masks (the S masks packed, in the aperture's dtype),
    cover (P x rows * cols int16: plane i holds the i-th segment whose window covers the point with a non-zero mask, -1 past the
    last), src (the grid source of each segment) and window_pts (the largest window)."""

    def __init__(self, shape, windows, masks, centers, src, nr, dtype, basis_offsets=None):
        rows, cols = shape
        S = len(windows)
        d = np.zeros(S, dtype=_DESC_DTYPE)
        off = 0
        count = np.zeros(rows * cols, dtype=np.int64)
        lists = []
        for s, (win, m) in enumerate(zip(windows, masks)):
            ys, xs = win
            g = windows[src[s]]
            d[s]['y0'], d[s]['x0'], d[s]['h'], d[s]['w'] = ys.start, xs.start, ys.stop - ys.start, xs.stop - xs.start
            d[s]['gy0'], d[s]['gx0'] = g[0].start, g[1].start
            d[s]['moff'] = off
            d[s]['boff'] = 0 if basis_offsets is None else basis_offsets[s]
            d[s]['cx'], d[s]['cy'] = (float(v) for v in centers[src[s]])
            d[s]['nr'] = nr
            off += m.size
            r, c = np.nonzero(m)
            pix = (r + ys.start) * cols + (c + xs.start)
            lists.append(pix)
            count[pix] += 1
        P = int(count.max()) if S and count.size else 0
        cover = np.full((P, rows * cols), -1, dtype=np.int16)
        fill = np.zeros(rows * cols, dtype=np.int64)
        for s, pix in enumerate(lists):
            cover[fill[pix], pix] = s
            fill[pix] += 1
        self.shape, self.desc, self.cover, self.src = (rows, cols), d, cover, list(src)
        self.masks = np.concatenate([np.asarray(m, dtype=dtype).ravel() for m in masks]) if S else np.zeros(0, dtype=dtype)
        self.window_pts = int(max((int(r['h']) * int(r['w']) for r in d), default=0))

    @property
    def nbytes(self):
        return self.desc.nbytes + self.masks.nbytes + self.cover.nbytes

    def check(self, nmodes, basis_elems=-1):
        """pm_segment_plan_check on the host copy: ValueError if any window, mask or basis would fall outside its buffer"""
        L.check(L.load().pm_segment_plan_check(self.shape[0], self.shape[1], len(self.desc), self.desc.ctypes.data_as(L.c_vp),
                                               self.masks.size, nmodes, basis_elems))

    def _seg(self, s):
        r = self.desc[s]
        y0, x0, h, w, moff = int(r['y0']), int(r['x0']), int(r['h']), int(r['w']), int(r['moff'])
        return y0, x0, h, w, self.masks[moff:moff + h * w]


def evaluate_compose(plan, coefs, bases, out=None):
    """compose_opd in numpy, driven by the plan's cover planes: (rows, cols) for coefs (S, K); bases[s] is the (K, h, w) basis
    segment s uses (that of its grid source).  The kernels' order: a pixel adds mask * tile of its segments in cover order."""
    rows, cols = plan.shape
    acc = np.zeros(rows * cols, dtype=plan.masks.dtype) if out is None else np.array(out, dtype=plan.masks.dtype).ravel()
    for pas in plan.cover:
        for s in np.unique(pas[pas >= 0]):
            y0, x0, h, w, m = plan._seg(s)
            pix = np.flatnonzero(pas == s)
            li = (pix // cols - y0) * w + (pix % cols - x0)
            tile = np.asarray(coefs[s]) @ np.asarray(bases[s]).reshape(len(coefs[s]), -1)[:, li]
            acc[pix] += tile * m[li]
    return acc.reshape(rows, cols)


def evaluate_project(plan, g, bases):
    """compose_opd_adjoint in numpy: (S, K), sum over the window of s of mask_s * basis_s[k] * g"""
    out = []
    for s in range(len(plan.desc)):
        y0, x0, h, w, m = plan._seg(s)
        gw = np.asarray(g)[y0:y0 + h, x0:x0 + w].ravel()
        out.append(np.asarray(bases[s]).reshape(-1, h * w) @ (m * gw))
    return np.array(out)


# ------------------------------------------------------------------------------------------------ the aperture

class _Lazy(Sequence):
    """A list whose element i is make(key_of[i]), made on first access and cached per key"""

    def __init__(self, keys, make):
        self._keys, self._make, self._cache = list(keys), make, {}

    def __len__(self):
        return len(self._keys)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        k = self._keys[i]
        if k not in self._cache:
            self._cache[k] = self._make(k)
        return self._cache[k]


def _check_real(a, what):
    if (a.is_complex() if isinstance(a, torch.Tensor) else np.iscomplexobj(a)):
        raise TypeError(f'{what} must be real')


def _shape(a):
    return tuple(a.shape) if isinstance(a, torch.Tensor) else np.shape(a)


class CompositeHexagonalAperture:
    """An aperture of hexagonal segments (prysm/segmented.py CompositeHexagonalAperture) whose per-segment OPD is composed on the
    device.  share_grids=True keeps the reference's grid sharing (see the module docstring); False gives each segment its own grid."""

    def __init__(self, x, y, rings, segment_diameter, segment_separation, segment_angle=90, exclude=(), share_grids=True):
        hx, hy = _host(x), _host(y)
        _check_real(hx, 'x')
        _check_real(hy, 'y')
        (self.vtov, self.all_centers, self.windows, self.host_local_coords, self.host_local_masks, self.segment_ids,
         self.host_amp) = _geometry(rings, segment_diameter, segment_separation, hx, hy, segment_angle, exclude)
        self.x, self.y = x, y
        self.segment_diameter = segment_diameter
        self.segment_separation = segment_separation
        self.segment_angle = segment_angle
        self.exclude = exclude
        self.share_grids = bool(share_grids)
        self.dtype = torch.float32 if hx.dtype == np.float32 and hy.dtype == np.float32 else torch.float64
        self._hx, self._hy = hx, hy
        self._src = _grid_sources(self.host_local_coords, self.share_grids)
        self._dev = {}

    # device copies, made once on first use
    def _upload(self, name, make):
        if name not in self._dev:
            self._dev[name] = make()
        return self._dev[name]

    @property
    def amp(self):
        return self._upload('amp', lambda: L.as_device(self.host_amp))

    @property
    def local_masks(self):
        return self._upload('masks', lambda: [L.as_device(m) for m in self.host_local_masks])

    @property
    def local_coords(self):
        return self._upload('coords', lambda: [(L.as_device(a), L.as_device(b)) for a, b in self.host_local_coords])

    @property
    def grid_sources(self):
        """g(s) for every segment: the segment whose local coordinates segment s is evaluated on"""
        return list(self._src)

    def _np_dtype(self):
        return np.float32 if self.dtype == torch.float32 else np.float64

    def _host_grid(self, s, polar, nr):
        lx, ly = self.host_local_coords[s]
        if polar:
            r, t = np.hypot(lx, ly), np.arctan2(ly, lx)
            return r / nr[0], t
        return lx / nr[0], ly / nr[1]

    def prepare_opd_bases(self, basis_func, orders, basis_func_kwargs=None, normalization_radius=None):
        """Prepare the per-segment bases (segmented.py:178-259); returns (grids, bases) and sets opd_grids / opd_bases.

        basis_func is polynomials.zernike_nm_seq (kwargs: norm only): no basis is stored, the kernels walk the Zernike table per
        point, and opd_bases / opd_grids are made on first access.  Any other callable is called per unique grid with r / t or x / y
        device tensors (chosen from its signature) and its (K, h, w) output is kept on the device."""
        from .polynomials import zernike as Z
        if normalization_radius is None:
            normalization_radius = self.vtov / 2
        if not isinstance(normalization_radius, (tuple, list)):
            normalization_radius = (normalization_radius, normalization_radius)
        nr = tuple(float(v) for v in normalization_radius)
        kw = dict(basis_func_kwargs or {})
        params = inspect.signature(basis_func).parameters
        polar = 'r' in params and 't' in params
        zern = basis_func is Z.zernike_nm_seq and set(kw) <= {'norm'}
        src, S = self._src, len(self.windows)
        npdt = self._np_dtype()
        if zern:
            nms = Z.check_nms(orders)
            norm = bool(kw.get('norm', True))
            plan = SegmentPlan(self._hx.shape, self.windows, self.host_local_masks, self.all_centers, src, nr[0], npdt)
            plan.check(len(nms))

            def grid(g):
                r, t = self._host_grid(g, True, nr)
                return L.as_device(r, self.dtype), L.as_device(t, self.dtype)

            grids = _Lazy(src, grid)
            bases = _Lazy(src, lambda g: Z.zernike_nm_seq(nms, *grids[g], norm=norm))
            self._route = dict(kind=L.PM_SEGMENT_ZERNIKE, nms=nms, norm=norm, nmodes=len(nms), plan=plan)
        else:
            uniq = sorted(set(src))
            made, grids_u = {}, {}
            for g in uniq:
                a, b = self._host_grid(g, polar, nr)
                a, b = L.as_device(a, self.dtype), L.as_device(b, self.dtype)
                out = basis_func(orders, **({'r': a, 't': b} if polar else {'x': a, 'y': b}), **kw)
                if isinstance(out, (list, tuple)):
                    out = torch.stack([L.as_device(m, self.dtype) for m in out])
                out = L.as_device(out, self.dtype)
                if out.dim() != 3 or tuple(out.shape[1:]) != tuple(a.shape):
                    raise ValueError(f'basis_func returned shape {tuple(out.shape)}, want (K, {a.shape[0]}, {a.shape[1]})')
                made[g], grids_u[g] = out, (a, b)
            Ks = {int(m.shape[0]) for m in made.values()}
            if len(Ks) > 1:
                raise ValueError(f'basis_func returned different numbers of modes per grid: {sorted(Ks)}')
            K = Ks.pop() if Ks else 0
            offs, off = {}, 0
            for g in uniq:
                offs[g] = off
                off += made[g].numel()
            packed = torch.empty(off, dtype=self.dtype, device=L.device())
            for g in uniq:
                packed[offs[g]:offs[g] + made[g].numel()] = made[g].reshape(-1)
            plan = SegmentPlan(self._hx.shape, self.windows, self.host_local_masks, self.all_centers, src, nr[0], npdt,
                               basis_offsets=[offs[src[s]] for s in range(S)])
            plan.check(K, packed.numel())
            views = {g: packed[offs[g]:offs[g] + made[g].numel()].view(made[g].shape) for g in uniq}
            grids = [grids_u[src[s]] for s in range(S)]
            bases = [views[src[s]] for s in range(S)]
            self._route = dict(kind=L.PM_SEGMENT_STORED, nmodes=K, plan=plan, basis=packed)
        self._dev.pop('plan', None)
        self.opd_grids, self.opd_bases = grids, bases
        return grids, bases

    @property
    def segment_plan(self):
        """the host SegmentPlan of the last prepare_opd_bases"""
        self._prepared()
        return self._route['plan']

    def _prepared(self):
        if not hasattr(self, '_route'):
            raise AttributeError("'CompositeHexagonalAperture' object has no attribute 'opd_bases': call prepare_opd_bases first")

    def _device_plan(self):
        def make():
            p = self._route['plan']
            d = dict(desc=L.as_device(p.desc.view(np.uint8)), masks=L.as_device(p.masks),
                     cover=L.as_device(p.cover) if p.cover.size else None)
            if self._route['kind'] == L.PM_SEGMENT_ZERNIKE:
                from .polynomials import zernike as Z
                d['x'], d['y'] = L.as_device(self._hx, self.dtype), L.as_device(self._hy, self.dtype)
                d['table'], d['nsteps'] = Z._table(self._route['nms'], self._route['norm'], self.dtype)
            else:
                d['x'] = d['y'] = d['table'] = None
                d['nsteps'] = 0
            return d
        return self._upload('plan', make)

    def _args(self):
        r = self._route
        d = self._device_plan()
        return d, r['kind'], r['nmodes'], r.get('basis')

    def compose_opd(self, coefs, out=None):
        """sum over segments of mask_s * sum_k coefs[s, k] basis_{s,k}, each in its window (segmented.py:261-285), in one launch.
        coefs (S, K) gives (rows, cols); (B, S, K) gives (B, rows, cols).  `out`, if given, is added to in place and returned.  The
        coefficients are read on the device when the kernel runs, so a captured graph uses their current values."""
        self._prepared()
        S, K = len(self.windows), self._route['nmodes']
        shape = _shape(coefs)
        if len(shape) not in (2, 3) or tuple(shape[-2:]) != (S, K):
            raise ValueError(f'coefs of shape {tuple(shape)} do not match {S} segments x {K} modes (want ({S}, {K}) or (B, {S}, {K}))')
        _check_real(coefs if isinstance(coefs, torch.Tensor) else np.asarray(coefs), 'coefs')
        rows, cols = self._hx.shape
        B = 1 if len(shape) == 2 else shape[0]
        oshape = (rows, cols) if len(shape) == 2 else (B, rows, cols)
        host_out = None
        if out is not None:
            if _shape(out) != oshape:
                raise ValueError(f'out of shape {_shape(out)} does not match the result shape {oshape}')
            _check_real(out, 'out')
            if isinstance(out, torch.Tensor):
                if out.device != L.device() or out.dtype != self.dtype or not out.is_contiguous():
                    raise TypeError(f'out must be a contiguous {self.dtype} tensor on {L.device()}')
                res = out
            else:
                host_out, res = out, L.as_device(out, self.dtype).clone()
        else:
            res = torch.empty(oshape, dtype=self.dtype, device=L.device())
        c = L.as_device(coefs, self.dtype)
        d, kind, K, basis = self._args()
        code = L.PM_F32 if self.dtype == torch.float32 else L.PM_F64
        L.check(L.load().pm_segment_compose(code, kind, rows, cols, L.ptr(d['x']), L.ptr(d['y']), S, L.ptr(d['desc']), L.ptr(d['masks']),
                                            d['cover'].shape[0] if d['cover'] is not None else 0, L.ptr(d['cover']), L.ptr(d['table']),
                                            d['nsteps'], K, L.ptr(basis), B, L.ptr(c), int(out is not None), L.ptr(res), L.stream_ptr()))
        if host_out is not None:
            host_out[...] = res.cpu().numpy()
            return host_out
        return res

    def compose_opd_adjoint(self, opd_bar):
        """The adjoint of compose_opd with respect to the coefficients: coefs_bar[s, k] = sum over the window of s of
        mask_s * basis_{s,k} * opd_bar, (S, K) for a (rows, cols) opd_bar and (B, S, K) for (B, rows, cols).  Two launches, no atomics:
        bitwise reproducible."""
        self._prepared()
        rows, cols = self._hx.shape
        shape = _shape(opd_bar)
        if shape != (rows, cols) and (len(shape) != 3 or tuple(shape[1:]) != (rows, cols)):
            raise ValueError(f'opd_bar of shape {tuple(shape)} does not match the aperture grid {(rows, cols)} (or a (B, ...) stack)')
        _check_real(opd_bar, 'opd_bar')
        S, K = len(self.windows), self._route['nmodes']
        single = len(shape) == 2
        B = 1 if single else shape[0]
        g = L.as_device(opd_bar, self.dtype)
        out = torch.empty((B, S, K), dtype=self.dtype, device=L.device())
        if S and K and B:
            d, kind, K, basis = self._args()
            from .polynomials._modal import _projector
            wpts = self._route['plan'].window_pts
            _projector('segment', self.dtype, wpts, S, K, B)(kind, rows, cols, L.ptr(d['x']), L.ptr(d['y']), S, L.ptr(d['desc']),
                                                             L.ptr(d['masks']), wpts, L.ptr(d['table']), d['nsteps'], K, L.ptr(basis), B,
                                                             L.ptr(g), L.ptr(out))
        elif B:
            out.zero_()
        return out[0] if single else out
