"""Host side of the ray trace (csrc/raytrace.hip): the surface table, the conic-seed departure band, and the kernel in numpy.

`pack_table` turns a list of prysm_amd.x.raytracing Surface objects into the (J, REC) float64 table pm_rt_trace reads, `unpack_table`
reads one back.  `departure_band` is Surface._compute_departure_band of the reference (surfaces.py:1272-1339) for the even asphere,
on the host in float64.

`trace` is pm_rt_trace: per ray-array the operations of the kernel in the kernel's order, in the dtype of the rays it is given, a
lane's `if` a mask.  Vectors are tuples of three component arrays.  It is the model the CPU tests run and the GPU tests compare the
device with at sizes the fixture does not hold; nothing here touches a device.
"""
import warnings

import numpy as np

# the record of one surface, in doubles (the enum at the top of csrc/raytrace.hip)
REC = 48
MAX_SURFACES = 4096
MAX_COEFS = 8
(REC_INTERACTION, REC_SHAPE, REC_C, REC_K, REC_DX, REC_DY, REC_NCOEF, REC_COEF) = (0, 1, 2, 3, 4, 5, 6, 7)
(REC_P, REC_R, REC_HAS_R, REC_NPOST) = (15, 18, 27, 28)
(REC_AP_KIND, REC_AP_X0, REC_AP_Y0, REC_AP_RIN, REC_AP_ROUT) = (29, 30, 31, 32, 33)
(REC_BOUNDED, REC_MAX_DEP, REC_DOMAIN_R, REC_GRAD_BOUND, REC_LIPSCHITZ) = (34, 35, 36, 37, 38)
(REC_FIRST, REC_ANALYTIC) = (39, 40)

REFLECT, REFRACT, MEASURE = 0, 1, 2
PLANE, CONIC, ASPHERE = 0, 1, 2
AP_NONE, AP_CIRCULAR, AP_ANNULAR = 0, 1, 2
OK, NEWTON, CLIP, MISS, TIR = 0, 1, 2, -1, -2

# the reference's interaction constants (spencer_and_murty.py:15-19)
STYPE_REFLECT, STYPE_REFRACT, STYPE_EVAL, STYPE_OBJ, STYPE_IMG = -1, -2, -3, -4, -5
_INTERACTION = {STYPE_REFLECT: REFLECT, STYPE_REFRACT: REFRACT, STYPE_EVAL: MEASURE, STYPE_OBJ: MEASURE, STYPE_IMG: MEASURE}
_SHAPE = {'Plane': PLANE, 'Sphere': CONIC, 'Conic': CONIC, 'OffAxisConic': CONIC, 'EvenAsphere': ASPHERE}

NEWTON_ITERS = 100
MARCH_STEPS = 256
DEPARTURE_BAND_SAMPLES = 64
DEPARTURE_GRADIENT_WARN = 0.5
MARCH_RADIUS_MARGIN = 1.1
DEFAULT_TOL_SAG = 1e-12


def resolve_tol_sag(tol_sag, dtype):
    """1e-12, or 100 eps of `dtype` where that is larger; a given value stands (spencer_and_murty.py:180-204)"""
    if tol_sag is None:
        return max(DEFAULT_TOL_SAG, float(np.finfo(np.dtype(dtype)).eps) * 100.0)
    return tol_sag


def index_of(material, wvl):
    """a material is anything with .n(wvl); a plain number is a constant index"""
    if material is None:
        return None
    if hasattr(material, 'n'):
        return float(material.n(wvl))
    return float(material)


def launch_index(surfaces, wvl):
    """the index the bundle starts in: that of a leading measurement surface's material, otherwise 1 (spencer_and_murty.py:482-497)"""
    if len(surfaces) > 0:
        first = surfaces[0]
        if _INTERACTION.get(getattr(first, 'typ', None)) == MEASURE and getattr(first, 'material', None) is not None:
            return index_of(first.material, wvl)
    return 1.0


def pack_table(surfaces, wvl):
    """(J, REC) float64: one record per surface, the indices at wavelength `wvl`"""
    J = len(surfaces)
    if J > MAX_SURFACES:
        raise ValueError(f'{J} surfaces are more than the table limit of {MAX_SURFACES}')
    tab = np.zeros((J, REC), dtype=np.float64)
    for j, s in enumerate(surfaces):
        r = tab[j]
        kind = _SHAPE[type(s.shape).__name__]
        p = s.shape.params or {}
        r[REC_INTERACTION] = _INTERACTION[s.typ]
        r[REC_SHAPE] = kind
        r[REC_C], r[REC_K] = p.get('c', 0.0), p.get('k', 0.0)
        r[REC_DX], r[REC_DY] = p.get('dx', 0.0), p.get('dy', 0.0)
        coefs = tuple(p.get('coefs', ()))
        if len(coefs) > MAX_COEFS:
            raise NotImplementedError(f'an even asphere of {len(coefs)} coefficients: the surface table holds {MAX_COEFS}')
        r[REC_NCOEF] = len(coefs)
        r[REC_COEF:REC_COEF + len(coefs)] = coefs
        r[REC_P:REC_P + 3] = s.P
        if s.R is not None:
            r[REC_R:REC_R + 9] = np.asarray(s.R, dtype=np.float64).reshape(9)
            r[REC_HAS_R] = 1.0
        n_post = index_of(s.material, wvl)
        r[REC_NPOST] = 1.0 if n_post is None else n_post
        clip = s.aperture.clip
        if clip is not None:
            r[REC_AP_X0], r[REC_AP_Y0] = clip.x0, clip.y0
            if hasattr(clip, 'inner_radius'):
                r[REC_AP_KIND], r[REC_AP_RIN], r[REC_AP_ROUT] = AP_ANNULAR, clip.inner_radius, clip.outer_radius
            else:
                r[REC_AP_KIND], r[REC_AP_ROUT] = AP_CIRCULAR, clip.radius
        band = s.departure_band()
        if band.bounded:
            r[REC_BOUNDED] = 1.0
            r[REC_MAX_DEP], r[REC_DOMAIN_R], r[REC_GRAD_BOUND], r[REC_LIPSCHITZ] = (band.max_departure, band.domain_radius, band.gradient_bound,
                                                                                    band.lipschitz)
        r[REC_FIRST] = 1.0 if j == 0 else 0.0
        r[REC_ANALYTIC] = 1.0 if kind != ASPHERE else 0.0
    return tab


def unpack_table(tab):
    """the records as dicts: what pack_table stored, by name"""
    out = []
    for r in np.asarray(tab, dtype=np.float64).reshape(-1, REC):
        nc = int(r[REC_NCOEF])
        out.append(dict(interaction=int(r[REC_INTERACTION]), shape=int(r[REC_SHAPE]), c=r[REC_C], k=r[REC_K], dx=r[REC_DX], dy=r[REC_DY],
                        coefs=tuple(r[REC_COEF:REC_COEF + nc]), P=r[REC_P:REC_P + 3].copy(),
                        R=r[REC_R:REC_R + 9].reshape(3, 3).copy() if r[REC_HAS_R] else None, n_post=r[REC_NPOST],
                        aperture=(int(r[REC_AP_KIND]), r[REC_AP_X0], r[REC_AP_Y0], r[REC_AP_RIN], r[REC_AP_ROUT]),
                        band=(r[REC_MAX_DEP], r[REC_DOMAIN_R], r[REC_GRAD_BOUND], r[REC_LIPSCHITZ]) if r[REC_BOUNDED] else None,
                        first=bool(r[REC_FIRST]), analytic=bool(r[REC_ANALYTIC])))
    return out


# --------------------------------------------------------------------------- sags and normals

def _conic_sag_normal(T, c, k, X, Y):
    """conic_sag_and_normal (sags.py:109-121), c != 0: (z, (nx, ny, nz))"""
    A = X * X + Y * Y
    phi = np.sqrt(T(1) - ((T(1) + k) * (c * c)) * A)
    phi = np.where(np.isnan(phi), T(0), phi)
    mag_sq = T(1) - ((k * c) * c) * A
    mag = np.sqrt(np.where(mag_sq < T(0), T(1), mag_sq))
    z = (c * A) / (T(1) + phi)
    return z, (((-c) * X) / mag, ((-c) * Y) / mag, phi / mag)


def _asphere(T, coefs, c, k, x, y):
    """EvenAsphere.sag_and_normal (surfaces.py:680-688, sags.py:413-483): (z, (nx, ny, nz))"""
    rsq = x * x + y * y
    phi = np.sqrt(T(1) - ((T(1) + k) * (c * c)) * rsq)
    z = (c * rsq) / (T(1) + phi)
    fx, fy = (c * x) / phi, (c * y) / phi
    if len(coefs) > 0:
        p, q = T(0), T(0)
        for i in range(len(coefs) - 1, -1, -1):
            a = T(coefs[i])
            p = p * rsq + a
            q = q * rsq + T(i + 2) * a
        z = z + (p * rsq) * rsq
        common = (T(2) * rsq) * q
        fx = fx + x * common
        fy = fy + y * common
    inv = T(1) / np.sqrt((T(1) + fx * fx) + fy * fy)
    return z, ((-fx) * inv, (-fy) * inv, inv)


class DepartureBand:
    """Conic-seed departure bounds (surfaces.py:92-132); bounded False: no finite bound"""
    __slots__ = ('bounded', 'max_departure', 'domain_radius', 'gradient_bound', 'lipschitz')

    def __init__(self, *, bounded, max_departure=None, domain_radius=None, gradient_bound=None, lipschitz=None):
        self.bounded, self.max_departure, self.domain_radius = bounded, max_departure, domain_radius
        self.gradient_bound, self.lipschitz = gradient_bound, lipschitz

    @classmethod
    def unbounded(cls):
        return cls(bounded=False)

    def __repr__(self):
        if not self.bounded:
            return 'DepartureBand(bounded=False)'
        return (f'DepartureBand(max_departure={self.max_departure:g}, domain_radius={self.domain_radius:g}, '
                f'gradient_bound={self.gradient_bound:g}, lipschitz={self.lipschitz:g})')


def departure_band(c, k, coefs, limiting_radius):
    """Surface._compute_departure_band (surfaces.py:1272-1339) for an even asphere: the largest departure of the sag from the seed conic,
    of its slope, and of the sag's slope, over 64 x 64 samples of the disk of the aperture's limiting radius (or, without one, just
    inside the seed conic's own domain), each padded by 1.1"""
    T = np.float64
    c, k = T(c), T(k)
    R = limiting_radius
    if R is None:
        ckk = (1.0 + k) * c * c
        if ckk > 0.0:
            R = 0.999 / np.sqrt(ckk)
    if R is None or not np.isfinite(R) or R <= 0:
        return DepartureBand.unbounded()
    R = float(R)
    n = DEPARTURE_BAND_SAMPLES
    xs = np.linspace(-R, R, n, dtype=np.float64)
    X, Y = np.meshgrid(xs, xs)
    outside = X * X + Y * Y > R * R
    with np.errstate(all='ignore'):
        z_sag, n_sag = _asphere(T, coefs, c, k, X, Y)
        if c == 0.0:
            z_con, n_con = np.zeros_like(X), (np.zeros_like(X), np.zeros_like(X), np.ones_like(X))
        else:
            z_con, n_con = _conic_sag_normal(T, c, k, X, Y)
            z_con = (c * (X * X + Y * Y)) / (1 + np.sqrt(1 - (1 + k) * (c * c) * (X * X + Y * Y)))      # conic_sag without the NaN guard
        dep = z_sag - z_con
        gx = n_con[0] / n_con[2] - n_sag[0] / n_sag[2]
        gy = n_con[1] / n_con[2] - n_sag[1] / n_sag[2]
        gmag_dep = np.hypot(gx, gy)
    dep[outside] = np.nan
    gmag_dep[outside] = np.nan
    if not np.isfinite(dep).any():
        return DepartureBand.unbounded()
    D = float(np.nanmax(np.abs(dep)))
    G = float(np.nanmax(gmag_dep))
    R_march = MARCH_RADIUS_MARGIN * R
    xm = np.linspace(-R_march, R_march, n, dtype=np.float64)
    Xm, Ym = np.meshgrid(xm, xm)
    with np.errstate(all='ignore'):
        _, nrm = _asphere(T, coefs, c, k, Xm, Ym)
        gmag = np.hypot(nrm[0], nrm[1]) / np.abs(nrm[2])
    gmag[Xm * Xm + Ym * Ym > R_march * R_march] = np.nan
    L = float(np.nanmax(gmag))
    if G >= DEPARTURE_GRADIENT_WARN:
        warnings.warn('a surface departs from its conic seed steeply enough that the intersection acceptance band can admit multiple ray '
                      'crossings; the traced intersection on such a surface may be ambiguous.')
    return DepartureBand(bounded=True, max_departure=1.1 * D, domain_radius=R, gradient_bound=1.1 * G, lipschitz=1.1 * L)


# --------------------------------------------------------------------------- the kernel in numpy

def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _axpy(p, t, s):
    return (p[0] + t * s[0], p[1] + t * s[1], p[2] + t * s[2])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _finite3(a):
    return np.isfinite(a[0]) & np.isfinite(a[1]) & np.isfinite(a[2])


def _where3(m, a, b):
    return tuple(np.where(m, a[i], b[i]) for i in range(3))


def _mul_rt(T, v, m):
    return tuple((v[0] * T(m[3 * i]) + v[1] * T(m[3 * i + 1])) + v[2] * T(m[3 * i + 2]) for i in range(3))


def _mul_r(T, v, m):
    return tuple((v[0] * T(m[i]) + v[1] * T(m[3 + i])) + v[2] * T(m[6 + i]) for i in range(3))


def _hit_plane(T, p, s):
    t = (-p[2]) / s[2]
    zero = np.zeros_like(t)
    return _axpy(p, t, s), (zero, zero, zero + T(1)), s[2] != T(0)


def _conic_abc(T, c, k, p1, s, dx, dy):
    xp, yp = p1[0] + dx, p1[1] + dy
    return T(1) + (k * s[2]) * s[2], (xp * s[0] + yp * s[1]) - s[2] / c, xp * xp + yp * yp


def _hit_conic(T, p, s, c, k, dx, dy):
    if c == T(0):
        return _hit_plane(T, p, s)
    s0 = (-p[2]) / s[2]
    p1 = _axpy(p, s0, s)
    A, B, C = _conic_abc(T, c, k, p1, s, dx, dy)
    disc = B * B - A * C
    disc_nonneg = disc >= T(0)
    disc = np.where(disc_nonneg, disc, T(0))
    sq = np.sqrt(disc)
    sign_c = T(1) if c > T(0) else T(-1)
    z_dir = np.where(s[2] < T(0), T(-1), T(1))
    denom = (z_dir * sign_c) * sq - B
    tangent = denom == T(0)
    t = np.where(tangent, T(0), C / np.where(tangent, T(1), denom))
    q = _axpy(p1, t, s)
    xq, yq = q[0] + dx, q[1] + dy
    rr = xq * xq + yq * yq
    phi_arg = T(1) - (((T(1) + k) * c) * c) * rr
    _, n = _conic_sag_normal(T, c, k, xq, yq)
    return q, n, disc_nonneg & (phi_arg >= T(0))


def _hit_asphere(T, rec, p, s, c, k, tol, tol100, forward_only, stats=None):
    coefs = rec[REC_COEF:REC_COEF + int(rec[REC_NCOEF])]
    nan = np.full_like(p[0], np.nan)
    s0 = (-p[2]) / s[2]
    p1 = _axpy(p, s0, s)
    seed_q, seed_n, seed_valid = _hit_conic(T, p1, s, c, k, T(0), T(0))
    s1 = seed_q[2] / s[2]
    q, n, valid = (nan, nan, nan), (nan, nan, nan), np.zeros(nan.shape, dtype=bool)
    active = _finite3(p1) & _finite3(s) & np.isfinite(s1)
    sj = s1.copy()
    for _ in range(NEWTON_ITERS):
        if not active.any():
            break
        pj = _axpy(p1, sj, s)
        z, nn = _asphere(T, coefs, c, k, pj[0], pj[1])
        F = pj[2] - z
        conv = active & (np.abs(F) < tol)
        q, n, valid = _where3(conv, pj, q), _where3(conv, nn, n), valid | conv
        active = active & ~conv
        Fp = _dot(s, nn) / nn[2]
        sj = np.where(active, sj - F / Fp, sj)
    bounded = rec[REC_BOUNDED] != 0.0
    if not bounded and not forward_only:
        return q, n, valid
    s_root = _dot(_sub(q, p1), s)
    if bounded:
        D, Rd, G, Lb = T(rec[REC_MAX_DEP]), T(rec[REC_DOMAIN_R]), T(rec[REC_GRAD_BOUND]), T(rec[REC_LIPSCHITZ])
        cosi = np.abs(_dot(s, seed_n))
        s_t = np.sqrt(np.maximum(T(0), T(1) - s[2] * s[2]))
        certified = (cosi - G * s_t) > T(1e-3)
        cosi = np.where(cosi >= T(1e-3), cosi, T(1e-3))
        band = (D + tol100 * (T(1) + np.abs(s1))) / cosi
        rseed_sq = seed_q[0] * seed_q[0] + seed_q[1] * seed_q[1]
        seed_ok = seed_valid & np.isfinite(s1)
        police = seed_ok & (rseed_sq <= Rd * Rd)
        in_band = np.abs(s_root - s1) <= band
        in_domain = (q[0] * q[0] + q[1] * q[1]) <= Rd * Rd
        prior_accept = valid & (~police | (in_band & in_domain)) & ~(~seed_ok & ~in_domain)
        certified_accept = valid & police & in_band & in_domain & certified
        rescue = police & ~certified_accept
        lo, hi = s1 - band, s1 + band
        if c != T(0):
            A, B, C = _conic_abc(T, c, k, p1, s, T(0), T(0))
            z_max = ((np.abs(c) * Rd) * Rd) / T(2) + D
            scale = T(2) / np.abs(c) + (T(2) * np.abs(T(1) + k)) * z_max
            d_imp = (D + tol100) * scale
            t_star = (-B) / A
            c_min = C - (B * B) / A
            wsq = (d_imp - c_min) / A
            rescuable = ~seed_ok & (A > T(0)) & (wsq >= T(0)) & np.isfinite(t_star)
            w = np.sqrt(np.abs(wsq))
            lo, hi = np.where(rescuable, t_star - w, lo), np.where(rescuable, t_star + w, hi)
            rescue = rescue | rescuable
        accept = certified_accept | prior_accept
        if rescue.any():
            Rm = T(1.1) * Rd
            a = s[0] * s[0] + s[1] * s[1]
            b = p1[0] * s[0] + p1[1] * s[1]
            cc = (p1[0] * p1[0] + p1[1] * p1[1]) - Rm * Rm
            disc = b * b - a * cc
            sq = np.sqrt(np.maximum(disc, T(0)))
            s_a, s_b = ((-b) - sq) / a, ((-b) + sq) / a
            swept = a > T(0)
            real = swept & (disc >= T(0))
            lo, hi = np.where(real, np.maximum(lo, s_a), lo), np.where(real, np.minimum(hi, s_b), hi)
            hi = np.where((swept & ~real) | (~swept & (cc > T(0))), lo - T(1), hi)
            lip = np.abs(s[2]) + Lb * s_t
            lip = np.where(lip > T(0), lip, T(1))
            found = np.zeros(rescue.shape, dtype=bool)
            active = rescue & (lo <= hi)
            sj = lo.copy()
            for _ in range(MARCH_STEPS):
                if not active.any():
                    break
                pj = _axpy(p1, sj, s)
                z, nn = _asphere(T, coefs, c, k, pj[0], pj[1])
                F = pj[2] - z
                conv = active & (np.abs(F) < tol)
                q, n, found = _where3(conv, pj, q), _where3(conv, nn, n), found | conv
                step_lip = np.abs(F) / lip
                Fp = _dot(s, nn) / nn[2]
                step_newton = (-F) / Fp
                near = np.isfinite(step_newton) & (np.abs(Fp) > T(1e-3)) & (step_lip < T(1e-2) * (T(1) + np.abs(sj)))
                s_new = np.minimum(np.maximum(np.where(near, sj + step_newton, sj + step_lip), lo), hi)
                exhausted = ~near & (sj + step_lip > hi)
                active = active & ~conv & ~exhausted & np.isfinite(F)
                sj = np.where(active, s_new, sj)
            if stats is not None:
                stats['rescued'] = stats.get('rescued', 0) + int(rescue.sum())
                stats['rescue_converged'] = stats.get('rescue_converged', 0) + int(found.sum())
            accept = np.where(rescue, found | prior_accept, accept)
            s_root = _dot(_sub(q, p1), s)
        valid = accept
    if forward_only:
        valid = valid & ~((s0 + s_root) < (-tol100) * (T(1) + np.abs(s0)))
    return q, n, valid


def trace(table, n_launch, tol_sag, P, S, history=True, stats=None):
    """pm_rt_trace on numpy arrays: P, S (N, 3) of float32 or float64, the dtype the walk runs in.  Returns P, S ((J + 1, N, 3), or
    (N, 3) without history), OPL ((J + 1, N) or (N,)) and the int32 status arrays surface and code.  `stats`: a dict that collects how
    many ray-visits went to the Lipschitz rescue and how many converged there."""
    P, S = np.asarray(P), np.asarray(S)
    T = P.dtype.type
    table = np.asarray(table, dtype=np.float64).reshape(-1, REC)
    J, N = table.shape[0], P.shape[0]
    tol, tol100, n = T(tol_sag), T(100.0 * tol_sag), T(n_launch)
    X, D = tuple(P[:, i].copy() for i in range(3)), tuple(S[:, i].astype(T) for i in range(3))
    code, surface = np.zeros(N, dtype=np.int32), np.zeros(N, dtype=np.int32)
    Ph, Sh, Oh = [np.stack(X, axis=-1)], [np.stack(D, axis=-1)], [np.zeros(N, dtype=T)]
    opl_sum = np.zeros(N, dtype=T)
    nan = np.full(N, np.nan, dtype=T)
    with np.errstate(all='ignore'):
        for j in range(J):
            rec = table[j]
            interaction, shape = int(rec[REC_INTERACTION]), int(rec[REC_SHAPE])
            has_r = rec[REC_HAS_R] != 0.0
            vertex = tuple(T(v) for v in rec[REC_P:REC_P + 3])
            p0, sl = _sub(X, vertex), D
            if has_r:
                p0, sl = _mul_rt(T, p0, rec[REC_R:REC_R + 9]), _mul_rt(T, sl, rec[REC_R:REC_R + 9])
            c, k = T(rec[REC_C]), T(rec[REC_K])
            if shape == PLANE:
                q, nh, valid = _hit_plane(T, p0, sl)
            elif shape == CONIC:
                q, nh, valid = _hit_conic(T, p0, sl, c, k, T(rec[REC_DX]), T(rec[REC_DY]))
            else:
                q, nh, valid = _hit_asphere(T, rec, p0, sl, c, k, tol, tol100, interaction != MEASURE and rec[REC_FIRST] == 0.0, stats)
            step = np.where(valid, OK, MISS if rec[REC_ANALYTIC] != 0.0 else NEWTON).astype(np.int32)
            ap = int(rec[REC_AP_KIND])
            if ap != AP_NONE:
                ax, ay = q[0] - T(rec[REC_AP_X0]), q[1] - T(rec[REC_AP_Y0])
                rsq = ax * ax + ay * ay
                rout, rin = T(rec[REC_AP_ROUT]), T(rec[REC_AP_RIN])
                inside = rsq <= rout * rout if ap == AP_CIRCULAR else (rsq >= rin * rin) & (rsq <= rout * rout)
                step[valid & ~inside] = CLIP
            sp = sl
            if interaction == REFLECT:
                cos_i = _dot(sl, nh)
                sp = _axpy(sl, -(T(2) * cos_i), nh)
            elif interaction == REFRACT:
                mu = n / T(rec[REC_NPOST])
                cos_i = _dot(nh, sl)
                sin_t_sq = (mu * mu) * (T(1) - cos_i * cos_i)
                cos_t = np.sqrt(T(1) - sin_t_sq)
                factor = np.sign(cos_i) * cos_t - mu * cos_i
                sp = (mu * sl[0] + factor * nh[0], mu * sl[1] + factor * nh[1], mu * sl[2] + factor * nh[2])
                step[(step == OK) & (np.isnan(sp[0]) | np.isnan(sp[1]) | np.isnan(sp[2]))] = TIR
            if has_r:
                q, sp = _mul_r(T, q, rec[REC_R:REC_R + 9]), _mul_r(T, sp, rec[REC_R:REC_R + 9])
            q = (q[0] + vertex[0], q[1] + vertex[1], q[2] + vertex[2])
            seg = _sub(q, X)
            opl = (n * np.sign(_dot(seg, D))) * np.sqrt(_dot(seg, seg))
            failed = (code == OK) & (step != OK)
            code[failed], surface[failed] = step[failed], j + 1
            if interaction == REFRACT:
                n = T(rec[REC_NPOST])
            dead = code != OK
            X, D, opl = _where3(dead, (nan, nan, nan), q), _where3(dead, (nan, nan, nan), sp), np.where(dead, nan, opl)
            X, D = tuple(np.asarray(v, dtype=T) for v in X), tuple(np.asarray(v, dtype=T) for v in D)
            if history:
                Ph.append(np.stack(X, axis=-1)), Sh.append(np.stack(D, axis=-1)), Oh.append(opl.astype(T))
            else:
                opl_sum = opl_sum + opl
    surface[code == OK] = J
    if history:
        return np.stack(Ph), np.stack(Sh), np.stack(Oh), surface, code
    return np.stack(X, axis=-1), np.stack(D, axis=-1), opl_sum, surface, code
