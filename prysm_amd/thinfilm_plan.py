"""The thin-film kernels (csrc/thinfilm.hip) restated in numpy, in both precisions.

`stack` is pm_tf_stack and `thickness_grad` is pm_tf_thickness_grad: the same sweep from the substrate, the same square root, sine
and cosine (written out on real and imaginary parts, as the kernel has them), the same order of every product, in complex64 /
float32 or complex128 / float64 throughout.  Samples are flat: every operand is an array of K values or of one value (a shared
operand), the layer tables are (L, K) or (L, 1).  What differs from the kernel is only the library behind sqrt, hypot, sin, cos and
expm1, and that numpy adds the samples of the gradient pairwise where the kernel adds per wavefront.

The tests compare the kernels against this model at sizes where the reference's own results are not stored, and the host tests
compare this model against the reference's results (tests/golden/coatings.npz), so the formulas are checked without a device.
"""
import numpy as np

S, P, BOTH = 0, 1, 2
T_STACK, T_THINFILM = 0, 1
_REAL = {np.dtype(np.complex64): np.float32, np.dtype(np.complex128): np.float64}


def pols_of(pol):
    """the polarisation code -> a tuple of is-p flags, one per vector the sweep carries"""
    return {S: (False,), P: (True,), BOTH: (False, True)}[pol]


def _cx(re, im, cd):
    out = np.empty(np.broadcast(re, im).shape, dtype=cd)
    out.real, out.imag = re, im
    return out


def csqrt(w):
    """principal square root; an imaginary part of zero of either sign counts as +0"""
    x, y = w.real, w.imag
    with np.errstate(invalid='ignore', divide='ignore'):
        m = np.hypot(x, y)
        two = x.dtype.type(2)
        re_a = np.sqrt((m + x) / two)
        a = (re_a, y / (two * re_a))
        im_b = np.sqrt((m - x) / two)
        b = (np.abs(y) / (two * im_b), np.where(y < 0, -im_b, im_b))
        re = np.where(x >= 0, a[0], b[0])
        im = np.where(x >= 0, a[1], b[1])
        zero = y == 0
        re = np.where(zero, np.where(x >= 0, np.sqrt(np.abs(x)), 0), re)
        im = np.where(zero, np.where(x >= 0, 0, np.sqrt(np.abs(x))), im)
    return _cx(re.astype(x.dtype), im.astype(x.dtype), w.dtype)


def csincos(z):
    """(sin z, cos z) of a complex array from sin, cos and expm1 of its parts"""
    rd = z.real.dtype.type
    sa, ca = np.sin(z.real), np.cos(z.real)
    em = np.expm1(z.imag)
    e = em + rd(1)
    sh = rd(0.5) * (em + em / e)
    ch = rd(0.5) * (e + rd(1) / e)
    return _cx(sa * ch, ca * sh, z.dtype), _cx(ca * ch, -(sa * sh), z.dtype)


def minus_i(z):
    return _cx(z.imag, -z.real, z.dtype)


def cos_snell(n0, n1, sin0):
    """cos(theta_1) by Snell's law, negated where sin(theta_1) is real and above 1"""
    sint = (n0 / n1) * sin0
    cost = csqrt(sint.dtype.type(1) - sint * sint)
    return np.where((sint.imag == 0) & (sint.real > 1), -cost, cost)


def admittance(n, cost, p):
    return n / cost if p else n * cost


class _Operands:
    def __init__(self, indices, thicknesses, wvl, theta, nsub, n0, dtype):
        cd = np.dtype(dtype)
        rd = _REAL[cd]
        self.cd, self.rd = cd, rd
        self.n = np.asarray(indices).astype(cd).reshape(len(indices), -1) if len(indices) else np.zeros((0, 1), cd)
        self.d = np.asarray(thicknesses).astype(rd).reshape(len(thicknesses), -1) if len(thicknesses) else np.zeros((0, 1), rd)
        self.L = self.n.shape[0]
        self.wvl = np.asarray(wvl).astype(rd).reshape(-1)
        theta = np.asarray(theta).astype(rd).reshape(-1)
        self.nsub = np.asarray(nsub).astype(cd).reshape(-1)
        self.n0 = np.asarray(n0).astype(cd).reshape(-1)
        self.K = max(self.wvl.size, theta.size, self.nsub.size, self.n0.size, self.n.shape[1], self.d.shape[1])
        self.sin0, self.cos0 = np.sin(theta), np.cos(theta)
        self.cost_sub = cos_snell(self.n0, self.nsub, self.sin0)

    def layer(self, j):
        rd = self.rd
        n, d = self.n[j], self.d[j]
        cost = cos_snell(self.n0, n, self.sin0)
        tpn = n * rd(6.283185307179586476925286766559)
        beta = ((tpn * d) * cost) / self.wvl
        dbdd = (tpn * cost) / self.wvl
        sinb, cosb = csincos(beta)
        return n, cost, sinb, cosb, dbdd

    def ends(self, p):
        eta0 = self.n0 / self.cos0 if p else self.n0 * self.cos0
        return eta0, admittance(self.nsub, self.cost_sub, p)

    def full(self, a):
        return np.broadcast_to(a, (self.K,)).copy()


def stack(indices, thicknesses, wvl, theta, nsub, n0, pol, dtype=np.complex128, t_convention=T_STACK):
    """pm_tf_stack: a dict of r, t, R, T (each (NP, K)), E, H ((NP, L + 1, K)) and A ((NP, L, K)); theta in radians"""
    op = _Operands(indices, thicknesses, wvl, theta, nsub, n0, dtype)
    cd, rd, K, L = op.cd, op.rd, op.K, op.L
    flags = pols_of(pol)
    NP = len(flags)
    out = dict(r=np.empty((NP, K), cd), t=np.empty((NP, K), cd), R=np.empty((NP, K), rd), T=np.empty((NP, K), rd),
               E=np.empty((NP, L + 1, K), cd), H=np.empty((NP, L + 1, K), cd), A=np.empty((NP, L, K), rd))
    ends = [op.ends(p) for p in flags]
    B = [op.full(np.ones(1, cd)) for _ in flags]
    C = [op.full(es) for _, es in ends]
    flux = [B[q].real * C[q].real + B[q].imag * C[q].imag for q in range(NP)]
    for q in range(NP):
        out['E'][q, L], out['H'][q, L] = B[q], C[q]
    for j in range(L - 1, -1, -1):
        n, cost, sinb, cosb, _ = op.layer(j)
        for q, p in enumerate(flags):
            eta = admittance(n, cost, p)
            m01, m10 = minus_i(sinb) / eta, minus_i(eta * sinb)
            nb = cosb * B[q] + m01 * C[q]
            nc = m10 * B[q] + cosb * C[q]
            B[q], C[q] = nb, nc
            out['E'][q, j], out['H'][q, j] = nb, nc
            f = nb.real * nc.real + nb.imag * nc.imag
            out['A'][q, j] = f - flux[q]
            flux[q] = f
    for q, p in enumerate(flags):
        eta0, etas = ends[q]
        den = eta0 * B[q] + C[q]
        rr = (eta0 * B[q] - C[q]) / den
        tt = (eta0 * rd(2)) / den
        out['r'][q] = rr
        out['t'][q] = tt * (_cx(op.cos0, np.zeros_like(op.cos0), cd) / op.cost_sub) if (t_convention == T_THINFILM and p) else tt
        t2 = tt.real * tt.real + tt.imag * tt.imag
        out['R'][q] = rr.real * rr.real + rr.imag * rr.imag
        out['T'][q] = etas.real / eta0.real * t2
        out['E'][q] = tt * out['E'][q]
        out['H'][q] = tt * out['H'][q]
        out['A'][q] = out['A'][q] * (t2 / eta0.real)
    return out


def thickness_grad(indices, thicknesses, wvl, theta, nsub, n0, pol, dR=None, dT=None, dtype=np.complex128, grad=None):
    """pm_tf_thickness_grad: (L,) real.  dR, dT: (K,) (shared by the polarisations) or (NP, K); `grad` is added to when given."""
    op = _Operands(indices, thicknesses, wvl, theta, nsub, n0, dtype)
    cd, rd, K, L = op.cd, op.rd, op.K, op.L
    flags = pols_of(pol)
    NP = len(flags)

    def seed(s):
        return None if s is None else np.broadcast_to(np.asarray(s).astype(rd).reshape(-1, K), (NP, K))
    dR, dT = seed(dR), seed(dT)
    ends = [op.ends(p) for p in flags]
    B = [op.full(np.ones(1, cd)) for _ in flags]
    C = [op.full(es) for _, es in ends]
    bB = np.empty((NP, L, K), cd)
    bC = np.empty((NP, L, K), cd)
    for j in range(L - 1, -1, -1):
        n, cost, sinb, cosb, _ = op.layer(j)
        for q, p in enumerate(flags):
            bB[q, j], bC[q, j] = B[q], C[q]
            eta = admittance(n, cost, p)
            m01, m10 = minus_i(sinb) / eta, minus_i(eta * sinb)
            B[q], C[q] = cosb * B[q] + m01 * C[q], m10 * B[q] + cosb * C[q]
    a0, a1 = [], []
    one = cd.type(1)
    for q, p in enumerate(flags):
        eta0, etas = ends[q]
        fac = etas.real / eta0.real
        den = eta0 * B[q] + C[q]
        rr = (eta0 * B[q] - C[q]) / den
        tt = (eta0 * rd(2)) / den
        rbar = rr * (rd(2) * dR[q]) if dR is not None else np.zeros(K, cd)
        tbar = tt * (rd(2) * fac * dT[q]) if dT is not None else np.zeros(K, cd)
        dr_dB, dr_dC = (eta0 * (one - rr)) / den, -((one + rr) / den)
        dt_dB, dt_dC = -((tt * eta0) / den), -(tt / den)
        a0.append(np.conj(dr_dB) * rbar + np.conj(dt_dB) * tbar)
        a1.append(np.conj(dr_dC) * rbar + np.conj(dt_dC) * tbar)
    out = np.zeros(L, rd)
    for j in range(L):
        n, cost, sinb, cosb, dbdd = op.layer(j)
        g = np.zeros(K, rd)
        for q, p in enumerate(flags):
            b0, b1 = np.conj(bB[q, j]), np.conj(bC[q, j])
            eta = admittance(n, cost, p)
            d00, d01, d10 = -sinb, minus_i(cosb) / eta, minus_i(eta * cosb)
            cb = np.conj(d00) * (a0[q] * b0) + np.conj(d01) * (a0[q] * b1) + np.conj(d10) * (a1[q] * b0) + np.conj(d00) * (a1[q] * b1)
            g = g + (cb.real * dbdd.real + cb.imag * dbdd.imag)
            m01, m10 = minus_i(sinb) / eta, minus_i(eta * sinb)
            a0[q], a1[q] = np.conj(cosb) * a0[q] + np.conj(m10) * a1[q], np.conj(m01) * a0[q] + np.conj(cosb) * a1[q]
        out[j] = rd(np.sum(g.astype(np.float64)))
    return out if grad is None else (np.asarray(grad, rd) + out)
