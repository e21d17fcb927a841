"""csrc/optym.hip in numpy: the costs, the optimizer steps, the activations and the spatial gradient, with the same arithmetic as the
kernels (which are compiled without fused multiply-add contraction).  No device, no torch: this is what the CPU tests hold against the
reference's results and what documents the kernels' formulas.

- costs: every element is widened to float64, the sums are float64, the scalars (1/N, alpha, beta, R) are float64 and the results are
  rounded once to the data's dtype.  A mask is a predicate; nothing is compacted.  The bias-and-gain-invariant cost takes its covariance
  and variance from CENTRED data, as the reference does (Ihat = I - I.mean()): a first pass leaves the means, a second sums
  (I - Imean)(D - Dmean) and (I - Imean)^2.  The one-pass form sum(I D) - sum(I) Dmean loses (mean / spread)^2 eps of alpha to a pedestal,
  which is the very thing the cost is meant not to see.
- steps: arithmetic in the data's dtype, expression by expression as prysm/x/optym/optimizers.py writes it; the scalars that depend
  on the iteration number (`coefficients`) are float64 and rounded once where they meet the data.
- softmax: the row maximum is subtracted; the forward sums are in the data's dtype (the kernel adds them in a butterfly over the lanes
  of a row, numpy pairwise: the results agree to rounding, not to the bit); the backprop's sums and bracket are float64.
"""
import numpy as np

COST_MSE, COST_BGI, COST_NLL = 0, 1, 2
GD, ADAGRAD, RMSPROP, ADAM, RADAM, ADAMOMENTUM, YOGI = range(7)
TANH, ARCTAN, SOFTPLUS, SIGMOID = range(4)
FORWARD_X, ADJOINT_X, FORWARD_Y, ADJOINT_Y = range(4)

# launch constants of the cost passes (csrc/optym.hip kCostThreads, kCostWgs): a first-stage workgroup runs its grid-stride loop
# ceil(n / (COST_THREADS * COST_WGS)) times at most.  COST_SUMS: most sums of the first pass (N, sum I, sum D, sum D^2 of the bias-and-gain-
# invariant cost), COST_CENTRED: the sums of its centred pass, and one more of the gradient pass (sum raw_err^2)
COST_THREADS, COST_WGS, COST_SUMS, COST_CENTRED, COST_SCALARS = 256, 1024, 4, 2, 8


def cost_workspace_bytes():
    return 8 * (COST_SCALARS + COST_WGS * COST_SUMS + COST_WGS * COST_CENTRED + COST_WGS)


def cost(kind, M, D, mask=None):
    """(cost, grad) of pm_optym_cost: cost a 0-d array of M's dtype, grad of M's shape and dtype, zero where the mask is false"""
    M = np.asarray(M)
    dt = M.dtype
    m = M.astype(np.float64).ravel()
    d = np.broadcast_to(np.asarray(D, dtype=np.float64), M.shape).ravel()
    keep = np.ones(m.shape, dtype=bool) if mask is None else np.asarray(mask).astype(bool).ravel()
    mk, dk = m[keep], d[keep]          # the model may compact: the sums are the same numbers
    N = np.float64(mk.size)
    with np.errstate(all='ignore'):
        if kind == COST_MSE:
            inv = np.float64(1.0) / N
            diff = mk - dk
            c = np.sum(diff * diff) * inv
            gk = 2.0 * inv * diff
        elif kind == COST_NLL:
            inv = np.float64(1.0) / N
            c = -inv * np.sum(dk * np.log(mk) + (1.0 - dk) * np.log(1.0 - mk))
            gk = ((-dk / mk) + ((1.0 - dk) / (1.0 - mk))) * inv
        elif kind == COST_BGI:
            sI, sD, sDD = np.sum(mk), np.sum(dk), np.sum(dk * dk)
            Imean, Dmean = sI / N, sD / N
            ci, cd = mk - Imean, dk - Dmean
            alpha = np.sum(ci * cd) / np.sum(ci * ci)
            beta = Dmean - alpha * Imean
            R = np.float64(1.0) / sDD
            raw = (alpha * mk + beta) - dk
            c = R * np.sum(raw * raw)
            gk = 2.0 * R * alpha * raw
        else:
            raise ValueError(f'unknown cost kind {kind}')
    g = np.zeros(m.shape, dtype=np.float64)
    g[keep] = gk
    return np.asarray(c).astype(dt), g.astype(dt).reshape(M.shape)


def coefficients(kind, k, beta1, beta2):
    """pm_optym_advance: the eight float64 coefficients of step k"""
    b1k, b2k = float(beta1) ** k, float(beta2) ** k
    rho = r = flag = 0.0
    if kind == RADAM:
        rhoinf = 2.0 / (1.0 - beta2) - 1.0
        rho = rhoinf - (2.0 * k * b2k) / (1.0 - b2k)
        if rho >= 5.0:
            r = float(np.sqrt(((rho - 4.0) * (rho - 2.0) * rhoinf) / ((rhoinf - 4.0) * (rhoinf - 2.0) * rho)))
            flag = 1.0
    return np.array([1.0 - b1k, 1.0 - b2k, rho, r, flag, np.sqrt(1.0 - b2k), 0.0, 0.0])


def step(kind, k, x, g, s1=None, s2=None, lower=None, upper=None, alpha=0.05, beta1=0.9, beta2=0.999, eps=None, coef=None):
    """pm_optym_advance + pm_optym_step out of place: dict(x, s1, s2, x_prev, g_step, active).  k is the number of THIS step (from 1);
    beta1 is RMSProp's gamma.  coef: the eight coefficients of the step where they come from elsewhere (read back from the device, whose
    pow is not numpy's to the bit); what is left of the step is + - * / and sqrt in x's dtype."""
    x = np.asarray(x)
    T = x.dtype.type
    g = np.asarray(g, dtype=x.dtype)
    eps = T(np.finfo(x.dtype).eps if eps is None else eps)
    co = coefficients(kind, k, beta1, beta2) if coef is None else np.asarray(coef, dtype=np.float64)
    al, b1, ob1, b2, ob2 = T(alpha), T(beta1), T(1.0 - beta1), T(beta2), T(1.0 - beta2)
    bounded = lower is not None
    gs = g
    if bounded:
        lower, upper = np.asarray(lower, dtype=x.dtype), np.asarray(upper, dtype=x.dtype)
        blocked = (np.isfinite(lower) & (x <= lower) & (g > 0)) | (np.isfinite(upper) & (x >= upper) & (g < 0))
        gs = np.where(blocked, T(0), g)
    with np.errstate(all='ignore'):
        if kind == GD:
            xn = x - al * gs
        elif kind == ADAGRAD:
            s1 = s1 + gs * gs
            xn = x - al * gs / (np.sqrt(s1) + eps)
        elif kind == RMSPROP:
            s1 = b1 * s1 + ob1 * (gs * gs)
            xn = x - al * gs / (np.sqrt(s1) + eps)
        elif kind == ADAM:
            s1 = b1 * s1 + ob1 * gs
            s2 = b2 * s2 + ob2 * (gs * gs)
            xn = x - al * (s1 / T(co[0])) / (np.sqrt(s2 / T(co[1])) + eps)
        elif kind == RADAM:
            s1 = b1 * s1 + ob1 * gs
            s2 = b2 * s2 + ob2 * (gs * gs)
            if co[4] != 0.0:
                xn = x - T(float(alpha) * co[3]) * (s1 / T(co[0])) * (T(co[5]) / (np.sqrt(s2) + eps))
            else:
                xn = x - al * gs
        elif kind == ADAMOMENTUM:
            s1 = b1 * s1 + ob1 * gs
            s2 = b2 * s2 + ob2 * (s1 * s1) + eps
            xn = x - al * (s1 / T(co[0])) / np.sqrt(s2 / T(co[1]))
        elif kind == YOGI:
            gsq = gs * gs
            s1 = b1 * s1 + ob1 * gs
            s2 = s2 - ob2 * np.sign(s2 - gsq) * gsq
            xn = x - al * s1 / (np.sqrt(np.sqrt(s2 + eps)) + eps)
        else:
            raise ValueError(f'unknown optimizer kind {kind}')
    out = dict(x_prev=x, s1=s1, s2=s2, g_step=None, active=None)
    if bounded:
        xn = np.minimum(np.maximum(xn, lower), upper)
        out['g_step'] = gs
        out['active'] = (np.isfinite(lower) & (xn <= lower)) | (np.isfinite(upper) & (xn >= upper))
    out['x'] = xn.astype(x.dtype)
    return out


def activation(kind, x, a=1, x0=0, y0=0, backprop=False):
    """pm_optym_activation"""
    x = np.asarray(x)
    T = x.dtype.type
    a_, m2a, ma, x0, y0, one = T(a), T(-2.0 * a), T(-a), T(x0), T(y0), T(1)
    xs = x - x0

    def forward():
        if kind == TANH:
            return T(2) / (one + np.exp(m2a * xs)) - one + y0
        if kind == ARCTAN:
            return np.arctan(a_ * xs) + y0
        if kind == SOFTPLUS:
            return np.log(one + np.exp(a_ * xs)) + y0
        if kind == SIGMOID:
            return (one / (one + np.exp(ma * xs))) + y0
        raise ValueError(f'unknown activation kind {kind}')

    with np.errstate(over='ignore'):
        if not backprop:
            return forward()
        if kind == TANH:
            fx = forward() - y0
            return a_ * (one - fx * fx)
        if kind == ARCTAN:
            u = a_ * xs
            return a_ / (u * u + one)
        if kind == SOFTPLUS:
            return a_ / (one + np.exp(ma * xs))
        sig = forward() - y0
        return a_ * sig * (one - sig)


def softmax_group(K):
    """lanes a row of K logits is spread over: the smallest power of two that holds K, at most 64"""
    G = 1
    while G < K and G < 64:
        G *= 2
    return G


def gumbel_logits(x, u, tau, eps):
    x = np.asarray(x)
    T = x.dtype.type
    return (x + (-np.log(-np.log(np.asarray(u, dtype=x.dtype) + T(eps)) + T(eps)))) / T(tau)


def softmax(x, u=None, tau=1.0, eps=0.0):
    """pm_optym_softmax over the last axis"""
    x = np.asarray(x)
    if u is not None:
        x = gumbel_logits(x, u, tau, eps)
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def softmax_backprop(y, grad, tau=1.0):
    """pm_optym_softmax_backprop over the last axis: y_k (g_k S - sum_j g_j y_j) / tau with S = sum_j y_j, everything in float64 and
    one rounding to y's dtype.  S is 1 up to the rounding of the stored y; with it the bracket is sum_j y_j (g_k - g_j), which does not
    cancel on a saturated row the way the reference's g_k - sum_j g_j y_j does."""
    y = np.asarray(y)
    y64, g64 = y.astype(np.float64), np.asarray(grad, dtype=np.float64)
    dot = (g64 * y64).sum(axis=-1, keepdims=True)
    S = y64.sum(axis=-1, keepdims=True)
    return (y64 * (g64 * S - dot) / float(tau)).astype(y.dtype)


def spatial_gradient(op, a):
    """pm_optym_spatial_gradient, as the gathers the kernels are"""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError('a must be 2-D')
    if op in (FORWARD_Y, ADJOINT_Y):
        return spatial_gradient(op - 2, a.T).T
    out = np.zeros_like(a)
    end = a.shape[1]
    if op == FORWARD_X:
        out[:, 1:end - 1] = a[:, 2:end] - a[:, 1:end - 1]
    else:
        out[:, 1:end - 1] = out[:, 1:end - 1] - a[:, 1:end - 1]
        out[:, 2:end] = out[:, 2:end] + a[:, 1:end - 1]
    return out
