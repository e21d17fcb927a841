"""Generate the optym fixture (tests/golden/optym.npz) from the REFERENCE itself.

Run in the build container (the only place the reference exists), on the CPU:

    python tests/golden/make_golden_optym.py

Imports brandondube/prysm from PRYSM_REFERENCE and stores data only:
- costs, shape (37, 67), float32-representable inputs held as float64: `cost_I`, `cost_D` (= 1.7 I + 0.3 + 0.05 noise), `cost_y`
  (uniform in [0.05, 0.95]), `cost_yhat` (binary), `cost_mask` (keeps about 70 %), and per case `cost_<kind>[_masked]_f` / `_g` from the
  reference in float64, kind in mse, bgi, nll, nlls (the likelihood with the scalar target `cost_nll_scalar`);
- optimizers: the problem f = 1/2 sum w (x - t)^2, g = w (x - t) with `opt_t`, `opt_w`, `opt_x0` (n = 1027), alpha 0.05, default
  betas, 12 steps, `free` and `bounded` (-0.4 / 0.6):
  one file per optimizer and mode, `optym_<Name>_<mode>.npz` (all 12 x n float64 rows of every array would not fit one committed
  file), row k - 1 the result of step k:
  (a) `x`, `s1`, `s2`: the reference's float64 trajectory from the projected start clip(x0) (s1 = m or the accumulator, s2 = v; absent
      where an optimizer has none); bounded cases add `gstep`, `active` (bool) and `nbounded` of last_step_metadata;
  (b) `nx`, `ns1`, `ns2`: the result of ONE reference step in float64 with eps = float32's, taken from the float32 rounding of the
      previous row (of clip(x0) and a zero state for the first), under the float32 roundings of the bounds: the state before step k + 1 is float32(row k - 1), which is what
      the tests feed.  Only single steps from a stored state are comparable across precisions (eps is dtype-dependent and
      AdaMomentum adds it into v).
- activations: `act_x` (3 x standard normal), (a, x0, y0) = (1.7, 0.3, -0.2), `act_<name>_f`, `act_<name>_b`; softmax for K in 2, 5,
  64, 100 over 3 rows (the tests take row subsets and tile): `sm_x_<K>`, `sm_g_<K>`, `sm_f_<K>`, `sm_b_<K>`; Gumbel with `gum_u`, tau 0.7:
  `gum_x`, `gum_g`, `gum_f`, `gum_b`; DiscreteEncoder over 5 levels around a Softmax: `enc_x`, `enc_g`, `enc_f`, `enc_b`, `enc_d`;
- SpatialGradient2D on 1x1, 2x2, 3x3 and 67x130: `sg_<m>x<n>_in` and `_fx`, `_ax`, `_fy`, `_ay`.
"""
import os
import sys

import numpy as np

REF = os.environ.get('PRYSM_REFERENCE', '/root/reference')
sys.path.insert(0, REF)

from prysm.x.optym import activation as RA  # noqa: E402
from prysm.x.optym import cost as RC  # noqa: E402
from prysm.x.optym import operators as RO  # noqa: E402
from prysm.x.optym import optimizers as ROPT  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ('GradientDescent', 'AdaGrad', 'RMSProp', 'Adam', 'RAdam', 'AdaMomentum', 'Yogi')
STEPS = 12
EPS32 = float(np.finfo(np.float32).eps)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def state_of(opt):
    z = np.zeros_like(opt.x)
    if hasattr(opt, 'accumulator'):
        return opt.accumulator, z
    if hasattr(opt, 'm'):
        return opt.m, opt.v
    return z, z


def set_state(opt, s1, s2):
    if hasattr(opt, 'accumulator'):
        opt.accumulator = s1.copy()
    elif hasattr(opt, 'm'):
        opt.m, opt.v = s1.copy(), s2.copy()


def main():
    rng = np.random.default_rng(20261019)
    out = {}
    # ---- costs
    shape = (37, 67)
    I = f32(rng.uniform(0.1, 1.0, shape))  # noqa: E741
    D = f32(1.7 * I + 0.3 + 0.05 * rng.standard_normal(shape))
    y = f32(rng.uniform(0.05, 0.95, shape))
    yhat = (rng.random(shape) > 0.5).astype(np.float64)
    mask = rng.random(shape) < 0.7
    scalar = 1.0
    out.update(cost_I=I, cost_D=D, cost_y=y, cost_yhat=yhat, cost_mask=mask, cost_nll_scalar=np.float64(scalar))
    for key, fn, a, b in (('mse', RC.mean_square_error, I, D), ('bgi', RC.bias_and_gain_invariant_error, I, D),
                          ('nll', RC.negative_loglikelihood, y, yhat), ('nlls', RC.negative_loglikelihood, y, scalar)):
        for tag, m in (('', None), ('_masked', mask)):
            c, g = fn(a, b, mask=m)
            out[f'cost_{key}{tag}_f'] = np.float64(c)
            out[f'cost_{key}{tag}_g'] = np.asarray(g, dtype=np.float64)
    # ---- optimizers
    n = 1027
    t = f32(rng.standard_normal(n))
    w = f32(rng.uniform(0.5, 2.0, n))
    x0 = f32(rng.standard_normal(n))
    out.update(opt_t=t, opt_w=w, opt_x0=x0)

    def fg(x):
        d = x - t
        return 0.5 * np.sum(w * d * d), w * d

    nstate = dict(GradientDescent=0, AdaGrad=1, RMSProp=1)
    for name in NAMES:
        cls = getattr(ROPT, name)
        for mode, kw in (('free', {}), ('bounded', dict(lower_bounds=np.full(n, -0.4), upper_bounds=np.full(n, 0.6)))):
            traj = {}
            ns = nstate.get(name, 2)
            # (a) the float64 trajectory
            opt = cls(fg, x0.copy(), 0.05, **kw)
            start = opt.x.copy()
            xs, s1s, s2s, gst, act, nb = [], [], [], [], [], []
            for _ in range(STEPS):
                opt.step()
                a, b = state_of(opt)
                xs.append(np.asarray(opt.x, dtype=np.float64).copy()), s1s.append(a.copy()), s2s.append(b.copy())
                if kw:
                    md = opt.last_step_metadata
                    gst.append(md['projected_gradient'].copy()), act.append(md['active_bounds'].copy()), nb.append(md['bounded_variables'])
            traj['x'] = np.array(xs)
            if ns >= 1:
                traj['s1'] = np.array(s1s)
            if ns >= 2:
                traj['s2'] = np.array(s2s)
            if kw:
                traj['gstep'], traj['active'], traj['nbounded'] = np.array(gst), np.array(act), np.array(nb)
                assert 0.2 * n < nb[-1] < 0.9 * n, (name, nb)
            # (b) single float64 steps (eps of float32) from float32-rounded states
            opt = cls(fg, x0.copy(), 0.05, **{key: f32(b) for key, b in kw.items()})      # the bounds a float32 run sees
            if hasattr(opt, 'eps'):
                opt.eps = EPS32
            x, (s1, s2) = opt.x.copy(), state_of(opt)
            assert np.array_equal(f32(x), x)
            NX, NS1, NS2 = [], [], []
            for k in range(STEPS):
                opt.x = x.copy()
                set_state(opt, s1, s2)
                opt.iter = k
                opt.step()
                a, b = state_of(opt)
                NX.append(np.asarray(opt.x, dtype=np.float64).copy()), NS1.append(a.copy()), NS2.append(b.copy())
                x, s1, s2 = f32(opt.x), f32(a), f32(b)
            traj['nx'] = np.array(NX)
            if ns >= 1:
                traj['ns1'] = np.array(NS1)
            if ns >= 2:
                traj['ns2'] = np.array(NS2)
            path = os.path.join(HERE, f'optym_{name}_{mode}.npz')
            np.savez_compressed(path, **traj)
            assert os.path.getsize(path) < 1 << 20, path
            print(path, os.path.getsize(path), 'bytes')
    # RAdam's branch is crossed inside the 12 steps, far from a tie
    rhoinf = 2 / (1 - 0.999) - 1
    rho = [rhoinf - 2 * k * 0.999 ** k / (1 - 0.999 ** k) for k in range(1, STEPS + 1)]
    assert rho[4] < 4.999 and rho[5] > 5.9, rho
    # ---- activations
    ax = f32(3 * rng.standard_normal((37, 67)))
    out['act_x'] = ax
    for name in ('Tanh', 'Arctan', 'Softplus', 'Sigmoid'):
        node = getattr(RA, name)(1.7, 0.3, -0.2)
        out[f'act_{name}_f'], out[f'act_{name}_b'] = node.forward(ax), node.backprop(ax)
    for K in (2, 5, 64, 100):
        x, g = f32(3 * rng.standard_normal((3, K))), f32(rng.standard_normal((3, K)))
        sm = RA.Softmax()
        out[f'sm_x_{K}'], out[f'sm_g_{K}'], out[f'sm_f_{K}'] = x, g, sm.forward(x)
        out[f'sm_b_{K}'] = sm.backprop(g)
    x, g, u = f32(3 * rng.standard_normal((11, 7))), f32(rng.standard_normal((11, 7))), f32(rng.random((11, 7)))

    class FixedRng:
        def uniform(self, low, high, size):
            assert size == u.shape
            return u

    gs = RA.GumbelSoftmax(tau=0.7)
    gs.rng = FixedRng()
    out.update(gum_x=x, gum_g=g, gum_u=u, gum_f=gs.forward(x), gum_eps=np.float64(gs.eps))
    out['gum_b'] = gs.backprop(g)
    x, g = f32(3 * rng.standard_normal((13, 5))), f32(rng.standard_normal(13))
    enc = RA.DiscreteEncoder(RA.Softmax(), 5)
    out.update(enc_x=x, enc_g=g, enc_f=enc.forward(x))
    out['enc_b'] = enc.backprop(g)
    out['enc_d'] = enc.discretize(x)
    # ---- spatial gradient
    sg = RO.SpatialGradient2D()
    for m, n2 in ((1, 1), (2, 2), (3, 3), (67, 130)):
        a = f32(rng.standard_normal((m, n2)))
        p = f'sg_{m}x{n2}'
        out[p + '_in'] = a
        out[p + '_fx'], out[p + '_ax'], out[p + '_fy'], out[p + '_ay'] = sg.forward_x(a), sg.adjoint_x(a), sg.forward_y(a), sg.adjoint_y(a)
    path = os.path.join(HERE, 'optym.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
