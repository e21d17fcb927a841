"""Generate the L-BFGS-B fixtures (tests/golden/lbfgsb.npz, lbfgsb_free.npz, lbfgsb_bounded.npz, lbfgsb_hand.npz) from the REFERENCE.

Run in the build container (the only place the reference exists), on the CPU:

    python tests/golden/make_golden_lbfgsb.py

Imports brandondube/prysm from PRYSM_REFERENCE and stores data only.

lbfgsb.npz also holds, per scalar function of tests/lbfgsb_linesearch_cases.py, what the reference's _strong_wolfe_lean does on it:
`ls_<name>_alphas` (every alpha it evaluates, in order) and `ls_<name>_result` (the accepted alpha, NaN for a failed search).

The problem (lbfgsb.npz): n = 1027, f = 1/2 sum w (x - t)^2 + (A / 4) sum (x[i+1] - x[i])^4, A = 0.3, t ~ N(0, 1), w ~ U(0.5, 20),
x0 ~ N(0, 1) (seed 1), memory 5; `free`, and `bounded` with the float32 roundings of -0.4 / 0.6 (a float32 state on a bound is
then ON it in the float64 step too) and the start clipped.  `xstar_free` / `xstar_bounded`: the
reference's x after 200 float64 steps.

States, one group `s<i>_*` per state in lbfgsb_<mode>.npz: the reference's float64 run is stopped before iteration i and x, S, Y (the
PHYSICAL rows) are ROUNDED TO FLOAT32 and stored as float32 with k and hist_next (theta is not part of the state: it is
(y . y) / (s . y) of the newest stored pair, 1 without one; `theta` holds it in double for information); then ONE reference float64 step (with
float32's eps in the curvature test) is taken from that rounded state and its result stored in float64: x_new, the new pair s_new /
y_new (zeros and accepted = 0 when the curvature test refused it), theta_new, alpha, free_vars, cauchy_breaks, mode (0 unbounded,
1 projected, 2 truncated), evals (the alphas the search evaluated) and for bounded steps xc, c, free (the mask) and zeros (the count
of t_i = 0).  `gap32_<quantity>`: the reference's own float32-against-float64 gap (rel_max) on x_new, s_new, y_new, xc and theta_new at
that state, the float32 step taken with a gradient rounded to float32.

Where the cases come from:
- iterations 0 .. 13 of both runs: k = 0 (iteration 0), 0 < k < m (1 .. 4), k = m with hist_next = 0 before any wrap (5), the ring
  wrapped with hist_next = 1 .. 4 (6 .. 9), the hist_next = 0 wrap (10), and on (11 .. 13).
- free iteration 0 is the step whose search goes through zoom (alpha = 0.063).
- bounded iteration 0 is taken from ANOTHER start (seed BOUNDED_K0_SEED): from the seed-1 start the reference's float32 and float64
  steps disagree on the number of breakpoints (948 against 949).  Its minimiser lies beyond the first chunk of 64 positive breakpoints
  (asserted below).
- lbfgsb_hand.npz, states built by hand on the reference object (each carries its own bounds `lo`, `hi`):
    h0 `subset box`: k = 0 at the clipped start, bounds only on 150 variables whose breakpoints lie in (0, 0.5): every finite
       breakpoint is visited and the path is exhausted (K = n_active = 150) in the second chunk (64, then 86), 877 variables stay
       free, and the search goes through zoom under bounds (4 evaluations);
    h1 `fixed box`: lo = hi = x: every variable is at a bound with t_i = 0, the direction is zero, the stop is 'no descent direction'.
    h2 `refused pair`: the clipped start with k = 0 under the usual box, but with A = -20 (stored as `A`): the objective is not
       convex, the search accepts alpha = 1 at the cap, s . y < 0 and the curvature test refuses the pair;
    h3 `truncated`: everything fixed (lo = hi = x) but two variables a, b that one stored pair couples: a sits just below its upper
       bound with the gradient pushing it up, b near its own minimum; the projected subspace direction is not descent, so the
       step falls back to BLNZ truncation (subspace_mode 'truncated') with alpha_max < 1, where the search's first trial, at that cap, is accepted.  Found
       by a seeded random search over (a, b, the distances, the pair) on the reference, the first draw that truncates, on which
       both precisions agree and whose own float32-against-float64 gap on x_new is below 1e-6.

The condition on inputs: each stored step is ALSO taken in the reference at float32, and a state is kept only if cauchy_breaks,
subspace_mode, the number of evaluations and the evaluated alphas (to 1e-3) agree between the two precisions.  The alpha sequence
stands in for the search's branch sequence: every branch (bracket by increase or slope, doubling, the pinned cap, the cubic,
quadratic or bisection step of zoom) puts a different next alpha, so two runs that evaluate the same alphas took the same branches.  Nothing else is
dropped; at least 10 states per mode must survive (asserted).
"""
import os
import sys

import numpy as np

REF = os.environ.get('PRYSM_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

from prysm.x.optym import _prysm_lbfgsb as RL  # noqa: E402

from lbfgsb_linesearch_cases import CASES  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
N, MEMORY, A = 1027, 5, 0.3
LO, HI = float(np.float32(-0.4)), float(np.float32(0.6))      # the bounds a float32 run sees, in every run here
ITERS = 14
EPS32 = float(np.finfo(np.float32).eps)
BOUNDED_K0_SEED = 2
MODES = {'unbounded': 0, 'projected': 1, 'truncated': 2}

_alphas = []
_orig_eval = RL._wolfe_eval


def _logging_eval(problem, xk, pk, alpha, dot):
    _alphas.append(float(alpha))
    return _orig_eval(problem, xk, pk, alpha, dot)


RL._wolfe_eval = _logging_eval


def f32(a):
    return np.asarray(a, dtype=np.float32)


def make_fg(t, w, A=A):
    def fg(x):
        d = x - t
        e = np.diff(x)
        e3 = A * e ** 3
        g = w * d
        g[:-1] -= e3
        g[1:] += e3
        return 0.5 * np.sum(w * d * d) + A / 4 * np.sum(e ** 4), g
    return fg


def one_step(fg, state, dtype, lo, hi):
    """one reference step in `dtype` from a stored (float32) state -> dict of results, or the stop's reason"""
    x = state['x'].astype(dtype)
    kw = {} if lo is None else dict(lower_bounds=lo.astype(dtype), upper_bounds=hi.astype(dtype))
    def fg_typed(v):      # an objective of the run's own precision: g comes back in the data's type
        f, g = fg(v)
        return f, g.astype(dtype)
    opt = RL.PrysmLBFGSB(fg_typed, x.copy(), memory=MEMORY, **kw)
    k = int(state['k'])
    opt.S[:], opt.Y[:] = state['S'].astype(dtype), state['Y'].astype(dtype)
    opt._k, opt._hist_next = k, int(state['hist_next'])
    rows = [opt._hist_slot(i) for i in range(k)]
    for r in rows:
        opt.ys[r] = opt.S[r] @ opt.Y[r]
        opt.rho[r] = 1 / opt.ys[r]
    if k:       # theta as the run's own update would have left it: (y . y) / (s . y) of the newest pair, in the run's type
        s_last, y_last = opt.S[rows[-1]], opt.Y[rows[-1]]
        opt.theta = np.asarray(float(y_last @ y_last) / float(s_last @ y_last), dtype=dtype)
    opt._eps = EPS32
    seen = {}
    cauchy = opt._cauchy

    def spy(g, *a, **kwa):
        xc, c, free = cauchy(g, *a, **kwa)
        t, _ = opt._compute_breakpoints(g)
        seen.update(xc=xc.copy(), c=np.array(c, dtype=np.float64), free=free.copy(), zeros=int(np.sum(t == 0)))
        return xc, c, free
    opt._cauchy = spy
    before = (opt._k, opt._hist_next)
    del _alphas[:]
    try:
        opt.step()
    except StopIteration as stop:
        return dict(stopped=stop.value.message, evals=np.array(_alphas), **seen)
    md = opt.last_step_metadata
    accepted = (opt._k, opt._hist_next) != before
    slot = (opt._hist_next - 1) % MEMORY if before[0] == MEMORY else before[0]
    out = dict(x_new=np.asarray(opt.x, dtype=np.float64), accepted=int(accepted), theta_new=float(opt.theta), alpha=md['alpha'],
               free_vars=md['free_vars'], cauchy_breaks=md['cauchy_breaks'], mode=MODES[md['subspace_mode']], evals=np.array(_alphas))
    out['s_new'] = np.asarray(opt.S[slot], dtype=np.float64) if accepted else np.zeros(N)
    out['y_new'] = np.asarray(opt.Y[slot], dtype=np.float64) if accepted else np.zeros(N)
    for key, v in seen.items():
        out[key] = np.asarray(v, dtype=np.float64) if key in ('xc', 'c') else v
    return out


def agree(a, b):
    if ('stopped' in a) != ('stopped' in b):
        return False
    if 'stopped' in a:
        return a['stopped'] == b['stopped']
    return (a['cauchy_breaks'] == b['cauchy_breaks'] and a['mode'] == b['mode'] and len(a['evals']) == len(b['evals'])
            and np.allclose(a['evals'], b['evals'], rtol=1e-3, atol=0))


def gaps_of(r32, r64):
    """the reference's own float32-against-float64 gap (rel_max) per compared quantity"""
    out = {}
    for key in ('x_new', 's_new', 'y_new', 'xc'):
        if key in r64 and np.max(np.abs(r64[key])) > 0:
            out['gap32_' + key] = float(np.max(np.abs(r32[key] - r64[key])) / np.max(np.abs(r64[key])))
    if 'theta_new' in r64:
        out['gap32_theta_new'] = abs(r32['theta_new'] - r64['theta_new']) / r64['theta_new']
    return out


def state_of(opt):
    return dict(x=f32(opt.x), S=f32(opt.S), Y=f32(opt.Y), k=opt._k, hist_next=opt._hist_next)


def theta_of(state):
    k = state['k']
    if k == 0:
        return np.float64(1)
    last = (state['hist_next'] - 1) % MEMORY if k == MEMORY else k - 1
    s, y = state['S'][last].astype(np.float64), state['Y'][last].astype(np.float64)
    return np.float64((y @ y) / (s @ y))


def main():
    rng = np.random.default_rng(1)
    t = f32(rng.standard_normal(N)).astype(np.float64)
    w = f32(rng.uniform(0.5, 20, N)).astype(np.float64)
    x0 = f32(rng.standard_normal(N)).astype(np.float64)
    x0b = f32(np.random.default_rng(BOUNDED_K0_SEED).standard_normal(N)).astype(np.float64)
    fg = make_fg(t, w)
    lo, hi = np.full(N, LO), np.full(N, HI)
    common = dict(t=t, w=w, x0=x0, x0_bounded_k0=x0b, A=np.float64(A), lo=np.float64(LO), hi=np.float64(HI), memory=np.int64(MEMORY))
    for mode, kw in (('free', {}), ('bounded', dict(lower_bounds=lo, upper_bounds=hi))):
        b = (lo, hi) if kw else (None, None)
        start = np.clip(x0, LO, HI) if kw else x0
        opt = RL.PrysmLBFGSB(lambda v: fg(v), start.copy(), memory=MEMORY, **kw)
        states = []
        for i in range(ITERS):
            st = state_of(opt)
            if kw and i == 0:
                st['x'] = f32(np.clip(x0b, LO, HI))
            states.append(st)
            opt.step()
        for _ in range(200 - ITERS):
            try:
                opt.step()
            except StopIteration:
                break
        common['xstar_' + mode] = np.asarray(opt.x, dtype=np.float64)
        out, kept = {}, []
        for i, st in enumerate(states):
            st['theta'] = theta_of(st)
            r64, r32 = one_step(fg, st, np.float64, *b), one_step(fg, st, np.float32, *b)
            ok = agree(r64, r32)
            gaps = gaps_of(r32, r64)
            gap = gaps['gap32_x_new']
            print(mode, i, 'k', st['k'], 'next', st['hist_next'], 'kept' if ok else 'DROPPED', 'breaks', r64['cauchy_breaks'], r32['cauchy_breaks'],
                  'evals', len(r64['evals']), 'alpha %.4g' % r64['alpha'], 'f32-f64 gap %.2e' % gap)
            if not ok:
                continue
            kept.append(i)
            for key, v in {**st, **r64, **gaps}.items():
                out[f's{i}_{key}'] = np.asarray(v)
        out['kept'] = np.array(kept)
        assert len(kept) >= 10, (mode, kept)
        assert 0 in kept, 'the k = 0 state must hold'
        if kw:
            assert out['s0_cauchy_breaks'] - out['s0_zeros'] > 64, 'the bounded k = 0 minimiser must lie beyond the first chunk'
        else:
            assert len(out['s0_evals']) > 1 and abs(out['s0_alpha'] - 0.063) < 1e-3, 'the first free step goes through zoom'
        path = os.path.join(HERE, f'lbfgsb_{mode}.npz')
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 1 << 20, path
        print(path, os.path.getsize(path), 'bytes')
    # ---- states built by hand
    hand = {}
    xs = f32(np.clip(x0, LO, HI))
    empty = dict(S=np.zeros((MEMORY, N), np.float32), Y=np.zeros((MEMORY, N), np.float32), k=0, hist_next=0)
    g0 = fg(xs.astype(np.float64))[1]
    with np.errstate(all='ignore'):
        tb = np.where(g0 > 0, (xs - lo) / g0, np.where(g0 < 0, (xs - hi) / g0, np.inf))
    J = np.nonzero((tb > 0) & (tb < 0.5))[0][:150]
    lsub, usub = np.full(N, -np.inf), np.full(N, np.inf)
    lsub[J], usub[J] = LO, HI
    cases = [('subset box', dict(x=xs, theta=np.float64(1), **empty), lsub, usub),
             ('fixed box', dict(x=xs, theta=np.float64(1), **empty), xs.astype(np.float64), xs.astype(np.float64))]
    cases = [c + (A,) for c in cases]
    cases.append(('refused pair', dict(x=xs, theta=np.float64(1), **empty), lo, hi, -20.0))
    # the truncated state: a seeded search (see the docstring)
    r = np.random.default_rng(7)
    cands_a = [i for i in range(5, N - 5) if t[i] > HI + 0.3]
    cands_b = [i for i in range(5, N - 5) if LO + 0.2 < t[i] < HI - 0.2]
    for trial in range(5000):
        a_, b_ = int(r.choice(cands_a)), int(r.choice(cands_b))
        if abs(a_ - b_) < 3:
            continue
        x = xs.astype(np.float64).copy()
        delta, eps_ = 10 ** r.uniform(-3, -1.3), 10 ** r.uniform(-3, -0.5)
        x[a_], x[b_] = HI - delta, t[b_] + eps_ / w[b_] * r.choice([1, -1])
        x = f32(x)
        l, u = x.astype(np.float64).copy(), x.astype(np.float64).copy()
        l[[a_, b_]], u[[a_, b_]] = LO, HI
        S, Y = np.zeros((MEMORY, N), np.float32), np.zeros((MEMORY, N), np.float32)
        sv, yv = r.standard_normal(2), r.standard_normal(2) * 10 ** r.uniform(-1, 1.5)
        if sv @ yv <= 0.05 * np.linalg.norm(sv) * np.linalg.norm(yv):
            continue
        S[0, [a_, b_]], Y[0, [a_, b_]] = sv, yv
        st = dict(x=x, S=S, Y=Y, k=1, hist_next=0)
        st['theta'] = theta_of(st)
        r64 = one_step(fg, st, np.float64, l, u)
        if r64.get('mode') != 2:
            continue
        r32 = one_step(fg, st, np.float32, l, u)
        if agree(r64, r32) and gaps_of(r32, r64)['gap32_x_new'] < 1e-6:
            print('truncated state: trial', trial, 'variables', a_, b_)
            cases.append(('truncated', st, l, u, A))
            break
    for i, (name, st, l, u, a_obj) in enumerate(cases):
        fgi = make_fg(t, w, a_obj)
        r64, r32 = one_step(fgi, st, np.float64, l, u), one_step(fgi, st, np.float32, l, u)
        assert agree(r64, r32), name
        print('hand', i, name, {k: v for k, v in r64.items() if np.ndim(v) == 0})
        for key, v in {**st, **r64, **gaps_of(r32, r64), 'lo': l, 'hi': u, 'A': a_obj}.items():
            hand[f'h{i}_{key}'] = np.asarray(v)
    assert hand['h2_accepted'] == 0 and hand['h2_alpha'] == 1.0 and 'stopped' not in [k[3:] for k in hand if k.startswith('h2_')]
    assert hand['h3_mode'] == 2 and hand['h3_alpha'] < 1.0 and len(hand['h3_evals']) == 1 and hand['h3_accepted'] == 1
    assert hand['h0_cauchy_breaks'] == 150 and hand['h0_free_vars'] == N - 150 and hand['h0_zeros'] == 0 and len(hand['h0_evals']) == 4
    assert str(hand['h1_stopped']) == 'no descent direction'
    hand['names'] = np.array([c[0] for c in cases])
    path = os.path.join(HERE, 'lbfgsb_hand.npz')
    np.savez_compressed(path, **hand)
    print(path, os.path.getsize(path), 'bytes')
    # ---- the reference's search on the scalar functions of tests/lbfgsb_linesearch_cases.py
    for name, (phi, maxalpha, c2, maxiter) in CASES.items():
        class Scalar:
            @staticmethod
            def fg(x):
                f, d = phi(float(x[0]))
                return f, np.array([d])
        f0, d0 = phi(0.0)
        del _alphas[:]
        alpha = RL._strong_wolfe_lean(Scalar, np.zeros(1), np.ones(1), fg_at_xk=(f0, np.array([d0])), maxalpha=maxalpha, c1=1e-4, c2=c2,
                                      maxiter=maxiter)[0]
        common[f'ls_{name}_alphas'] = np.array(_alphas)
        common[f'ls_{name}_result'] = np.float64(np.nan if alpha is None else alpha)
        print('line search', name, alpha, len(_alphas))
    path = os.path.join(HERE, 'lbfgsb.npz')
    np.savez_compressed(path, **common)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
