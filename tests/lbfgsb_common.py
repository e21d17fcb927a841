"""What tests/test_lbfgsb_host.py and tests/test_gpu_lbfgsb.py share: the fixture's problem and states (tests/golden/make_golden_lbfgsb.py),
the problem's fg in numpy and in torch, and the comparison of one step with the fixture."""
import os

import numpy as np

from conftest import GOLDEN, rel_max

TOL64, TOL32 = 1e-10, 5e-6      # the project's tolerances (tests/gpu_common.py)
TOL = {np.dtype(np.float64): TOL64, np.dtype(np.float32): TOL32}
MODES = {'unbounded': 0, 'projected': 1, 'truncated': 2}


def _load(name):
    return np.load(os.path.join(GOLDEN, name + '.npz'))


PROBLEM = _load('lbfgsb')
N = PROBLEM['t'].size
MEMORY = int(PROBLEM['memory'])
A = float(PROBLEM['A'])


def fg_numpy(dtype, A=A):
    """the fixture's problem; f and g are formed in double and g rounded to the data's type (fg is not what is under test)"""
    t, w = PROBLEM['t'], PROBLEM['w']

    def fg(x):
        x = np.asarray(x, dtype=np.float64)
        d = x - t
        e = np.diff(x)
        e3 = A * e ** 3
        g = w * d
        g[:-1] -= e3
        g[1:] += e3
        return float(0.5 * np.sum(w * d * d) + A / 4 * np.sum(e ** 4)), g.astype(dtype)
    return fg


def fg_torch(tdtype, f_on_device=True, A=A):
    """the same on the device; f comes back as a 0-d tensor (or, with f_on_device=False, as a Python float: a host read of fg's own)"""
    import torch
    t = torch.from_numpy(PROBLEM['t']).cuda()
    w = torch.from_numpy(PROBLEM['w']).cuda()

    def fg(x):
        x = x.to(torch.float64)
        d = x - t
        e = x[1:] - x[:-1]
        e3 = A * e ** 3
        g = w * d
        g[:-1] -= e3
        g[1:] += e3
        f = 0.5 * torch.sum(w * d * d) + A / 4 * torch.sum(e ** 4)
        return (f if f_on_device else float(f)), g.to(tdtype)
    return fg


def _group(z, prefix):
    return {key[len(prefix):]: z[key] for key in z.files if key.startswith(prefix)}


def _states():
    out = []
    for mode in ('free', 'bounded'):
        z = _load('lbfgsb_' + mode)
        for i in z['kept']:
            st = _group(z, f's{i}_')
            if mode == 'bounded':
                st['lo'], st['hi'] = np.full(N, float(PROBLEM['lo'])), np.full(N, float(PROBLEM['hi']))
            out.append((f'{mode}-{i}', st))
    z = _load('lbfgsb_hand')
    for i, name in enumerate(z['names']):
        out.append((f'hand-{i}-{str(name).replace(" ", "-")}', _group(z, f'h{i}_')))
    return out


STATES = _states()
STATE_IDS = [s[0] for s in STATES]


def logical(st):
    """(S, Y) of the state's k live pairs, oldest first, from the fixture's physical rows (the reference's _hist_slot)"""
    k, nxt = int(st['k']), int(st['hist_next'])
    rows = [(nxt + i) % MEMORY if k == MEMORY else i for i in range(k)]
    return st['S'][rows], st['Y'][rows]


def A_of(st):
    """the quartic term's weight: the problem's, or the state's own (the non-convex hand state)"""
    return float(st['A']) if 'A' in st else A


def bounds_of(st, dtype):
    if 'lo' not in st:
        return {}
    return dict(lower_bounds=st['lo'].astype(dtype), upper_bounds=st['hi'].astype(dtype))


def step_from(opt, st):
    """set the optimizer to the state and take one step -> None, or the stop's message"""
    S, Y = logical(st)
    opt._set_state(st['x'], S, Y)      # theta follows from the newest pair
    try:
        opt.step()
    except StopIteration as stop:
        return stop.value.message
    return None


def compare_step(label, st, stopped, x_new, pair, theta, metadata, evals, accepted, dtype, xc=None, c=None, free=None, tol=None,
                 want=None):
    """one step against the fixture's (or, with `want`, another result of the same layout): decisions exactly, arrays to tol.
    Prints the figures it asserts on and returns them."""
    want = st if want is None else want
    tol = TOL[np.dtype(dtype)] if tol is None else tol
    if 'stopped' in want:
        assert stopped == str(want['stopped']), (label, stopped)
        return {}
    assert stopped is None, (label, stopped)
    assert metadata['cauchy_breaks'] == int(want['cauchy_breaks']) and metadata['free_vars'] == int(want['free_vars']), (label, metadata)
    assert MODES[metadata['subspace_mode']] == int(want['mode']) and metadata['subspace_solved'] is True, (label, metadata)
    assert evals == len(want['evals']) and bool(accepted) == bool(want['accepted']), (label, evals, accepted)
    figs = dict(x_new=rel_max(x_new, want['x_new']), alpha=abs(metadata['alpha'] - float(want['alpha'])) / float(want['alpha']),
                theta=abs(theta - float(want['theta_new'])) / float(want['theta_new']))
    if accepted:
        figs['s'], figs['y'] = rel_max(pair[0], want['s_new']), rel_max(pair[1], want['y_new'])
    if xc is not None:
        figs['xc'] = rel_max(xc, want['xc'])
        assert np.array_equal(np.asarray(free, dtype=bool), np.asarray(want['free'], dtype=bool)), label
        if np.size(want['c']):
            figs['c'] = rel_max(c, want['c'])
    print(label, ' '.join(f'{k} {v:.2e}' for k, v in figs.items()))
    # c = W^T (xc - x) is printed, not held: it is not a result of the step, and its cancellation follows the conditioning of M.
    # A float32 figure above TOL32 is held to 4 x the reference's OWN float32-against-float64 gap on that quantity at that state
    # (the fixture's gap32_*): y = g_new - g cancels as the steps shrink, in the reference's float32 run exactly as here.
    ref_gap = {'x_new': 'gap32_x_new', 's': 'gap32_s_new', 'y': 'gap32_y_new', 'xc': 'gap32_xc', 'theta': 'gap32_theta_new'}
    for key, v in figs.items():
        if key == 'c':
            continue
        bound = tol
        if np.dtype(dtype) == np.float32 and v > tol and ref_gap.get(key) in st:
            bound = 4 * float(st[ref_gap[key]])
            print(f'  {label}: {key} {v:.2e} is above {tol:.0e}; the reference\'s own gap there is {bound / 4:.2e}, the bound {bound:.2e}')
        assert v <= bound, (label, key, v, bound)
    return figs
