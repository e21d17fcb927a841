"""Helpers shared by tests/test_detector_host.py and tests/test_gpu_detector.py: the fixture's exposure cases and the statistics that
judge a sampler (thresholds are false-alarm rates, derived, not fitted)."""
import json

import numpy as np
import scipy.stats as st

MEANS = (0.03, 0.7, 4.0, 9.99, 10.0, 37.0, 1e3, 1e5)      # 9.99 / 10: the two sides of the sampler's switch point (detector_plan.PTRS_MIN)
ALARM = 1e-9


def chi_square_poisson(x, lam):
    """Pearson chi-square of integer draws x against Poisson(lam): one cell per count from the 1e-4 to the 1 - 1e-4 quantile, two tail
    cells, cells with expectation below 5 merged into one.  Returns (statistic, degrees of freedom)."""
    x = np.asarray(x).astype(np.int64).ravel()
    n = x.size
    lo, hi = int(st.poisson.ppf(1e-4, lam)), int(st.poisson.ppf(1 - 1e-4, lam))
    k = np.arange(lo, hi + 1)
    obs = np.bincount(np.clip(x, lo - 1, hi + 1) - (lo - 1), minlength=hi - lo + 3).astype(float)
    p = np.concatenate([[st.poisson.cdf(lo - 1, lam)], st.poisson.pmf(k, lam), [st.poisson.sf(hi, lam)]])
    e = p * n
    small = e < 5
    o = np.append(obs[~small], obs[small].sum())
    e = np.append(e[~small], e[small].sum())
    o, e = o[e > 0], e[e > 0]
    return float(((o - e) ** 2 / e).sum()), len(o) - 1


def assert_poisson(x, lam, what=''):
    x = np.asarray(x)
    assert np.all(x == np.floor(x)) and np.all(x >= 0), f'{what}: counts must be non-negative integers'
    chi, dof = chi_square_poisson(x, lam)
    bound = st.chi2.isf(ALARM, dof)
    dmean, mbound = abs(float(x.mean()) - lam), 6 * np.sqrt(lam / x.size)
    print(f'{what} mean {lam}: chi2 {chi:.1f} / {bound:.1f} (dof {dof}), |mean error| {dmean:.3g} / {mbound:.3g}')
    assert chi < bound, f'{what} mean {lam}: chi-square {chi:.1f} >= {bound:.1f} (dof {dof})'
    assert dmean < mbound, f'{what} mean {lam}: sample mean off by {dmean:.3g} >= {mbound:.3g}'


def ks_normal(z):
    """Kolmogorov-Smirnov statistic of z against N(0, 1) and its bound at the false-alarm rate (the DKW inequality)"""
    z = np.asarray(z, dtype=np.float64).ravel()
    return float(st.kstest(z, 'norm').statistic), float(np.sqrt(-0.5 * np.log(0.5 * ALARM) / z.size))


def corr(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float(abs((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum())))


def exposure_cases(g):
    """the fixture's Detector.expose cases: name -> (scalar parameters, arrays)"""
    out = {}
    for name, c in json.loads(str(g['cases'])).items():
        arr = {k: g[f'{name}_{k}'] for k in ('img', 'mean', 'shot', 'read', 'dn')}
        for k in ('prnu', 'dcnu', 'lut'):
            arr[k] = g[f'{name}_{k}'] if c[k] else None
        out[name] = (c, arr)
    return out


def detector_kwargs(c, arr):
    """keyword arguments of Detector / detector_plan.expose_walk of a fixture case"""
    return dict(dark_current=c['dark_current'], read_noise=c['read_noise'], bias=c['bias'], fwc=c['fwc'],
                conversion_gain=c['conversion_gain'], bits=c['bits'], exposure_time=c['exposure_time'], prnu=arr['prnu'],
                dcnu=arr['dcnu'], lut=arr['lut'])
