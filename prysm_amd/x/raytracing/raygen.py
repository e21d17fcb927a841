"""Ray fans and grids (prysm/x/raytracing/raygen.py), as device tensors built from torch operations.

generate_collimated_ray_fan, generate_collimated_rect_ray_grid and generate_finite_ray_fan return P and S of (N, 3) in
config.precision; concat_rayfans and split_rayfans join and split bundles.  The hexapolar and spiral grids and clip_to_aperture are
not here.
"""
import math

import torch

from ... import _lib as L
from ...conf import config
from ...coordinates import make_rotation_matrix, promote_3d_point

__all__ = ['generate_collimated_ray_fan', 'generate_collimated_rect_ray_grid', 'generate_finite_ray_fan', 'concat_rayfans', 'split_rayfans']


def _dtype():
    return L.torch_dtype(config.compute_precision)


def sample_axis(distribution, lo, hi, n, dtype=None):
    """n samples from lo to hi: 'uniform', 'random', or 'cheby' (Chebyshev-Gauss-Lobatto nodes) (coordinates.py:128-165)"""
    dtype = _dtype() if dtype is None else dtype
    dev = L.device()
    if n == 1:
        return torch.tensor([(lo + hi) / 2.0], dtype=dtype, device=dev)
    distribution = distribution.lower()
    if distribution == 'uniform':
        return torch.linspace(lo, hi, n, dtype=torch.float64, device=dev).to(dtype)
    if distribution == 'random':
        return (lo + (hi - lo) * torch.rand(n, dtype=torch.float64, device=dev)).to(dtype)
    if distribution == 'cheby':
        nodes = torch.cos(torch.arange(n, dtype=torch.float64, device=dev) * (math.pi / (n - 1)))
        return ((lo + hi) / 2.0 - (hi - lo) / 2.0 * nodes).to(dtype)
    raise ValueError(f"unknown distribution {distribution!r}; expected 'uniform', 'random', or 'cheby'")


def _make_collimated_S(npoints, yangle=0, xangle=0):
    """the (npoints, 3) direction cosines of collimated rays: the z axis turned by (0, yangle, -xangle)"""
    R = make_rotation_matrix((0, yangle, -xangle))
    S = torch.from_numpy(R[:, 2].copy()).to(L.device()).to(_dtype())
    return S[None, :].expand(npoints, 3)


def concat_rayfans(*rayfans):
    """merge the (P, S) pairs of several generators into one bundle"""
    return torch.cat([p for p, _ in rayfans], dim=0), torch.cat([s for _, s in rayfans], dim=0)


def split_rayfans(P, chunksizes, S=None):
    """views of P (and S) -- a bundle or its history's rows -- that are the chunks concat_rayfans joined"""
    if P.shape[0] != sum(chunksizes):
        raise ValueError('P is not sum(chunksizes) in length')

    def chunks(a):
        out, low = [], 0
        for size in chunksizes:
            out.append(a[low:low + size])
            low += size
        return out
    return chunks(P) if S is None else (chunks(P), chunks(S))


def generate_collimated_ray_fan(nrays, maxr, z=0, minr=None, azimuth=90, yangle=0, xangle=0, distribution='uniform'):
    """a 1-D fan of nrays collimated rays from radius minr (-maxr) to maxr along `azimuth` (degrees; 0 an X fan, 90 a Y fan)"""
    if minr is None:
        minr = -maxr
    S = _make_collimated_S(nrays, yangle=yangle, xangle=xangle)
    r = sample_axis(distribution, minr, maxr, nrays)
    t = math.radians(azimuth)
    return torch.stack([r * math.cos(t), r * math.sin(t), torch.full_like(r, z)], dim=1), S


def generate_collimated_rect_ray_grid(nrays, maxx, z=0, minx=None, maxy=None, miny=None, yangle=0, xangle=0, distribution='uniform'):
    """an nrays x nrays grid of collimated rays over [minx, maxx] x [miny, maxy], x fastest"""
    if minx is None:
        minx = -maxx
    if maxy is None:
        maxy = maxx
    if miny is None:
        miny = -maxy
    S = _make_collimated_S(nrays * nrays, yangle=yangle, xangle=xangle)
    x = sample_axis(distribution, minx, maxx, nrays)
    y = sample_axis(distribution, miny, maxy, nrays)
    xx, yy = x[None, :].expand(nrays, nrays).reshape(-1), y[:, None].expand(nrays, nrays).reshape(-1)
    return torch.stack([xx, yy, torch.full_like(xx, z)], dim=1), S


def generate_finite_ray_fan(nrays, na, P=0, min_na=None, azimuth=90, yangle=0, xangle=0, n=1, distribution='uniform'):
    """a 1-D fan of nrays rays from the point P filling the numerical aperture min_na (-na) .. na in a medium of index n"""
    P = torch.from_numpy(promote_3d_point(P, dtype=config.compute_precision)).to(L.device())
    if min_na is None:
        min_na = -na
    t = sample_axis(distribution, math.asin(min_na / n), math.asin(na / n), nrays)
    l = torch.sin(t)  # noqa: E741
    m = torch.sqrt(1 - l * l)
    k = torch.zeros_like(l)
    if azimuth == 0:
        k, l = l, k  # noqa: E741
    S = torch.stack([k, l, m], dim=1)
    if yangle != 0 or xangle != 0:
        R = torch.from_numpy(make_rotation_matrix((0, yangle, -xangle))).to(S.device).to(S.dtype)
        S = S @ R.T
    return P[None, :].expand(nrays, 3), S
