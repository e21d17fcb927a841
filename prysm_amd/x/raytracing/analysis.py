"""Spot positions and transverse ray aberrations of a trace (prysm/x/raytracing/analysis.py: spot_positions,
transverse_ray_aberration), from torch operations on the trace's tensors.  The rest of the reference module (wavefronts, field
curves, chromatic focus, full-field maps) is not here."""
import torch

from .spencer_and_murty import valid_mask

__all__ = ['spot_positions', 'transverse_ray_aberration']

_AXES = {'x': 0, 'y': 1}


def _anchor(values, valid, reference, chief):
    """the value the others are measured from: the mean over the valid rays, or the chief ray's, which must be valid"""
    if reference == 'centroid':
        return values[valid].mean()
    if reference != 'chief':
        raise ValueError(f"reference must be 'centroid' or 'chief', got {reference!r}")
    if not bool(valid[chief]):
        raise ValueError('chief ray is invalid; pass reference="centroid" for an obscured or vignetted bundle')
    return values[chief]


def transverse_ray_aberration(P_hist, axis='y', chief_index=None, status=None, reference='chief'):
    """(pupil, delta) over the valid rays of a history P_hist (J + 1, N, 3): the launch coordinate along `axis` ('x' or 'y') and the
    landing coordinate on the last surface, each measured from `reference` -- 'chief', the ray `chief_index` (by default the launch
    ray nearest the centroid of the launch bundle), or 'centroid', the mean over the valid rays.  Valid: code OK in `status` (when
    given) and a finite landing."""
    if axis not in _AXES:
        raise ValueError(f"axis must be 'x' or 'y', got {axis!r}")
    launch, landing = P_hist[0], P_hist[-1]
    valid = valid_mask(status, landing)
    if chief_index is None:
        xy = launch[:, :2]
        chief_index = int(((xy - xy.mean(dim=0)) ** 2).sum(dim=1).argmin())
    pupil, image = launch[:, _AXES[axis]], landing[:, _AXES[axis]]
    if reference == 'chief':      # the pupil coordinate of the chief ray stands even where that ray did not arrive
        pupil_ref = pupil[chief_index]
    else:
        pupil_ref = _anchor(pupil, valid, reference, chief_index)
    return pupil[valid] - pupil_ref, image[valid] - _anchor(image, valid, reference, chief_index)


def spot_positions(P_final, status=None, origin=None):
    """(x, y) of the rays on the last surface, P_final (N, 3): with a `status` only the valid rays (code OK, finite position); `origin`
    'centroid' or an (x, y) pair is subtracted"""
    x, y = P_final[..., 0], P_final[..., 1]
    if status is not None:
        keep = valid_mask(status, P_final)
        x, y = x[keep], y[keep]
    if origin is None:
        return x, y
    if isinstance(origin, str):
        if origin.lower() != 'centroid':
            raise ValueError("origin string must be 'centroid'")
        origin = (torch.nanmean(x), torch.nanmean(y))
    return x - origin[0], y - origin[1]
