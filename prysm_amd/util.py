"""Statistics of the valid elements of an array (prysm/util.py:7-97): mean, pv, rms, Sa, std.

Each is one call of pm_ifg_stats (csrc/interferogram.hip) -- four launches that leave the whole record on the device -- and one host
read of that record; the result is a Python float.  Valid means np.isfinite, as in the reference: NaN and +-inf are left out.  The sums
run in double whatever the array's precision, and the variance is two-pass.  There is no CPU path: a call without a device raises.

ecdf and sort_xy of the reference module are host conveniences on sorted copies and are not here.
"""
import numpy as np
import torch

from . import _lib as L
from . import _ops
from .conf import config

__all__ = ['mean', 'pv', 'rms', 'Sa', 'std']


def as_map(array):
    """an array of any shape as the 2-D real device tensor the statistics kernels read: float32 and float64 stay, anything else becomes
    config.precision; a strided 2-D view of a device tensor passes as it is"""
    if isinstance(array, torch.Tensor) and array.is_cuda and array.dim() == 2 and array.dtype in (torch.float32, torch.float64) \
            and array.stride(1) == 1 and (array.shape[0] <= 1 or array.stride(0) >= array.shape[1]):
        return array
    dt = array.dtype if isinstance(array, torch.Tensor) else L._NP2TORCH.get(np.asarray(array).dtype)
    if dt not in (torch.float32, torch.float64):
        dt = L.torch_dtype(config.compute_precision)
    t = L.as_device(array, dt)
    return t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])


def record(array):
    """the statistics record of an array on the host: L.PM_IFG_RECORD float64 values (one host read)"""
    return _ops.ifg_stats(as_map(array)).cpu().numpy()


def mean(array):
    """Mean of the valid elements (util.py:7-22)."""
    return float(record(array)[L.PM_IFG_MEAN])


def pv(array):
    """Peak-to-valley of the valid elements (util.py:25-40): both extrema are selections, so the result is exact in float64."""
    rec = record(array)
    return float(rec[L.PM_IFG_MAX] - rec[L.PM_IFG_MIN])


def rms(array):
    """Root mean square of the valid elements (util.py:43-58)."""
    return float(record(array)[L.PM_IFG_RMS])


def Sa(array):
    """Mean absolute deviation from the mean of the valid elements (util.py:61-78)."""
    return float(record(array)[L.PM_IFG_SA])


def std(array):
    """Standard deviation of the valid elements (util.py:81-97)."""
    return float(record(array)[L.PM_IFG_STD])
