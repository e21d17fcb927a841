"""Thin-film coating analysis on the device (the core of prysm/x/coatings).

Stack, stack_rt, internal_fields and RTA (stack.py), forward_eval / ForwardEval and thickness_gradient for R and T seeds (diff.py),
and the Reflectance and Transmittance terms with MeritFunction and as_merit (merit.py), on the kernels of csrc/thinfilm.hip;
prysm_amd/thinfilm_plan.py restates those in numpy.  A merit's value_and_grad stays on the device, so it drives the
prysm_amd.x.optym optimizers directly and can be captured in a graph.

Not built, each raising NotImplementedError with its name: the dA and dEsq seeds and the terms that need them, index_gradient,
field_at_depth, the matrix-level helpers, CoatingProblem and refine, needle synthesis, monitoring, rugate synthesis and the
materials catalogue (common_materials).
"""
from .diff import ForwardEval, forward_eval, index_gradient, thickness_gradient  # noqa: F401
from .merit import (  # noqa: F401
    FieldInLayer, FieldIntensityAtBoundary, LayerAbsorptance, MeritFunction, PeakFieldAtInterfaces, Reflectance, Transmittance, as_merit)
from .stack import (  # noqa: F401
    RTA, Stack, backward_products, field_at_depth, forward_products, internal_fields, stack_characteristic_matrices, stack_rt)

# the reference's names this package does not provide, by the module that holds them there
NOT_BUILT = {
    'CoatingProblem': 'problem', 'refine': 'refine', 'CoatingResult': 'refine',
    'needle_function': 'needle', 'insert_needle': 'needle', 'cleanup': 'needle', 'synthesize': 'needle', 'NeedleResult': 'needle',
    'monitoring_trace': 'monitoring', 'turning_points': 'monitoring', 'level_cut': 'monitoring', 'cutoff_levels': 'monitoring',
    'simulate_run': 'monitoring', 'monitoring_error_sensitivity': 'monitoring', 'choose_monitor_wavelength': 'monitoring',
    'quintic_taper': 'rugate', 'discretize_profile': 'rugate', 'rugate_period': 'rugate', 'notch_wavelength': 'rugate',
    'sinusoidal_rugate': 'rugate', 'apodize': 'rugate', 'rugate_from_target': 'rugate',
    'common_materials': 'common_materials',
}

__all__ = ['Stack', 'stack_characteristic_matrices', 'forward_products', 'backward_products', 'internal_fields', 'field_at_depth', 'RTA',
           'stack_rt', 'ForwardEval', 'forward_eval', 'thickness_gradient', 'index_gradient', 'Reflectance', 'Transmittance',
           'LayerAbsorptance', 'FieldIntensityAtBoundary', 'PeakFieldAtInterfaces', 'FieldInLayer', 'MeritFunction', 'as_merit']


class _NotBuilt:
    """stands where one of the reference's names would: calling it or reaching into it raises NotImplementedError"""

    def __init__(self, name):
        self.__dict__['_name'] = name

    def _refuse(self):
        name = self.__dict__['_name']
        raise NotImplementedError(f'prysm_amd.x.coatings.{name} (prysm/x/coatings/{NOT_BUILT[name]}.py) is not implemented')

    def __call__(self, *args, **kwargs):
        self._refuse()

    def __getattr__(self, attr):
        if attr.startswith('__'):
            raise AttributeError(attr)
        self._refuse()


def __getattr__(name):
    if name in NOT_BUILT:
        return _NotBuilt(name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
