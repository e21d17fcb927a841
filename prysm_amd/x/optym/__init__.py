"""Optimization primitives on the device (prysm/x/optym): costs, activations, first-order optimizers, L-BFGS-B and their governors.

One iteration of a gradient-based model -- the model, a cost, the adjoints, an optimizer step -- stays on the device with no host
read and can be captured with prysm_amd.graph.capture.  csrc/optym.hip holds the kernels, prysm_amd/x/optym_plan.py restates them in
numpy.  PrysmLBFGSB (lbfgsb.py) runs its passes over the variables and its 2k x 2k algebra on csrc/lbfgsb.hip, its line search and breakpoint
sweep on the host (prysm_amd/x/lbfgsb_plan.py); it reads small records on the host every step and is not capturable.
"""
from .activation import Arctan, DiscreteEncoder, GumbelSoftmax, Sigmoid, Softmax, Softplus, Tanh  # noqa: F401
from .cost import bias_and_gain_invariant_error, mean_square_error, negative_loglikelihood  # noqa: F401
from .governors import (  # noqa: F401
    AllGovernor, AnyGovernor, ConstraintTolerance, FunctionTolerance, Governor, GovernorDecision, GradientTolerance, MaxEvaluations,
    MaxIterations, OptimizationResult, StepRecord, StepTolerance)
from .lbfgsb import PrysmLBFGSB  # noqa: F401
from .operators import SpatialGradient2D  # noqa: F401
from .optimizers import (  # noqa: F401
    AdaGrad, AdaMomentum, Adam, GradientDescent, RAdam, RMSProp, Yogi, as_problem, runN, run_until)
