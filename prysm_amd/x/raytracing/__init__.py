"""Sequential ray tracing on the device (the core of prysm/x/raytracing).

surfaces: Plane, Sphere, Conic, OffAxisConic, EvenAsphere, Surface and the circular and annular apertures.  spencer_and_murty:
raytrace on the kernel of csrc/raytrace.hip (one thread per ray, one launch per bundle), prepare / Prescription, the status helpers.
raygen: collimated fans and grids, finite fans.  analysis: spot_positions and transverse_ray_aberration.
prysm_amd/x/raytrace_plan.py packs the surface table and restates the kernel in numpy.

Not built: gratings and surface coatings, the polynomial, toroidal and biconic shapes, keep_intermediates and the differential and
adjoint traces, OpticalSystem, LensData, launch and aiming, the paraxial and first-order tools, the rest of analysis, Zemax and
Code V input, a materials catalogue.
"""
from . import analysis, raygen, spencer_and_murty, surfaces  # noqa: F401
from .analysis import spot_positions, transverse_ray_aberration  # noqa: F401
from .raygen import (  # noqa: F401
    concat_rayfans, generate_collimated_ray_fan, generate_collimated_rect_ray_grid, generate_finite_ray_fan, split_rayfans)
from .spencer_and_murty import (  # noqa: F401
    STATUS_CLIP, STATUS_MISS, STATUS_NEWTON, STATUS_OK, STATUS_TIR, Prescription, RayStatus, RayTraceResult, decode_status, prepare,
    raytrace, resolve_tol_sag, valid_mask)
from .surfaces import (  # noqa: F401
    STYPE_EVAL, STYPE_IMG, STYPE_OBJ, STYPE_REFLECT, STYPE_REFRACT, Conic, DepartureBand, EvenAsphere, OffAxisConic, Plane, Sphere, Surface,
    annular_aperture, circular_aperture)
