"""MI355X-native vertical-ionogram forward operator (drop-in for PyRayHF's hot path).

``pyrayhf_amd.library.vertical_forward_operator`` keeps the signature of the reference's
``PyRayHF.library.vertical_forward_operator`` (reference ``PyRayHF/library.py:459-460``)
and runs on hand-written HIP kernels for gfx950 through a C-ABI shim (``include/prhf.h``).
"""

import logging

logger = logging.getLogger("pyrayhf_amd")

__version__ = "0.1.0"

from .gradient import (STATUS_NAMES, RefractiveField, build_mup_function,                       # noqa: E402
                       build_refractive_index_interpolator_cartesian,
                       build_refractive_index_interpolator_spherical, home_hops_cartesian_gradient,
                       home_hops_spherical_gradient, home_rays_cartesian_gradient,
                       home_rays_spherical_gradient, muf_cartesian_gradient, muf_spherical_gradient,
                       refractive_field, refractive_field_device, skip_distance_cartesian_gradient,
                       skip_distance_spherical_gradient, muf_hops_cartesian_gradient,
                       muf_hops_spherical_gradient, skip_distance_hops_cartesian_gradient,
                       skip_distance_hops_spherical_gradient,
                       trace_fan_cartesian_gradient, trace_fan_spherical_gradient,
                       trace_hop_fan_cartesian_gradient, trace_hop_fan_spherical_gradient,
                       trace_hops_cartesian_gradient, trace_hops_spherical_gradient,
                       trace_ray_cartesian_gradient, trace_ray_spherical_gradient,
                       trace_rays_cartesian_gradient, trace_rays_spherical_gradient)
from .tracers import (home_rays_cartesian_snells, home_rays_spherical_snells, muf_cartesian_snells,  # noqa: E402
                      muf_spherical_snells, skip_distance_cartesian_snells, skip_distance_spherical_snells)
from .fitting import (brute_force_fit_many, fit_profiles_lm, minimize_parameters_many,              # noqa: E402
                      residual_VH_many)

__all__ = ["logger", "__version__", "STATUS_NAMES", "RefractiveField", "build_mup_function",
           "build_refractive_index_interpolator_cartesian", "build_refractive_index_interpolator_spherical",
           "refractive_field", "trace_fan_cartesian_gradient", "trace_fan_spherical_gradient",
           "trace_ray_cartesian_gradient", "trace_ray_spherical_gradient", "trace_rays_cartesian_gradient",
           "trace_rays_spherical_gradient", "home_rays_cartesian_snells", "home_rays_spherical_snells",
           "home_rays_cartesian_gradient", "home_rays_spherical_gradient", "skip_distance_cartesian_snells",
           "skip_distance_spherical_snells", "muf_cartesian_snells", "muf_spherical_snells",
           "refractive_field_device", "skip_distance_cartesian_gradient", "skip_distance_spherical_gradient",
           "muf_cartesian_gradient", "muf_spherical_gradient", "trace_hops_cartesian_gradient",
           "trace_hops_spherical_gradient", "trace_hop_fan_cartesian_gradient", "trace_hop_fan_spherical_gradient",
           "home_hops_cartesian_gradient", "home_hops_spherical_gradient",
           "skip_distance_hops_cartesian_gradient", "skip_distance_hops_spherical_gradient",
           "muf_hops_cartesian_gradient", "muf_hops_spherical_gradient", "residual_VH_many", "brute_force_fit_many",
           "minimize_parameters_many", "fit_profiles_lm"]
