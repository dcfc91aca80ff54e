"""actinon_amd -- MI355X-native trace/radiance path of the Actinon ray tracer behind its scene_s render seam.

The product is two C libraries (actinon_amd/lib): libactinon_hip.so (HIP kernels + C ABI, include/actinon_hip.h)
and libactinon_host.so (plain-C scene assembly + render driver, include/acn_scene.h).  This package is ctypes
plumbing over them for tests and benchmarks; importing it fails if the libraries are not built."""
import os as _os
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # see actinon_hip.hip (concurrent lanes); no effect once HIP is initialised

from . import abi
from ._lib import AcnError, check, hip, host
from .scene import (Flat, Frame, Handle, KeptHandle, LensStats, Scene, Surface, cps_from_cl, detmath_eval, device_count, key_hist_edge, key_hist_threshold,
                    lcg00_jump, main_pass_positions, motion_from_scenes, run_script, set_host_cycles, v3)
from .motion import rigid_copy

__all__ = ["abi", "AcnError", "check", "hip", "host", "Flat", "Frame", "Handle", "KeptHandle", "LensStats", "Scene", "Surface", "cps_from_cl", "detmath_eval", "run_script",
           "device_count", "key_hist_edge", "key_hist_threshold", "lcg00_jump", "main_pass_positions", "motion_from_scenes", "rigid_copy", "set_host_cycles", "v3"]
