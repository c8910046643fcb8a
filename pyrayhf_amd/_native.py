"""ctypes binding of libprhf.so (C ABI: include/prhf.h).

The shared library is built in-tree by ``__graft_entry__.build()`` /
``make -C pyrayhf_amd/csrc`` and is the only compute path: if it is missing, or no GPU is
visible, the operator raises - there is no CPU fallback in this package.
"""

from __future__ import annotations

import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PRHF_LIB") or os.path.join(_HERE, "libprhf.so")   # PRHF_LIB: A/B builds

OK, EINVAL, ENEGDEN, EPEAK0, EHIP, ENOMEM = 0, -1, -2, -3, -4, -5
MODE_O, MODE_X = 0, 1
FLAG_DEVICE_PTRS, FLAG_ASYNC, FLAG_GRID_STABLE, FLAG_SHARED_FIELD = 0x1, 0x2, 0x4, 0x8
MATH_FAITHFUL, MATH_FAST, MATH_AUTO = 0, 1, 2
ABI_VERSION = 4

c_double_p = ctypes.POINTER(ctypes.c_double)


class Segment(ctypes.Structure):
    """``prhf_segment`` of include/prhf.h."""
    _fields_ = [("prof_begin", ctypes.c_int64), ("prof_end", ctypes.c_int64),
                ("mode", ctypes.c_int32), ("n_points", ctypes.c_int32),
                ("mult_offset", ctypes.c_int64), ("out_offset", ctypes.c_int64)]


class LmOptions(ctypes.Structure):
    """``prhf_lm_options`` of include/prhf.h."""
    _fields_ = [("max_iter", ctypes.c_int32), ("reserved", ctypes.c_int32), ("lambda0", ctypes.c_double),
                ("lambda_up", ctypes.c_double), ("lambda_down", ctypes.c_double), ("step_max", ctypes.c_double),
                ("ftol", ctypes.c_double), ("xtol", ctypes.c_double)]


# statuses of prhf_vfo_lm_fit_f64 (PRHF_LM_* of include/prhf.h)
LM_RUNNING, LM_CONVERGED_F, LM_CONVERGED_X, LM_SINGULAR, LM_NO_DATA, LM_NO_COST = range(6)
LM_MAX_TANGENTS = 8
LM_FIT_COUNTERS = 3


class NativeLibraryError(RuntimeError):
    """libprhf.so is missing, stale, or the HIP runtime failed."""


# every symbol include/prhf.h declares: name -> (restype, argtypes)
_PROTOTYPES = {
    "prhf_abi_version": (ctypes.c_int, []),
    "prhf_last_error": (ctypes.c_char_p, []),
    "prhf_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "prhf_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]),
    "prhf_ctx_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "prhf_ctx_set_stream": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]),
    "prhf_ctx_set_math": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "prhf_ctx_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_double]),
    "prhf_vfo_batch_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_vfo_jacobian_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_vfo_vjp_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_vfo_jvp_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_uint32]),
    "prhf_vfo_lm_fit_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_void_p] * 10 + [ctypes.c_uint32]),
    "prhf_lm_fit_counters": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "prhf_vfo_worklist_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_int64, ctypes.POINTER(Segment), ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_mu_mup_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_uint32]),
    "prhf_find_vh_f64": (ctypes.c_int, [ctypes.c_void_p] + [ctypes.c_void_p] * 4 +
                         [ctypes.c_int64, ctypes.c_int64, ctypes.c_double, ctypes.c_int32, ctypes.c_void_p,
                          ctypes.c_uint32]),
    "prhf_regrid_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4 +
                        [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + [ctypes.c_void_p] * 8 +
                        [ctypes.c_uint32]),
    "prhf_residual_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                         ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_vfo_residual_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_uint32]),
    "prhf_residual_many_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                              ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_uint32]),
    "prhf_vfo_residual_many_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 6 + [ctypes.c_uint32]),
    "prhf_snell_cartesian_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
        ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32]),
    "prhf_snell_spherical_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
        ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32]),
    "prhf_snell_fan_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, ctypes.c_double,
        ctypes.c_double, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
        ctypes.c_uint32]),
    "prhf_snell_home_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
        ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_double, ctypes.c_int32,
        ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_snell_skip_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
        ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
        ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.c_double,
        ctypes.c_int32, ctypes.c_double, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_snell_muf_f64": (ctypes.c_int, [
        ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_double,
        ctypes.c_double, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
        ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_double, ctypes.c_int32,
        ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_field_pack_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                           ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_field_sample_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_int64] +
                              [ctypes.c_double] * 3 + [ctypes.c_void_p] * 4 + [ctypes.c_uint32]),
    "prhf_trace_gradient_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                               ctypes.c_int64] + [ctypes.c_void_p] * 6 + [ctypes.c_int64] +
                                [ctypes.c_double] * 8 + [ctypes.c_int32] + [ctypes.c_double] * 3 +
                                [ctypes.c_void_p] * 6 + [ctypes.c_int64, ctypes.c_uint32]),
    "prhf_trace_gradient_spherical_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                                         ctypes.c_int64] + [ctypes.c_void_p] * 6 + [ctypes.c_int64] +
                                          [ctypes.c_double] * 9 + [ctypes.c_int32] + [ctypes.c_double] * 3 +
                                          [ctypes.c_void_p] * 6 + [ctypes.c_int64, ctypes.c_uint32]),
    "prhf_gradient_home_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_int64] +
                               [ctypes.c_void_p] * 2 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64] +
                               [ctypes.c_double] * 9 + [ctypes.c_int32] + [ctypes.c_double] * 4 +
                               [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_gradient_home_counters": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "prhf_trace_gradient_hops_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                                    ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 6 +
                                     [ctypes.c_int64] + [ctypes.c_double] * 9 + [ctypes.c_int32] + [ctypes.c_double] * 3 +
                                     [ctypes.c_int32] + [ctypes.c_void_p] * 6 + [ctypes.c_int64, ctypes.c_uint32]),
    "prhf_gradient_hop_home_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                                  ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 5 +
                                   [ctypes.c_int64] + [ctypes.c_void_p] * 2 +
                                   [ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_double] * 9 +
                                   [ctypes.c_int32] + [ctypes.c_double] * 4 +
                                   [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_uint32]),
    "prhf_field_build_f64": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int64, ctypes.c_int64] +
                             [ctypes.c_void_p] * 3 + [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32] +
                             [ctypes.c_void_p] * 3 + [ctypes.c_uint32]),
    "prhf_gradient_skip_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                              ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 5 + [ctypes.c_int64] +
                               [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_double] * 9 + [ctypes.c_int32] +
                               [ctypes.c_double] * 4 + [ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_gradient_muf_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 3 +
                              [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                               ctypes.c_int32] + [ctypes.c_void_p] * 3 +
                              [ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_void_p,
                               ctypes.c_int64] + [ctypes.c_double] * 9 + [ctypes.c_int32] + [ctypes.c_double] * 4 +
                              [ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_gradient_hop_skip_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64,
                                                  ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 5 +
                                   [ctypes.c_int64] + [ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_double] * 9 +
                                   [ctypes.c_int32] + [ctypes.c_double] * 4 +
                                   [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_gradient_hop_muf_f64": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_void_p] * 3 +
                                  [ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                   ctypes.c_int32] + [ctypes.c_void_p] * 3 +
                                  [ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_int32, ctypes.c_void_p,
                                   ctypes.c_int64] + [ctypes.c_double] * 9 + [ctypes.c_int32] + [ctypes.c_double] * 4 +
                                  [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_uint32]),
    "prhf_gradient_skip_counters": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "prhf_gradient_hop_skip_counters": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "prhf_pair_plan_counters": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "prhf_panel_counters": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "prhf_panel_upper_counters": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "prhf_panel_plan_counters": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "prhf_panel_quick_counters": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "prhf_stream_launches": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]),
    "prhf_occupancy": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                      ctypes.POINTER(ctypes.c_int32)]),
    "prhf_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "prhf_last_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]),
    "prhf_recent_kernel_ms": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int32,
                                             ctypes.POINTER(ctypes.c_int32)]),
}

_lib = None
_lib_lock = threading.Lock()


def load():
    """Load libprhf.so once and attach prototypes; raise NativeLibraryError if unusable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C pyrayhf_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
        # PyTorch-ROCm bundles its own HIP runtime.  If libprhf.so pulled in the system runtime first, a
        # later `import torch` would bring a second runtime into the process and that one finds no GPU
        # ("No HIP GPUs are available").  Loading torch first makes both share torch's runtime.
        if os.environ.get("PRHF_NO_TORCH_PRELOAD", "") == "":
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as exc:
            raise NativeLibraryError(f"cannot load {LIB_PATH}: {exc}") from exc
        for name, (res, args) in _PROTOTYPES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as exc:
                raise NativeLibraryError(f"{LIB_PATH} does not export {name}; rebuild it") from exc
            fn.restype = res
            fn.argtypes = args
        if lib.prhf_abi_version() != ABI_VERSION:
            raise NativeLibraryError(f"ABI version {lib.prhf_abi_version()} != {ABI_VERSION}; rebuild libprhf.so")
        _lib = lib
        return _lib


def exported_symbols():
    return sorted(_PROTOTYPES)


def last_error():
    msg = load().prhf_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def error_for(code, msg):
    """The exception the reference raises for the condition a PRHF_E* code stands for (``msg``: prhf_last_error of
    the thread that made the call)."""
    if code == ENEGDEN:
        return ValueError("Density must be non-negative")          # reference library.py:93-94
    if code == EPEAK0:
        return IndexError(msg or "density peak at index 0")         # the reference fails with IndexError too
    if code == EINVAL:
        return ValueError(msg or "invalid argument")
    if code == ENOMEM:
        return MemoryError(msg)
    return NativeLibraryError(msg or f"libprhf error {code}")


def raise_for(code):
    """Map a PRHF_E* code to the exception the reference raises for the same condition."""
    if code == OK:
        return
    raise error_for(code, last_error())


def device_count():
    n = ctypes.c_int(0)
    raise_for(load().prhf_device_count(ctypes.byref(n)))
    return n.value


class Context:
    """Owns one ``prhf_ctx`` (one device, one stream, scratch buffers)."""

    def __init__(self, device=0):
        self._lib = load()
        self._h = ctypes.c_void_p()
        raise_for(self._lib.prhf_ctx_create(int(device), ctypes.byref(self._h)))
        self.device = int(device)
        # what the library was last told, so that the per-call setters cost a comparison, not a foreign call
        self._math = None
        self._stream = (0, False)          # (handle, borrowed): the context starts on its own stream

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.prhf_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001 - interpreter shutdown
            pass

    def set_stream(self, stream_ptr, borrow=True):
        """Launch on the caller's stream (``stream_ptr`` 0 = the legacy default stream) or, with
        ``borrow=False``, on the context's own stream."""
        want = (int(stream_ptr or 0), bool(borrow)) if borrow else (0, False)
        if want == self._stream:
            return
        raise_for(self._lib.prhf_ctx_set_stream(self._h, ctypes.c_void_p(stream_ptr or None), 1 if borrow else 0))
        self._stream = want

    def set_math(self, level):
        level = int(level)
        if level == self._math:
            return
        raise_for(self._lib.prhf_ctx_set_math(self._h, level))
        self._math = level

    def set_option(self, name, value):
        """A launch-shaping or arithmetic setting of this context (include/prhf.h, prhf_ctx_set_option)."""
        raise_for(self._lib.prhf_ctx_set_option(self._h, str(name).encode(), float(value)))

    def vfo_batch(self, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride, alt_stride,
                  mult, n_points, mode, out, flags):
        """All array arguments are raw addresses (ints)."""
        return self._lib.prhf_vfo_batch_f64(self._h, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt,
                                            prof_stride, alt_stride, mult, n_points, mode, out, flags)

    def vfo_jacobian(self, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride, alt_stride,
                     mult, n_points, mode, vh_out, jac_out, flags):
        """d vh / d den, dense; ``vh_out`` may be None.  All array arguments are raw addresses (ints)."""
        return self._lib.prhf_vfo_jacobian_f64(self._h, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt,
                                               prof_stride, alt_stride, mult, n_points, mode, vh_out, jac_out, flags)

    def vfo_vjp(self, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride, alt_stride,
                mult, n_points, mode, grad_vh, vh_out, grad_den_out, flags):
        """sum_f grad_vh * d vh / d den; ``vh_out`` may be None."""
        return self._lib.prhf_vfo_vjp_f64(self._h, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride,
                                          alt_stride, mult, n_points, mode, grad_vh, vh_out, grad_den_out, flags)

    def vfo_jvp(self, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride, alt_stride,
                mult, n_points, mode, tangents, n_tan, tan_prof_stride, vh_out, dvh_out, flags):
        """sum_k d vh / d den_k * tangent_k for ``n_tan`` tangents; ``vh_out`` may be None."""
        return self._lib.prhf_vfo_jvp_f64(self._h, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride,
                                          alt_stride, mult, n_points, mode, tangents, n_tan, tan_prof_stride, vh_out,
                                          dvh_out, flags)

    def vfo_worklist(self, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride, alt_stride,
                     mult, mult_len, segments, out, flags):
        arr = (Segment * len(segments))(*segments)
        return self._lib.prhf_vfo_worklist_f64(self._h, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt,
                                               prof_stride, alt_stride, mult, mult_len, arr, len(segments),
                                               out, flags)

    def mu_mup(self, X, Y, psi, n, mode, mu, mup, flags):
        return self._lib.prhf_mu_mup_f64(self._h, X, Y, psi, n, mode, mu, mup, flags)

    def find_vh(self, X, Y, psi, dh, n_rows, n_cols, alt_min, mode, vh, flags):
        return self._lib.prhf_find_vh_f64(self._h, X, Y, psi, dh, n_rows, n_cols, float(alt_min), mode, vh, flags)

    def regrid(self, freq_hz, n_freq, den, bmag, bpsi, alt, n_alt, mult, n_points, mode, outs, flags):
        """outs: eight raw addresses in the order freq, den, bmag, bpsi, dist, alt, crit_height, ind."""
        return self._lib.prhf_regrid_f64(self._h, freq_hz, n_freq, den, bmag, bpsi, alt, n_alt, mult, n_points,
                                         mode, *outs, flags)

    def residual(self, vh_model, vh_obs, n_prof, n_freq, residual, cost, flags):
        return self._lib.prhf_residual_f64(self._h, vh_model, vh_obs, n_prof, n_freq, residual or None,
                                           cost or None, flags)

    def vfo_residual(self, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride, alt_stride, mult,
                     n_points, mode, vh_obs, vh, residual, cost, flags):
        return self._lib.prhf_vfo_residual_f64(self._h, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt,
                                               prof_stride, alt_stride, mult, n_points, mode, vh_obs,
                                               vh or None, residual or None, cost or None, flags)

    def residual_many(self, vh_model, n_rows, vh_obs, n_iono, n_freq, ionogram_of_row, residual, cost, best, best_cost,
                      flags):
        """``ionogram_of_row``: (n_rows) int32, or None for shared candidates (``cost`` is then (n_iono, n_rows))."""
        return self._lib.prhf_residual_many_f64(self._h, vh_model, n_rows, vh_obs, n_iono, n_freq,
                                                ionogram_of_row or None, residual or None, cost, best, best_cost, flags)

    def vfo_residual_many(self, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt, prof_stride, alt_stride, mult,
                          n_points, mode, vh_obs, n_iono, ionogram_of_row, vh, residual, cost, best, best_cost, flags):
        return self._lib.prhf_vfo_residual_many_f64(self._h, freq, n_freq, den, bmag, bpsi, alt, n_prof, n_alt,
                                                    prof_stride, alt_stride, mult, n_points, mode, vh_obs, n_iono,
                                                    ionogram_of_row or None, vh or None, residual or None, cost, best,
                                                    best_cost, flags)

    def snell_cartesian(self, freq_hz, elev, prof_idx, n_rays, den, bmag, bpsi, alt, n_prof, n_alt, alt_stride,
                        mode, out, path_x, path_z, path_stride, flags):
        return self._lib.prhf_snell_cartesian_f64(self._h, freq_hz, elev, prof_idx or None, n_rays, den, bmag, bpsi,
                                                  alt, n_prof, n_alt, alt_stride, mode, out, path_x or None,
                                                  path_z or None, path_stride, flags)

    def snell_spherical(self, freq_hz, elev, prof_idx, n_rays, den, bmag, bpsi, alt, n_prof, n_alt, alt_stride,
                        mode, r_e, dz_target, apex_boost, max_substeps, out, path_x, path_z, path_stride, flags):
        return self._lib.prhf_snell_spherical_f64(self._h, freq_hz, elev, prof_idx or None, n_rays, den, bmag, bpsi,
                                                  alt, n_prof, n_alt, alt_stride, mode, float(r_e), float(dz_target),
                                                  float(apex_boost), int(max_substeps), out, path_x or None,
                                                  path_z or None, path_stride, flags)

    def snell_fan(self, geometry, group_freq, group_prof, n_groups, ray_group, elev, n_rays, den, bmag, bpsi, alt, n_prof,
                  n_alt, alt_stride, mode, r_e, dz_target, apex_boost, max_substeps, out, path_x, path_z, path_stride,
                  flags):
        return self._lib.prhf_snell_fan_f64(self._h, int(geometry), group_freq, group_prof or None, n_groups, ray_group,
                                            elev, n_rays, den, bmag, bpsi, alt, n_prof, n_alt, alt_stride, mode,
                                            float(r_e), float(dz_target), float(apex_boost), int(max_substeps), out,
                                            path_x or None, path_z or None, path_stride, flags)

    def snell_home(self, geometry, group_freq, group_prof, n_groups, link_group, link_range, n_links, scan_elev, n_scan,
                   den, bmag, bpsi, alt, n_prof, n_alt, alt_stride, mode, r_e, dz_target, apex_boost, max_substeps,
                   range_tol, max_iter, max_roots, out, n_brackets, flags):
        """``out``: (n_links, max_roots, 11) doubles, ``n_brackets``: (n_links) int64 (include/prhf.h)."""
        return self._lib.prhf_snell_home_f64(self._h, int(geometry), group_freq, group_prof or None, n_groups, link_group,
                                             link_range, n_links, scan_elev, n_scan, den, bmag, bpsi, alt, n_prof, n_alt,
                                             alt_stride, mode, float(r_e), float(dz_target), float(apex_boost),
                                             int(max_substeps), float(range_tol), int(max_iter), int(max_roots), out,
                                             n_brackets, flags)

    def snell_skip(self, geometry, group_freq, group_prof, n_groups, scan_elev, n_scan, den, bmag, bpsi, alt, n_prof,
                   n_alt, alt_stride, mode, r_e, dz_target, apex_boost, max_substeps, elev_tol, max_iter, out, flags):
        """``out``: (n_groups, 13) doubles (include/prhf.h)."""
        return self._lib.prhf_snell_skip_f64(self._h, int(geometry), group_freq, group_prof or None, n_groups, scan_elev,
                                             n_scan, den, bmag, bpsi, alt, n_prof, n_alt, alt_stride, mode, float(r_e),
                                             float(dz_target), float(apex_boost), int(max_substeps), float(elev_tol),
                                             int(max_iter), out, flags)

    def snell_muf(self, geometry, link_prof, link_range, n_links, f_lo, f_hi, n_bisect, scan_elev, n_scan, den, bmag,
                  bpsi, alt, n_prof, n_alt, alt_stride, mode, r_e, dz_target, apex_boost, max_substeps, elev_tol, max_iter,
                  out, flags):
        """``out``: (n_links, 16) doubles (include/prhf.h)."""
        return self._lib.prhf_snell_muf_f64(self._h, int(geometry), link_prof or None, link_range, n_links, float(f_lo),
                                            float(f_hi), int(n_bisect), scan_elev, n_scan, den, bmag, bpsi, alt, n_prof,
                                            n_alt, alt_stride, mode, float(r_e), float(dz_target), float(apex_boost),
                                            int(max_substeps), float(elev_tol), int(max_iter), out, flags)

    def field_pack(self, mu, mup, n_fields, n0, n1, axis0, axis1, edge_order, records, flags):
        """``records``: a device address in every flag combination; the axes: host addresses."""
        return self._lib.prhf_field_pack_f64(self._h, mu, mup, n_fields, n0, n1, axis0, axis1, int(edge_order),
                                             records, flags)

    def field_sample(self, records, n_fields, n0, n1, axis0, axis1, p0, p1, field_index, n, fills, outs, flags):
        """fills: (fill_n, fill_grad, fill_mup); outs: four raw addresses (mu, d/da1, d/da0, mu'), None to skip."""
        return self._lib.prhf_field_sample_f64(self._h, records, n_fields, n0, n1, axis0, axis1, p0, p1,
                                               field_index or None, n, *(float(v) for v in fills),
                                               *(o or None for o in outs), flags)

    def trace_gradient(self, records, n_fields, nz, nx, z_axis, x_axis, x0, z0, elev, ray_field, n_rays, controls, fills,
                       out, paths, path_stride, flags):
        """controls: (s_max_km, rtol, atol, max_step_km, z_ground_km, z_max_km, x_min_km, x_max_km, renormalize_every);
        paths: five raw addresses (t, x, z, vx, vz) or None."""
        paths = paths or (None,) * 5
        return self._lib.prhf_trace_gradient_f64(self._h, records, n_fields, nz, nx, z_axis, x_axis, x0, z0, elev,
                                                 ray_field or None, n_rays, *(float(v) for v in controls[:8]),
                                                 int(controls[8]), *(float(v) for v in fills), out, *paths,
                                                 int(path_stride), flags)

    def trace_gradient_spherical(self, records, n_fields, nr, nphi, r_axis, phi_axis, x0, z0, elev, ray_field, n_rays,
                                 earth_radius, controls, fills, out, paths, path_stride, flags):
        """controls: (s_max_km, rtol, atol, max_step_km, z_ground_km, r_max_km, phi_min, phi_max, renormalize_every);
        paths: five raw addresses (t, r, phi, v_r, v_phi) or None."""
        paths = paths or (None,) * 5
        return self._lib.prhf_trace_gradient_spherical_f64(self._h, records, n_fields, nr, nphi, r_axis, phi_axis, x0, z0,
                                                           elev, ray_field or None, n_rays, float(earth_radius),
                                                           *(float(v) for v in controls[:8]), int(controls[8]),
                                                           *(float(v) for v in fills), out, *paths, int(path_stride),
                                                           flags)

    def gradient_home(self, geometry, records, n_fields, n0, n1, axis0, axis1, group_field, group_x0, group_z0, n_groups,
                      link_group, link_target, n_links, scan_elev, n_scan, earth_radius, controls, fills, range_tol,
                      max_iter, max_roots, out, n_brackets, flags):
        """controls: (s_max_km, rtol, atol, max_step_km, z_ground_km, top, left, right, renormalize_every) - the tracer's;
        ``out``: (n_links, max_roots, 15) doubles, ``n_brackets``: (n_links) int64 (include/prhf.h)."""
        return self._lib.prhf_gradient_home_f64(self._h, int(geometry), records, n_fields, n0, n1, axis0, axis1,
                                                group_field, group_x0, group_z0, n_groups, link_group, link_target,
                                                n_links, scan_elev, n_scan, float(earth_radius),
                                                *(float(v) for v in controls[:8]), int(controls[8]),
                                                *(float(v) for v in fills), float(range_tol), int(max_iter),
                                                int(max_roots), out, n_brackets, flags)

    def trace_gradient_hops(self, geometry, records, n_fields, n0, n1, axis0, axis1, x0, z0, elev, ray_field, n_rays,
                            earth_radius, controls, fills, n_hops, out, paths, path_stride, flags):
        """controls: gradient_home's; ``out``: (n_rays, n_hops, 15) doubles; paths: five raw addresses of
        (n_rays n_hops, path_stride) doubles each, or None (include/prhf.h)."""
        paths = paths or (None,) * 5
        return self._lib.prhf_trace_gradient_hops_f64(self._h, int(geometry), records, n_fields, n0, n1, axis0, axis1, x0, z0,
                                                      elev, ray_field or None, n_rays, float(earth_radius),
                                                      *(float(v) for v in controls[:8]), int(controls[8]),
                                                      *(float(v) for v in fills), int(n_hops), out, *paths,
                                                      int(path_stride), flags)

    def gradient_hop_home(self, geometry, records, n_fields, n0, n1, axis0, axis1, group_field, group_x0, group_z0, n_groups,
                          link_group, link_target, n_links, scan_elev, n_scan, earth_radius, controls, fills, range_tol,
                          max_iter, max_roots, n_hops, out, n_brackets, flags):
        """gradient_home on the landing of hop ``n_hops`` - 1; ``out``: (n_links, max_roots, 3 + 15 n_hops) doubles."""
        return self._lib.prhf_gradient_hop_home_f64(self._h, int(geometry), records, n_fields, n0, n1, axis0, axis1,
                                                    group_field, group_x0, group_z0, n_groups, link_group, link_target,
                                                    n_links, scan_elev, n_scan, float(earth_radius),
                                                    *(float(v) for v in controls[:8]), int(controls[8]),
                                                    *(float(v) for v in fills), float(range_tol), int(max_iter),
                                                    int(max_roots), int(n_hops), out, n_brackets, flags)

    def gradient_home_counters(self):
        """(brackets refined, rays traced by the refine lanes, ray slots, refine wavefronts) of the last gradient_home."""
        buf = (ctypes.c_uint64 * 4)()
        raise_for(self._lib.prhf_gradient_home_counters(self._h, buf))
        return tuple(int(v) for v in buf)

    def field_build(self, den, bmag, bpsi, n0, n1, axis0, axis1, freq_hz, n_freq, mode, edge_order, records, mu, mup,
                    flags):
        """``records``: a device address in every flag combination; the axes: host addresses; ``mu``, ``mup``: both or
        neither (include/prhf.h)."""
        return self._lib.prhf_field_build_f64(self._h, den, bmag, bpsi, n0, n1, axis0, axis1, freq_hz, n_freq, int(mode),
                                              int(edge_order), records, mu or None, mup or None, flags)

    def gradient_skip(self, geometry, records, n_fields, n0, n1, axis0, axis1, group_field, group_x0, group_z0, n_groups,
                      scan_elev, n_scan, earth_radius, controls, fills, elev_tol, max_iter, out, flags):
        """controls: gradient_home's; ``out``: (n_groups, 18) doubles (include/prhf.h)."""
        return self._lib.prhf_gradient_skip_f64(self._h, int(geometry), records, n_fields, n0, n1, axis0, axis1,
                                                group_field, group_x0, group_z0, n_groups, scan_elev, n_scan,
                                                float(earth_radius), *(float(v) for v in controls[:8]), int(controls[8]),
                                                *(float(v) for v in fills), float(elev_tol), int(max_iter), out, flags)

    def gradient_muf(self, geometry, den, bmag, bpsi, n0, n1, axis0, axis1, mode, edge_order, link_x0, link_z0, link_target,
                     n_links, f_lo, f_hi, n_bisect, scan_elev, n_scan, earth_radius, controls, fills, elev_tol, max_iter,
                     out, flags):
        """controls: gradient_home's; ``out``: (n_links, 21) doubles (include/prhf.h)."""
        return self._lib.prhf_gradient_muf_f64(self._h, int(geometry), den, bmag, bpsi, n0, n1, axis0, axis1, int(mode),
                                               int(edge_order), link_x0, link_z0, link_target, n_links, float(f_lo),
                                               float(f_hi), int(n_bisect), scan_elev, n_scan, float(earth_radius),
                                               *(float(v) for v in controls[:8]), int(controls[8]),
                                               *(float(v) for v in fills), float(elev_tol), int(max_iter), out, flags)

    def gradient_hop_skip(self, geometry, records, n_fields, n0, n1, axis0, axis1, group_field, group_x0, group_z0, n_groups,
                          scan_elev, n_scan, earth_radius, controls, fills, elev_tol, max_iter, n_hops, out, flags):
        """gradient_skip on the landing of hop ``n_hops`` - 1; ``out``: (n_groups, 6 + 15 n_hops) doubles."""
        return self._lib.prhf_gradient_hop_skip_f64(self._h, int(geometry), records, n_fields, n0, n1, axis0, axis1,
                                                    group_field, group_x0, group_z0, n_groups, scan_elev, n_scan,
                                                    float(earth_radius), *(float(v) for v in controls[:8]),
                                                    int(controls[8]), *(float(v) for v in fills), float(elev_tol),
                                                    int(max_iter), int(n_hops), out, flags)

    def gradient_hop_muf(self, geometry, den, bmag, bpsi, n0, n1, axis0, axis1, mode, edge_order, link_x0, link_z0,
                         link_target, n_links, f_lo, f_hi, n_bisect, scan_elev, n_scan, earth_radius, controls, fills,
                         elev_tol, max_iter, n_hops, out, flags):
        """gradient_muf of the ``n_hops``-hop mode; ``out``: (n_links, 3 + 6 + 15 n_hops) doubles."""
        return self._lib.prhf_gradient_hop_muf_f64(self._h, int(geometry), den, bmag, bpsi, n0, n1, axis0, axis1, int(mode),
                                                   int(edge_order), link_x0, link_z0, link_target, n_links, float(f_lo),
                                                   float(f_hi), int(n_bisect), scan_elev, n_scan, float(earth_radius),
                                                   *(float(v) for v in controls[:8]), int(controls[8]),
                                                   *(float(v) for v in fills), float(elev_tol), int(max_iter),
                                                   int(n_hops), out, flags)

    def gradient_hop_skip_counters(self):
        """``gradient_skip_counters`` and, fifth, the hop rays of the refine lanes' chains that landed (0 after a
        one-hop call), of the last skip or MUF call of the gradient tracers."""
        buf = (ctypes.c_uint64 * 5)()
        raise_for(self._lib.prhf_gradient_hop_skip_counters(self._h, buf))
        return tuple(int(v) for v in buf)

    def gradient_skip_counters(self):
        """(groups refined, rays traced by the refine lanes, ray slots, refine wavefronts) of the last gradient_skip or
        gradient_muf."""
        buf = (ctypes.c_uint64 * 4)()
        raise_for(self._lib.prhf_gradient_skip_counters(self._h, buf))
        return tuple(int(v) for v in buf)

    def pair_plan_counters(self):
        """(pairs whose sum ran from a plan, eligible pairs that planned themselves) since this context was made
        (option ``pair_plan``, include/prhf.h)."""
        buf = (ctypes.c_uint64 * 2)()
        raise_for(self._lib.prhf_pair_plan_counters(self._h, buf))
        return tuple(int(v) for v in buf)

    def panel_counters(self):
        """(pairs whose lower segments took the panel sum, eligible pairs that kept the sum of before) since this
        context was made (option ``panel_lower``, include/prhf.h)."""
        buf = (ctypes.c_uint64 * 2)()
        raise_for(self._lib.prhf_panel_counters(self._h, buf))
        return tuple(int(v) for v in buf)

    def panel_upper_counters(self):
        """(pairs whose panel region reached the top segment, pairs that kept the lower region only) since this
        context was made (option ``panel_upper``, include/prhf.h)."""
        buf = (ctypes.c_uint64 * 2)()
        raise_for(self._lib.prhf_panel_upper_counters(self._h, buf))
        return tuple(int(v) for v in buf)

    def panel_plan_counters(self):
        """(pairs whose plan carried the panel sum's region, so that their waves read it instead of computing it,)
        since this context was made (include/prhf.h)."""
        buf = (ctypes.c_uint64 * 1)()
        raise_for(self._lib.prhf_panel_plan_counters(self._h, buf))
        return tuple(int(v) for v in buf)

    def panel_quick_counters(self):
        """(list passes of the panel sum whose runs all passed the quick bound and skipped the exact tests, list passes
        that took the exact tests) since this context was made (option ``panel_quick``, include/prhf.h)."""
        buf = (ctypes.c_uint64 * 2)()
        raise_for(self._lib.prhf_panel_quick_counters(self._h, buf))
        return tuple(int(v) for v in buf)

    def stream_launches(self):
        """Operator launches of this context that took the streaming form of the persistent launch (option
        ``stream_blocks``, include/prhf.h) since it was made."""
        n = ctypes.c_uint64(0)
        raise_for(self._lib.prhf_stream_launches(self._h, ctypes.byref(n)))
        return int(n.value)

    def vfo_lm_fit(self, freq, n_freq, den0, bmag, bpsi, alt, n_iono, n_alt, den0_stride, alt_stride, mult, n_points, mode,
                   basis, n_tan, basis_stride, vh_obs, c0, prior_weight, options, c_out, cost_out, status_out, n_eval_out,
                   n_accept_out, lambda_out, den_out, vh_out, history_out, state_out, flags):
        """Levenberg-Marquardt fits of ``n_iono`` ionograms in a basis of ``n_tan`` log-density perturbations;
        ``options`` an ``LmOptions`` or None, ``c0``, ``prior_weight``, ``history_out``, ``state_out`` may be None."""
        return self._lib.prhf_vfo_lm_fit_f64(self._h, freq, n_freq, den0, bmag, bpsi, alt, n_iono, n_alt, den0_stride,
                                             alt_stride, mult, n_points, mode, basis, n_tan, basis_stride, vh_obs, c0,
                                             prior_weight, ctypes.addressof(options) if options is not None else None,
                                             c_out, cost_out, status_out, n_eval_out, n_accept_out, lambda_out, den_out,
                                             vh_out, history_out, state_out, flags)

    def lm_fit_counters(self):
        """(evaluations enqueued, timed launches enqueued, times the host waited for the stream) of this context's last
        ``vfo_lm_fit`` (include/prhf.h)."""
        buf = (ctypes.c_uint64 * LM_FIT_COUNTERS)()
        raise_for(self._lib.prhf_lm_fit_counters(self._h, buf))
        return tuple(int(v) for v in buf)

    def occupancy(self, n_alt, math):
        n = ctypes.c_int32(0)
        raise_for(self._lib.prhf_occupancy(self._h, int(n_alt), int(math), ctypes.byref(n)))
        return n.value

    def sync(self):
        return self._lib.prhf_sync(self._h)

    def last_kernel_ms(self):
        ms = ctypes.c_double(0.0)
        raise_for(self._lib.prhf_last_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def recent_kernel_ms(self, count=64):
        """Device times [ms] of the most recent launches (at most 64 are remembered), oldest first; one
        synchronisation on the newest."""
        buf = (ctypes.c_double * max(int(count), 1))()
        n = ctypes.c_int32(0)
        raise_for(self._lib.prhf_recent_kernel_ms(self._h, buf, int(count), ctypes.byref(n)))
        return [buf[i] for i in range(n.value)]


_tls = threading.local()


def default_device():
    for key in ("PRHF_DEVICE", "LOCAL_RANK"):
        if os.environ.get(key, "") != "":
            return int(os.environ[key])
    return 0


def host_context(device=None):
    """The cached context, launching on its OWN stream: what every host-buffer (NumPy) call uses.  A
    previous torch call on this thread may have left the context on torch's stream (borrowed); a host
    call must not keep running there - that stream may be the legacy blocking one, or already destroyed."""
    ctx = context(device)
    ctx.set_stream(0, borrow=False)
    return ctx


def context(device=None):
    """Per-thread, per-device cached context."""
    dev = default_device() if device is None else int(device)
    cache = getattr(_tls, "ctx", None)
    if cache is None:
        cache = _tls.ctx = {}
    ctx = cache.get(dev)
    if ctx is None:
        ctx = cache[dev] = Context(dev)
    return ctx
