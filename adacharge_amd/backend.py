"""ctypes binding of the C ABI in include/acn_qp.h (libacn_qp_hip.so).

There is exactly one compute path: the HIP library.  If it is missing or no GPU
is visible, everything here raises -- there is no CPU fallback by design
(the CPU implementations under oracle/ are test infrastructure and are never
imported from this package).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .builder import CONE_SOC, ProblemBatch, SiteData

_LIB_NAME = "libacn_qp_hip.so"
_LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")

STATUS_UNSET = 0
STATUS_SOLVED = 1
STATUS_MAX_ITER = 2
STATUS_PRIMAL_INFEASIBLE = 3
STATUS_EMPTY_SET = 4
STATUS_SOLVED_INACCURATE = 5   # cp.OPTIMAL_INACCURATE: accepted by the reference (aco.py:319)
ACCEPTED_STATUSES = (STATUS_SOLVED, STATUS_SOLVED_INACCURATE)
STATUS_NAMES = {
    STATUS_UNSET: "unset",
    STATUS_SOLVED: "optimal",
    STATUS_MAX_ITER: "max_iter_reached",
    STATUS_PRIMAL_INFEASIBLE: "infeasible",
    STATUS_EMPTY_SET: "infeasible",
    STATUS_SOLVED_INACCURATE: "optimal_inaccurate",
}


class BackendUnavailable(RuntimeError):
    """The HIP library could not be loaded or no MI355X is visible."""


class _Site(C.Structure):
    _fields_ = [
        ("n_evse", C.c_int32),
        ("n_infra", C.c_int32),
        ("n_rows", C.c_int32),
        ("cone", C.c_int32),
        ("has_peak", C.c_int32),
        ("has_flat", C.c_int32),
        ("has_max", C.c_int32),
        ("G", C.c_void_p),
        ("limits", C.c_void_p),
    ]


class _Problems(C.Structure):
    _fields_ = [
        ("batch", C.c_int32),
        ("t_max", C.c_int32),
        ("k_sessions", C.c_int32),
        ("horizon", C.c_void_p),
        ("lb", C.c_void_p),
        ("ub", C.c_void_p),
        ("q", C.c_void_p),
        ("pdiag", C.c_void_p),
        ("s_off", C.c_void_p),
        ("s_len", C.c_void_p),
        ("s_cap", C.c_void_p),
        ("s_eq", C.c_void_p),
        ("peak", C.c_void_p),
        ("lf", C.c_void_p),
        ("dc", C.c_void_p),
        ("dfloor", C.c_void_p),
        ("warm_x", C.c_void_p),
        ("warm_y", C.c_void_p),
    ]


class _Table(C.Structure):
    """Mirror of ``acnqp_table`` (include/acn_qp.h)."""

    _fields_ = [(k, C.c_int32) for k in ("batch", "t_max", "k_sessions", "n_sessions", "n_horizons")] + [
        (k, C.c_void_p) for k in ("horizon", "q_index", "q_table", "pdiag", "s_eq", "peak", "lf", "dc", "dfloor", "sess_seg",
                                  "s_evse", "s_slot", "s_off", "s_len", "s_cap", "rate_seg", "min_rates", "max_rates")]


class _Results(C.Structure):
    _fields_ = [
        ("x", C.c_void_p),
        ("status", C.c_void_p),
        ("iters", C.c_void_p),
        ("pri_res", C.c_void_p),
        ("dua_res", C.c_void_p),
        ("obj", C.c_void_p),
        ("y", C.c_void_p),
        ("x_dev", C.c_void_p),
    ]


class _Duals(C.Structure):
    """Mirror of ``acnqp_duals`` (include/acn_qp.h)."""

    _fields_ = [("mu", C.c_void_p), ("z", C.c_void_p), ("res", C.c_void_p)]


class _PilotPlan(C.Structure):
    """Mirror of ``acnqp_pilot_plan`` (include/acn_qp.h)."""

    _fields_ = [(k, C.c_int32) for k in ("batch", "t_max", "n_evse", "n_infra", "n_levels", "n_sessions", "mode")] + [
        (k, C.c_void_p) for k in ("cre", "cim", "limits", "max_pilot", "levels", "sess_seg", "s_evse", "s_arrived", "s_cap")]


class _Pilots(C.Structure):
    """Mirror of ``acnqp_pilots`` (include/acn_qp.h)."""

    _fields_ = [("pilots", C.c_void_p), ("first", C.c_void_p), ("visits", C.c_void_p)]


PILOTS_CONTINUOUS, PILOTS_DISCRETE, PILOTS_REALLOCATE = 0, 1, 2


class _AdvancePlan(C.Structure):
    """Mirror of ``acnqp_advance_plan`` (include/acn_qp.h)."""

    _fields_ = [(k, C.c_int32) for k in ("n_evse", "n_rows", "n_horizons", "step", "peak_len", "n_arrivals", "n_rates")] + [
        ("done_tol", C.c_double), ("kw_per_amp", C.c_double), ("warm_arrival_gain", C.c_double)] + [
        (k, C.c_void_p) for k in ("q_table", "h_scal", "h_row", "peak_series", "a_seg", "a_evse", "a_slot", "a_len", "a_cap",
                                  "a_rate_seg", "a_min", "a_max")]


class ClockCost(C.Structure):
    """Mirror of ``acnqp_clock_cost`` (include/acn_qp.h): the clock cost of the advance's rule 6b."""

    _fields_ = [("n_evse", C.c_int32), ("series_len", C.c_int32), ("coef", C.c_double), ("weight", C.c_void_p), ("series", C.c_void_p)]


class _Next(C.Structure):
    """Mirror of ``acnqp_next`` (include/acn_qp.h)."""

    _fields_ = [(k, C.c_void_p) for k in ("horizon", "lb", "ub", "q", "pdiag", "s_off", "s_len", "s_cap", "peak", "lf", "dc",
                                          "dfloor", "warm_x", "warm_y")]


ADVANCE_REFUSED, ADVANCE_NO_ROW, ADVANCE_BAD_SLOT = 1, 2, 4


class _PreparePlan(C.Structure):
    """Mirror of ``acnqp_prepare_plan`` (include/acn_qp.h)."""

    _fields_ = [("n_evse", C.c_int32), ("n_infra", C.c_int32)] + [(k, C.c_void_p) for k in ("key", "cre", "cim", "limits", "min_pilot")]


class _PrepareView(C.Structure):
    """Mirror of ``acnqp_prepare_view`` (include/acn_qp.h)."""

    _fields_ = [("v_evse", C.c_void_p), ("v_arrived", C.c_void_p), ("v_cap", C.c_void_p)]


PREPARE_FUTURE = 1


class Options(C.Structure):
    """Mirror of ``acnqp_options``; construct with ``default_options()``."""

    _fields_ = [
        ("eps_abs", C.c_double),
        ("eps_rel", C.c_double),
        ("max_iter", C.c_int32),
        ("check_every", C.c_int32),
        ("adapt_every", C.c_int32),
        ("rho", C.c_double),
        ("sigma", C.c_double),
        ("alpha", C.c_double),
        ("adapt_tol", C.c_double),
        ("reg_rel", C.c_double),
        ("precision", C.c_int32),
        ("accel_mem", C.c_int32),
        ("stall_iters", C.c_int32),
        ("retry_passes", C.c_int32),
        ("retry_max_iter", C.c_int32),
        ("polish_iters", C.c_int32),
        ("retry_rho", C.c_double),
        ("inaccurate_floor", C.c_double),
        ("polish_stall", C.c_int32),
    ]


# every symbol include/acn_qp.h declares; tests check the library exports all of them
EXPORTED_SYMBOLS = (
    "acnqp_create",
    "acnqp_solve_batch",
    "acnqp_solve_batch_device",
    "acnqp_destroy",
    "acnqp_default_options",
    "acnqp_last_error",
    "acnqp_abi_version",
    "acnqp_last_kernel_ms",
    "acnqp_accel_columns",
    "acnqp_kernel_times",
    "acnqp_ordered_launch_count",
    "acnqp_polish_stats",
    "acnqp_solve_batches",
    "acnqp_solve_table",
    "acnqp_host_alloc",
    "acnqp_host_free",
    "acnqp_launch_count",
    "acnqp_route",
    "acnqp_duals_device",
    "acnqp_duals_host",
    "acnqp_pilots_device",
    "acnqp_pilots_host",
    "acnqp_advance_device",
    "acnqp_advance_host",
    "acnqp_advance_priced_device",
    "acnqp_advance_priced_host",
    "acnqp_prepare_device",
    "acnqp_prepare_host",
)

# kernel families of acnqp_route (ACNQP_ROUTE_* in include/acn_qp.h)
ROUTE_NAMES = {1: "wave1", 2: "wave2", 3: "wave3", 4: "wave4", 5: "wave5", 6: "tiled_ct1", 7: "tiled_ct2",
               8: "long_lds", 9: "long_ws", 10: "stream", 11: "general"}

_lib = None


def library_path() -> str:
    return os.environ.get("ACNQP_LIBRARY", os.path.join(_LIB_DIR, _LIB_NAME))


def load_library():
    """dlopen the HIP library (once) and set the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own HIP runtime; it must be the one already loaded when our
    # library resolves libamdhip64, or the process ends up with two runtimes and the
    # second sees no GPU.  torch is plumbing here (device memory, torch.distributed).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = library_path()
    if not os.path.exists(path):
        raise BackendUnavailable(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  adacharge_amd has no CPU fallback."
        )
    try:
        lib = C.CDLL(path)
    except OSError as exc:  # missing ROCm runtime etc.
        raise BackendUnavailable(f"cannot load {path}: {exc}") from exc
    lib.acnqp_create.argtypes = [C.POINTER(_Site), C.c_int32, C.POINTER(C.c_void_p)]
    lib.acnqp_create.restype = C.c_int
    lib.acnqp_solve_batch.argtypes = [C.c_void_p, C.POINTER(_Problems), C.POINTER(Options), C.POINTER(_Results)]
    lib.acnqp_solve_batch.restype = C.c_int
    lib.acnqp_solve_batch_device.argtypes = [
        C.c_void_p, C.POINTER(_Problems), C.POINTER(Options), C.POINTER(_Results), C.c_void_p,
    ]
    lib.acnqp_solve_batch_device.restype = C.c_int
    lib.acnqp_destroy.argtypes = [C.c_void_p]
    lib.acnqp_destroy.restype = None
    lib.acnqp_default_options.argtypes = [C.POINTER(Options)]
    lib.acnqp_default_options.restype = None
    lib.acnqp_last_error.argtypes = []
    lib.acnqp_last_error.restype = C.c_char_p
    lib.acnqp_abi_version.argtypes = []
    lib.acnqp_abi_version.restype = C.c_int32
    lib.acnqp_last_kernel_ms.argtypes = [C.c_void_p]
    lib.acnqp_last_kernel_ms.restype = C.c_float
    lib.acnqp_accel_columns.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.acnqp_accel_columns.restype = C.c_int32
    lib.acnqp_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32]
    lib.acnqp_kernel_times.restype = C.c_int32
    lib.acnqp_solve_batches.argtypes = [C.c_void_p, C.c_int32, C.POINTER(_Problems), C.POINTER(Options), C.POINTER(_Results)]
    lib.acnqp_solve_batches.restype = C.c_int
    lib.acnqp_solve_table.argtypes = [C.c_void_p, C.POINTER(_Table), C.POINTER(Options), C.POINTER(_Results)]
    lib.acnqp_solve_table.restype = C.c_int
    lib.acnqp_host_alloc.argtypes = [C.c_size_t]
    lib.acnqp_host_alloc.restype = C.c_void_p
    lib.acnqp_host_free.argtypes = [C.c_void_p]
    lib.acnqp_host_free.restype = None
    lib.acnqp_launch_count.argtypes = [C.c_void_p]
    lib.acnqp_launch_count.restype = C.c_int64
    lib.acnqp_ordered_launch_count.argtypes = [C.c_void_p]
    lib.acnqp_ordered_launch_count.restype = C.c_int64
    lib.acnqp_polish_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int32]
    lib.acnqp_polish_stats.restype = C.c_int
    lib.acnqp_route.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    lib.acnqp_route.restype = C.c_int32
    lib.acnqp_duals_device.argtypes = [C.c_void_p, C.POINTER(_Problems), C.POINTER(Options), C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(_Duals), C.c_void_p]
    lib.acnqp_duals_device.restype = C.c_int
    lib.acnqp_duals_host.argtypes = [C.c_void_p, C.POINTER(_Problems), C.POINTER(Options), C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.POINTER(_Duals)]
    lib.acnqp_duals_host.restype = C.c_int
    lib.acnqp_pilots_device.argtypes = [C.c_void_p, C.POINTER(_PilotPlan), C.c_void_p, C.POINTER(_Pilots), C.c_void_p]
    lib.acnqp_pilots_device.restype = C.c_int
    lib.acnqp_pilots_host.argtypes = [C.c_void_p, C.POINTER(_PilotPlan), C.c_void_p, C.POINTER(_Pilots)]
    lib.acnqp_pilots_host.restype = C.c_int
    lib.acnqp_advance_device.argtypes = [C.c_void_p, C.POINTER(_Problems), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(_AdvancePlan), C.POINTER(_Next), C.c_void_p, C.c_void_p]
    lib.acnqp_advance_device.restype = C.c_int
    lib.acnqp_advance_host.argtypes = [C.c_void_p, C.POINTER(_Problems), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.POINTER(_AdvancePlan), C.POINTER(_Next), C.c_void_p]
    lib.acnqp_advance_host.restype = C.c_int
    lib.acnqp_advance_priced_device.argtypes = [C.c_void_p, C.POINTER(_Problems), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(_AdvancePlan), C.POINTER(ClockCost), C.POINTER(_Next), C.c_void_p, C.c_void_p]
    lib.acnqp_advance_priced_device.restype = C.c_int
    lib.acnqp_advance_priced_host.argtypes = [C.c_void_p, C.POINTER(_Problems), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(_AdvancePlan), C.POINTER(ClockCost), C.POINTER(_Next), C.c_void_p]
    lib.acnqp_advance_priced_host.restype = C.c_int
    lib.acnqp_prepare_device.argtypes = [C.c_void_p, C.POINTER(_Problems), C.POINTER(_PreparePlan), C.c_void_p, C.c_void_p,
                                         C.POINTER(_PrepareView), C.c_void_p, C.c_void_p]
    lib.acnqp_prepare_device.restype = C.c_int
    lib.acnqp_prepare_host.argtypes = [C.c_void_p, C.POINTER(_Problems), C.POINTER(_PreparePlan), C.c_void_p, C.c_void_p,
                                       C.POINTER(_PrepareView), C.c_void_p]
    lib.acnqp_prepare_host.restype = C.c_int
    _lib = lib
    return lib


def default_options(**overrides) -> Options:
    o = Options()
    load_library().acnqp_default_options(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown solver option {k!r}")
        setattr(o, k, v)
    return o


def _check(rc: int, what: str):
    if rc != 0:
        msg = load_library().acnqp_last_error().decode()
        if rc == -3:
            raise BackendUnavailable(f"{what}: {msg}")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed (rc={rc}): {msg}")


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dptr(t):
    """the device address of a torch tensor (None stays None)"""
    return None if t is None else C.c_void_p(t.data_ptr())


@dataclass
class BatchResult:
    x: np.ndarray        # (B, N, Tm)
    status: np.ndarray   # (B,) int32
    iters: np.ndarray    # (B,) int32
    pri_res: np.ndarray
    dua_res: np.ndarray
    obj: np.ndarray
    kernel_ms: float = float("nan")   # sum of the HIP-event durations of the call's launches (chunks of the pipelined
                                      # entry overlap on the GPU: an upper bound of the time the GPU was busy)
    y: Optional[np.ndarray] = None   # (B, Mg, Tm) multipliers of the site rows (when asked for): warm_y of a later solve
    x_dev: Optional[object] = None   # the device tensor (B, N, Tm) that also received x (acnqp_results.x_dev), when one was given
    handle: Optional[object] = None  # the SiteHandle that solved it (set by AdaptiveChargingOptimization.solve_table)


@dataclass
class DualResult:
    """The dual report of a batch of answers (acnqp_duals_host / acnqp_duals_device, include/acn_qp.h), in the units of the
    C ABI (minimisation form, energy rows in A-periods)."""
    mu: np.ndarray       # (B, K, N) multiplier of each session's energy row (layout of s_cap; 0 for an empty slot)
    z: Optional[np.ndarray]   # (B, N, Tm) multipliers of the rate bounds: > 0 of ub, < 0 of lb (None: not asked for)
    stat: np.ndarray     # (B,) natural residual |x - clip(v - mu)|_inf
    energy: np.ndarray   # (B,) worst energy-row violation / max(1, |cap|)
    site: np.ndarray     # (B,) worst site-row violation / max(1, limit)
    comp: np.ndarray     # (B,) worst multiplier x slack over the site rows (oracle-free KKT check, scaled as documented)


@dataclass
class PilotPlan:
    """The arrays of ``acnqp_pilot_plan`` (include/acn_qp.h): numpy arrays for ``SiteHandle.pilots``, torch tensors on the
    handle's GPU (``to_device``) for ``SiteHandle.pilots_device``.  ``postprocessing.pilot_plan_arrays`` builds one."""
    mode: int
    B: int
    Tm: int
    N: int
    max_pilot: Optional[object] = None   # (N,)
    levels: Optional[object] = None      # (N, L) ascending, padded with +inf
    cre: Optional[object] = None         # (M, N)
    cim: Optional[object] = None
    limits: Optional[object] = None      # (M,)
    sess_seg: Optional[object] = None    # (B + 1,) int32
    s_evse: Optional[object] = None      # (S,) int32
    s_arrived: Optional[object] = None   # (S,) uint8
    s_cap: Optional[object] = None       # (S,)

    _ARRAYS = ("cre", "cim", "limits", "max_pilot", "levels", "sess_seg", "s_evse", "s_arrived", "s_cap")

    def to_device(self, device) -> "PilotPlan":
        import torch

        moved = {k: None if getattr(self, k) is None else torch.from_numpy(np.ascontiguousarray(getattr(self, k))).to(device)
                 for k in self._ARRAYS}
        return PilotPlan(self.mode, self.B, self.Tm, self.N, **moved)

    def _struct(self, batch=None, t_max=None) -> "_PilotPlan":
        def ptr(a):
            if a is None or (hasattr(a, "numel") and a.numel() == 0) or (isinstance(a, np.ndarray) and a.size == 0):
                return None
            return C.c_void_p(a.data_ptr()) if hasattr(a, "data_ptr") else _ptr(a)

        M = 0 if self.cre is None else int(self.cre.shape[0])
        L = 0 if self.levels is None else int(self.levels.shape[1])
        S = 0 if self.s_evse is None else int(self.s_evse.shape[0])
        return _PilotPlan(int(self.B if batch is None else batch), int(self.Tm if t_max is None else t_max), self.N, M, L, S,
                          self.mode, *[ptr(getattr(self, k)) for k in self._ARRAYS])


@dataclass
class AdvancePlan:
    """The arrays of ``acnqp_advance_plan`` (include/acn_qp.h): numpy arrays for ``SiteHandle.advance``, torch tensors on the
    handle's GPU (``to_device``) for ``SiteHandle.advance_device``.  ``a_seg`` may hold one row of B + 1 entries per step
    (``(steps, B + 1)``, absolute record indices): ``seg_row`` picks the step's.  ``rollout.FleetTable`` builds one.
    ``c_coef, c_weight, c_series``: the clock cost of rule 6b (``acnqp_clock_cost``); all None is the plain advance, all
    given goes through ``acnqp_advance_priced_device / _host``."""
    q_table: object                       # (H, N, Tm)
    h_scal: object                        # (H, 3) pdiag, lf, dc
    h_row: object                         # (Tm + 1,) int32
    done_tol: float
    kw_per_amp: float
    peak_series: Optional[object] = None  # (B, P)
    a_seg: Optional[object] = None        # (B + 1,) or (rows, B + 1) int32
    a_evse: Optional[object] = None       # (A,) int32
    a_slot: Optional[object] = None
    a_len: Optional[object] = None
    a_cap: Optional[object] = None        # (A,)
    a_rate_seg: Optional[object] = None   # (A + 1,) int32
    a_min: Optional[object] = None        # (R,)
    a_max: Optional[object] = None
    warm_arrival_gain: float = 0.0        # rule 9: != 0 starts an admitted session at -gain * q' instead of the shifted x
    c_coef: Optional[float] = None        # rule 6b: q' += c_coef * (c_weight[i] * c_series[b][step + 1 + t])
    c_weight: Optional[object] = None     # (N,)
    c_series: Optional[object] = None     # (B, P)

    _COST = ("c_weight", "c_series")
    _ARRAYS = ("q_table", "h_scal", "h_row", "peak_series", "a_seg", "a_evse", "a_slot", "a_len", "a_cap", "a_rate_seg", "a_min", "a_max")
    _INT = ("h_row", "a_seg", "a_evse", "a_slot", "a_len", "a_rate_seg")

    def to_device(self, device) -> "AdvancePlan":
        import torch

        moved = {}
        for k in self._ARRAYS:
            a = getattr(self, k)
            moved[k] = None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32 if k in self._INT else np.float64)).to(device)
        for k in self._COST:
            a = getattr(self, k)
            moved[k] = None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(device)
        return AdvancePlan(done_tol=self.done_tol, kw_per_amp=self.kw_per_amp, warm_arrival_gain=self.warm_arrival_gain, c_coef=self.c_coef, **moved)

    def _struct(self, N: int, Mg: int, step: int, seg_row: int = 0, keep=None) -> "_AdvancePlan":
        def ptr(k, row=None):
            a = getattr(self, k)
            if a is None or (a.numel() if hasattr(a, "numel") else a.size) == 0:
                return None
            if row is not None and a.ndim == 2:
                a = a[row]
            if hasattr(a, "data_ptr"):
                return C.c_void_p(a.data_ptr())
            a = np.ascontiguousarray(a, np.int32 if k in self._INT else np.float64)
            if keep is not None:
                keep.append(a)
            return _ptr(a)

        A = 0 if self.a_evse is None else int(self.a_evse.shape[0])
        R = 0 if self.a_min is None else int(self.a_min.shape[0])
        P = 0 if self.peak_series is None else int(self.peak_series.shape[1])
        return _AdvancePlan(int(N), int(Mg), int(self.q_table.shape[0]), int(step), P, A, R, float(self.done_tol), float(self.kw_per_amp),
                            float(self.warm_arrival_gain),
                            ptr("q_table"), ptr("h_scal"), ptr("h_row"), ptr("peak_series"), ptr("a_seg", seg_row) if A else None,
                            ptr("a_evse"), ptr("a_slot"), ptr("a_len"), ptr("a_cap"), ptr("a_rate_seg"), ptr("a_min"), ptr("a_max"))

    def _cost_struct(self, N: int, keep=None) -> Optional["ClockCost"]:
        """the ``acnqp_clock_cost`` of the plan, or None (the plain advance) when no c_ field is set"""
        given = [self.c_coef is not None, self.c_weight is not None, self.c_series is not None]
        if not any(given):
            return None
        if not all(given):
            raise ValueError("a clock cost needs c_coef, c_weight and c_series")
        if self.c_series.ndim != 2:
            raise ValueError("c_series must have shape (B, P)")
        ptrs = []
        for k in self._COST:
            a = getattr(self, k)
            if hasattr(a, "data_ptr"):
                if a.element_size() != 8 or not a.is_contiguous():
                    raise ValueError(f"{k} must be a contiguous float64 tensor")
                ptrs.append(C.c_void_p(a.data_ptr()) if a.numel() else None)
            else:
                a = np.ascontiguousarray(a, np.float64)
                if keep is not None:
                    keep.append(a)
                ptrs.append(_ptr(a) if a.size else None)
        return ClockCost(int(N), int(self.c_series.shape[1]), float(self.c_coef), *ptrs)


@dataclass
class PreparePlan:
    """The arrays of ``acnqp_prepare_plan`` (include/acn_qp.h): numpy arrays for ``SiteHandle.prepare_host``, torch tensors on the
    handle's GPU (``to_device``) for ``SiteHandle.prepare_device``.  ``key`` may hold one (B, N) block per step
    (``(steps, B, N)``): ``key_row`` picks the step's.  ``min_pilot=None``: no minimum-rate step."""
    key: object                          # (B, N) or (rows, B, N) int32: list position of the session on each EVSE
    cre: Optional[object] = None         # (M, N) the site in the SOC form of ``PilotPlan``
    cim: Optional[object] = None
    limits: Optional[object] = None      # (M,)
    min_pilot: Optional[object] = None   # (N,)

    _ARRAYS = ("key", "cre", "cim", "limits", "min_pilot")

    def to_device(self, device) -> "PreparePlan":
        import torch

        moved = {}
        for k in self._ARRAYS:
            a = getattr(self, k)
            moved[k] = None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32 if k == "key" else np.float64)).to(device)
        return PreparePlan(**moved)

    def _struct(self, N: int, key_row=None, min_rates: bool = True, keep=None) -> "_PreparePlan":
        def ptr(k):
            a = getattr(self, k)
            if a is None or (a.numel() if hasattr(a, "numel") else a.size) == 0:
                return None
            if k == "key" and a.ndim == 3:
                a = a[0 if key_row is None else key_row]
            if hasattr(a, "data_ptr"):
                return C.c_void_p(a.data_ptr())
            a = np.ascontiguousarray(a, np.int32 if k == "key" else np.float64)
            if keep is not None:
                keep.append(a)
            return _ptr(a)

        M = 0 if self.cre is None else int(self.cre.shape[0])
        return _PreparePlan(int(N), M, ptr("key"), ptr("cre"), ptr("cim"), ptr("limits"), ptr("min_pilot") if min_rates else None)


class _PinnedBlock:
    """Owner of one acnqp_host_alloc block; freed when the last numpy view of it is gone."""

    def __init__(self, nbytes: int):
        self._lib = load_library()
        self.nbytes = int(nbytes)
        self.ptr = self._lib.acnqp_host_alloc(self.nbytes)
        if not self.ptr:
            raise MemoryError(f"acnqp_host_alloc({nbytes}) failed: {self._lib.acnqp_last_error().decode()}")

    def __del__(self):
        try:
            if self.ptr:
                self._lib.acnqp_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float64) -> np.ndarray:
    """A zero-filled numpy array in pinned host memory (acnqp_host_alloc): the library's H2D / D2H copies of such
    arrays are direct DMA.  Same call shape as ``np.zeros``; use it as ``alloc=`` of ``builder.build_batch``."""
    dt = np.dtype(dtype)
    shape = (int(shape),) if np.isscalar(shape) else tuple(int(k) for k in shape)
    n = int(np.prod(shape)) if shape else 1
    block = _PinnedBlock(max(n * dt.itemsize, 1))
    buf = (C.c_char * block.nbytes).from_address(block.ptr)
    buf._owner = block   # numpy keeps `buf` alive through .base; `buf` keeps the block
    a = np.frombuffer(buf, dtype=dt, count=n).reshape(shape)
    a[...] = 0
    return a


class SiteHandle:
    """One ``acnqp_handle``: a site uploaded to one GPU."""

    def __init__(self, site: SiteData, device: int = 0):
        self._lib = load_library()
        self.site = site
        self.device = int(device)
        G = np.ascontiguousarray(site.G, dtype=np.float64)
        lim = np.ascontiguousarray(site.limits, dtype=np.float64)
        desc = _Site(
            site.N, site.M, site.Mg, 1 if site.cone == CONE_SOC else 0, 1 if site.has_peak else 0,
            1 if site.has_flat else 0, 1 if site.has_max else 0,
            _ptr(G) if G.size else None, _ptr(lim) if lim.size else None,
        )
        h = C.c_void_p()
        _check(self._lib.acnqp_create(C.byref(desc), self.device, C.byref(h)), "acnqp_create")
        self._h = h
        self._launches_seen = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.acnqp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host buffers -----------------------------------------------------------
    def _check_site(self, batch: ProblemBatch):
        if batch.site is not self.site and (
            batch.site.Mg != self.site.Mg or batch.site.N != self.site.N or batch.site.cone != self.site.cone
            or batch.site.has_flat != self.site.has_flat or batch.site.has_max != self.site.has_max
        ):
            raise ValueError("batch was built for a different site than this handle")

    def _marshal(self, batch: ProblemBatch, pinned: bool, x_dev=None, warm=None, want_y=False):
        """ctypes views of one batch: (_Problems, _Results, BatchResult, keep-alive list).  Arrays that already
        are C-contiguous with the ABI's dtype are passed as they are (e.g. pinned arrays from ``pinned_empty``)."""
        B, N, Tm = batch.B, batch.N, batch.Tm
        arrs = dict(
            horizon=np.ascontiguousarray(batch.T, np.int32),
            lb=np.ascontiguousarray(batch.lb, np.float64),
            ub=np.ascontiguousarray(batch.ub, np.float64),
            q=np.ascontiguousarray(batch.q, np.float64),
            pdiag=np.ascontiguousarray(batch.pdiag, np.float64),
            s_off=np.ascontiguousarray(batch.s_off, np.int32),
            s_len=np.ascontiguousarray(batch.s_len, np.int32),
            s_cap=np.ascontiguousarray(batch.s_cap, np.float64),
            s_eq=np.ascontiguousarray(batch.s_eq, np.uint8),
        )
        peak = None if batch.peak is None else np.ascontiguousarray(batch.peak, np.float64)
        lf = np.ascontiguousarray(batch.lf, np.float64) if self.site.has_flat else None
        dc = np.ascontiguousarray(batch.dc, np.float64) if self.site.has_max else None
        dfl = np.ascontiguousarray(batch.dfloor, np.float64) if self.site.has_max else None
        wx = wy = None
        if warm is not None:
            wx = np.ascontiguousarray(warm[0], np.float64)
            wy = np.ascontiguousarray(warm[1], np.float64)
            if wx.shape != (B, N, Tm) or wy.shape != (B, self.site.Mg, Tm):
                raise ValueError(f"warm start arrays must have shapes {(B, N, Tm)} and {(B, self.site.Mg, Tm)}")
        p = _Problems(B, Tm, batch.K, *[_ptr(arrs[k]) for k in
                                       ("horizon", "lb", "ub", "q", "pdiag", "s_off", "s_len", "s_cap", "s_eq")],
                      _ptr(peak), _ptr(lf), _ptr(dc), _ptr(dfl), _ptr(wx), _ptr(wy))
        new = pinned_empty if pinned else (lambda shape, dtype=np.float64: np.zeros(shape, dtype))
        res = BatchResult(
            new((B, N, Tm)), new(B, np.int32), new(B, np.int32), new(B), new(B), new(B),
        )
        if want_y:
            res.y = new((B, self.site.Mg, Tm))
        r = _Results(_ptr(res.x), _ptr(res.status), _ptr(res.iters), _ptr(res.pri_res), _ptr(res.dua_res), _ptr(res.obj),
                     _ptr(res.y), None if x_dev is None else C.c_void_p(int(x_dev)))
        return p, r, res, (arrs, peak, lf, dc, dfl, wx, wy)

    def _finish(self, batch: ProblemBatch, res: "BatchResult"):
        if self.site.has_flat:   # the kernel's obj covers pdiag and q; add 1/2 lf sum_t (v' x_t)^2
            v = self.site.G[self.site.flat_row]
            res.obj = res.obj + 0.5 * batch.lf * np.einsum("n,bnt->bt", v, res.x).__pow__(2).sum(axis=1)
        if self.site.has_max:   # ... and dc * max(max_t v' x_t, dfloor)
            v = self.site.G[self.site.max_row]
            agg = np.einsum("n,bnt->bt", v, res.x)
            res.obj = res.obj + batch.dc * np.maximum(agg.max(axis=1), batch.dfloor)
        if batch.presolve_status is not None:
            res.status[batch.presolve_status != 0] = STATUS_EMPTY_SET
        return res

    def solve(self, batch: ProblemBatch, options: Optional[Options] = None, pinned_results: bool = False,
              warm=None, want_y: bool = False) -> BatchResult:
        """acnqp_solve_batch: one batch, host buffers in and out, synchronous (pipelined in chunks inside).
        ``warm = (x0, y0)``: optional warm start (an earlier schedule (B, N, Tm) and its ``BatchResult.y`` (B, Mg, Tm),
        shifted by the caller); ``want_y``: also return the site-row multipliers ``y`` for a later warm start.
        Problems a pass leaves SOLVED_INACCURATE / MAX_ITER on a plateau are re-solved inside the library
        (``options.retry_passes``, include/acn_qp.h) -- every entry point behaves the same."""
        self._check_site(batch)
        o = options if options is not None else default_options()
        p, r, res, keep = self._marshal(batch, pinned_results, warm=warm, want_y=want_y)
        self.kernel_times()   # forget earlier launches: kernel_ms below is the sum over THIS call's launches (chunks)
        self._launches_seen = int(self._lib.acnqp_launch_count(self._h))
        _check(self._lib.acnqp_solve_batch(self._h, C.byref(p), C.byref(o), C.byref(r)), "acnqp_solve_batch")
        del keep
        res.kernel_ms = self._kernel_ms_of_call()
        return self._finish(batch, res)

    def solve_table(self, plan, options: Optional[Options] = None, pinned_results: bool = False, want_y: bool = False,
                    out: Optional["BatchResult"] = None, x_dev=None) -> "BatchResult":
        """acnqp_solve_table: a ``builder.TablePlan`` (sessions + one linear cost per horizon) in, schedules out; the
        dense (B, N, Tm) problem arrays are formed on the device.  Same results as ``solve(plan.expand())``.
        ``out``: a BatchResult of an earlier call of the same shape to write into (a service that solves every control
        period keeps its -- pinned -- result arrays instead of allocating 85 MB per call).  ``x_dev``: a float64 device tensor
        (B, N, Tm) on the handle's GPU that also receives the schedules (acnqp_results.x_dev); it comes back as
        ``BatchResult.x_dev``."""
        if plan.site is not self.site and (plan.site.N, plan.site.Mg, plan.site.cone) != (self.site.N, self.site.Mg, self.site.cone):
            raise ValueError("plan was built for another site")
        o = options if options is not None else default_options()
        B, N, Tm = plan.B, plan.N, plan.Tm
        c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
        keep = dict(
            horizon=c(plan.T, np.int32), q_index=c(plan.q_index, np.int32), q_table=c(plan.q_table, np.float64),
            pdiag=c(plan.pdiag, np.float64), s_eq=c(plan.s_eq, np.uint8), peak=c(plan.peak, np.float64) if self.site.has_peak else None,
            lf=c(plan.lf, np.float64) if self.site.has_flat else None, dc=c(plan.dc, np.float64) if self.site.has_max else None,
            dfloor=c(plan.dfloor, np.float64) if self.site.has_max else None, sess_seg=c(plan.sess_seg, np.int32),
            s_evse=c(plan.s_evse, np.int32), s_slot=c(plan.s_slot, np.int32), s_off=c(plan.s_off, np.int32), s_len=c(plan.s_len, np.int32),
            s_cap=c(plan.s_cap, np.float64), rate_seg=c(plan.rate_seg, np.int32), min_rates=c(plan.min_rates, np.float64),
            max_rates=c(plan.max_rates, np.float64))
        t = _Table(B, Tm, plan.K, plan.S, len(plan.q_table), *[_ptr(keep[k]) for k in (
            "horizon", "q_index", "q_table", "pdiag", "s_eq", "peak", "lf", "dc", "dfloor", "sess_seg", "s_evse", "s_slot", "s_off",
            "s_len", "s_cap", "rate_seg", "min_rates", "max_rates")])
        new = pinned_empty if pinned_results else (lambda shape, dtype=np.float64: np.zeros(shape, dtype))
        if out is not None and out.x.shape == (B, N, Tm) and (not want_y or (out.y is not None and out.y.shape == (B, self.site.Mg, Tm))):
            res = out
        else:
            res = BatchResult(new((B, N, Tm)), new(B, np.int32), new(B, np.int32), new(B), new(B), new(B))
            if want_y:
                res.y = new((B, self.site.Mg, Tm))
        r = _Results(_ptr(res.x), _ptr(res.status), _ptr(res.iters), _ptr(res.pri_res), _ptr(res.dua_res), _ptr(res.obj),
                     _ptr(res.y) if want_y else None, None if x_dev is None else C.c_void_p(x_dev.data_ptr()))
        if x_dev is not None and (tuple(x_dev.shape) != (B, N, Tm) or not x_dev.is_contiguous() or x_dev.element_size() != 8):
            raise ValueError(f"x_dev must be a contiguous float64 tensor of shape {(B, N, Tm)}")
        res.x_dev = x_dev
        self.kernel_times()
        self._launches_seen = int(self._lib.acnqp_launch_count(self._h))
        _check(self._lib.acnqp_solve_table(self._h, C.byref(t), C.byref(o), C.byref(r)), "acnqp_solve_table")
        del keep
        res.kernel_ms = self._kernel_ms_of_call()
        return self._finish(plan, res)

    def solve_many(self, batches, options: Optional[Options] = None, pinned_results: bool = True, want_y=None, warm=None):
        """acnqp_solve_batches: several independent batches in ONE pipelined pass (shared launches, overlapped
        copies).  Returns one BatchResult per batch.  ``want_y[g]`` / ``warm[g]``: optional per-batch multiplier output
        and warm start, as ``solve`` takes them (None = no batch wants / has one)."""
        o = options if options is not None else default_options()
        n = len(batches)
        want_y = [False] * n if want_y is None else list(want_y)
        warm = [None] * n if warm is None else list(warm)
        if len(want_y) != n or len(warm) != n:
            raise ValueError("want_y and warm need one entry per batch")
        P, R = (_Problems * n)(), (_Results * n)()
        results, keep = [], []
        for g, batch in enumerate(batches):
            self._check_site(batch)
            P[g], R[g], res, k = self._marshal(batch, pinned_results, warm=warm[g], want_y=bool(want_y[g]))
            results.append(res)
            keep.append(k)
        _check(self._lib.acnqp_solve_batches(self._h, n, P, C.byref(o), R), "acnqp_solve_batches")
        del keep
        return [self._finish(b, r) for b, r in zip(batches, results)]

    def prepare_many(self, batches, pinned_results: bool = True, x_dev_ptrs=None):
        """Marshal once, solve repeatedly (bench.py): returns a callable ``run(options)`` that re-submits the same
        host buffers through acnqp_solve_batches and the list of BatchResults it fills.  ``x_dev_ptrs[g]``: optional
        device address that also receives batch g's schedules (acnqp_results.x_dev)."""
        n = len(batches)
        P, R = (_Problems * n)(), (_Results * n)()
        results, keep = [], []
        for g, batch in enumerate(batches):
            self._check_site(batch)
            P[g], R[g], res, k = self._marshal(batch, pinned_results, None if x_dev_ptrs is None else x_dev_ptrs[g])
            results.append(res)
            keep.append(k)

        def run(options: Options):
            _check(self._lib.acnqp_solve_batches(self._h, n, P, C.byref(options), R), "acnqp_solve_batches")
            return results

        run.keep = keep
        return run, results

    # -- device buffers (torch tensors or any object with data_ptr()) --------------
    def solve_device(self, dev: "DeviceBatch", options: Optional[Options] = None, stream: int = 0, warm_x=None, warm_y=None) -> None:
        """acnqp_solve_batch_device on a ``DeviceBatch``; asynchronous on ``stream``.  ``warm_x`` (B, N, Tm) and ``warm_y``
        (B, Mg, Tm): optional float64 device tensors of a warm start (both or neither; none = cold, NULL in the ABI)."""
        o = options if options is not None else default_options()
        if (warm_x is None) != (warm_y is None):
            raise ValueError("warm_x and warm_y go together (both or neither)")
        if warm_x is not None and (tuple(warm_x.shape) != (dev.B, dev.N, dev.Tm) or tuple(warm_y.shape) != (dev.B, self.site.Mg, dev.Tm)
                                   or not warm_x.is_contiguous() or not warm_y.is_contiguous()
                                   or warm_x.element_size() != 8 or warm_y.element_size() != 8):
            raise ValueError(f"warm start tensors must be contiguous float64 of shapes {(dev.B, dev.N, dev.Tm)} and {(dev.B, self.site.Mg, dev.Tm)}")
        p = _Problems(
            dev.B, dev.Tm, dev.K,
            dev.horizon.data_ptr(), dev.lb.data_ptr(), dev.ub.data_ptr(), dev.q.data_ptr(), dev.pdiag.data_ptr(),
            dev.s_off.data_ptr(), dev.s_len.data_ptr(), dev.s_cap.data_ptr(), dev.s_eq.data_ptr(),
            None if dev.peak is None else dev.peak.data_ptr(),
            dev.lf.data_ptr() if self.site.has_flat else None,
            dev.dc.data_ptr() if self.site.has_max else None,
            dev.dfloor.data_ptr() if self.site.has_max else None,
            None if warm_x is None else warm_x.data_ptr(), None if warm_y is None else warm_y.data_ptr(),
        )
        r = _Results(dev.x.data_ptr(), dev.status.data_ptr(), dev.iters.data_ptr(),
                     dev.pri_res.data_ptr(), dev.dua_res.data_ptr(), dev.obj.data_ptr(),
                     None if dev.y is None else dev.y.data_ptr(), None)
        _check(
            self._lib.acnqp_solve_batch_device(self._h, C.byref(p), C.byref(o), C.byref(r), C.c_void_p(stream)),
            "acnqp_solve_batch_device",
        )

    # -- dual report (acn_qp_duals.hpp) -------------------------------------------------------------------------------
    def duals(self, batch: ProblemBatch, res: "BatchResult", options: Optional[Options] = None, want_z: bool = True) -> DualResult:
        """acnqp_duals_host: the multipliers of the energy rows and rate bounds of the answers ``res`` (a BatchResult with
        ``y``, i.e. solved with ``want_y=True``) to ``batch``, and their KKT residuals, computed on the GPU.  ``options``:
        the options of the solve (``reg_rel`` is read)."""
        self._check_site(batch)
        B, N, Tm, K = batch.B, batch.N, batch.Tm, batch.K
        if self.site.Mg > 0 and res.y is None:
            raise ValueError("duals need the site-row multipliers: solve with want_y=True")
        o = options if options is not None else default_options()
        p, _, _, keep = self._marshal(batch, False)
        x = np.ascontiguousarray(res.x, np.float64)
        y = None if res.y is None else np.ascontiguousarray(res.y, np.float64)
        st = np.ascontiguousarray(res.status, np.int32)
        if x.shape != (B, N, Tm) or st.shape != (B,) or (y is not None and y.shape != (B, self.site.Mg, Tm)):
            raise ValueError("result arrays do not match the batch")
        mu, z, r = np.zeros((B, K, N)), (np.zeros((B, N, Tm)) if want_z else None), np.zeros((B, 4))
        d = _Duals(_ptr(mu), _ptr(z), _ptr(r))
        _check(self._lib.acnqp_duals_host(self._h, C.byref(p), C.byref(o), _ptr(x), _ptr(y), _ptr(st), C.byref(d)), "acnqp_duals_host")
        del keep
        return DualResult(mu, z, r[:, 0].copy(), r[:, 1].copy(), r[:, 2].copy(), r[:, 3].copy())

    def duals_device(self, dev: "DeviceBatch", mu, res, z=None, options: Optional[Options] = None, stream: int = 0,
                     use_status: bool = True) -> None:
        """acnqp_duals_device: the same for a ``DeviceBatch`` after ``solve_device`` (it needs ``want_y=True`` on a site with
        rows); ``mu`` (B, K, N), ``res`` (B, 4) and the optional ``z`` (B, N, Tm) are float64 device tensors that receive the
        report.  Asynchronous on ``stream``."""
        o = options if options is not None else default_options()
        if self.site.Mg > 0 and dev.y is None:
            raise ValueError("duals need the site-row multipliers: DeviceBatch(..., want_y=True)")
        p = _Problems(
            dev.B, dev.Tm, dev.K,
            dev.horizon.data_ptr(), dev.lb.data_ptr(), dev.ub.data_ptr(), dev.q.data_ptr(), dev.pdiag.data_ptr(),
            dev.s_off.data_ptr(), dev.s_len.data_ptr(), dev.s_cap.data_ptr(), dev.s_eq.data_ptr(),
            None if dev.peak is None else dev.peak.data_ptr(),
            dev.lf.data_ptr() if self.site.has_flat else None,
            dev.dc.data_ptr() if self.site.has_max else None,
            dev.dfloor.data_ptr() if self.site.has_max else None,
            None, None,
        )
        d = _Duals(mu.data_ptr(), None if z is None else z.data_ptr(), res.data_ptr())
        _check(
            self._lib.acnqp_duals_device(self._h, C.byref(p), C.byref(o), C.c_void_p(dev.x.data_ptr()),
                                         None if dev.y is None else C.c_void_p(dev.y.data_ptr()),
                                         C.c_void_p(dev.status.data_ptr()) if use_status else None, C.byref(d), C.c_void_p(stream)),
            "acnqp_duals_device",
        )

    # -- pilot signals (acn_qp_pilots.hpp) ----------------------------------------------------------------------------
    def pilots(self, plan: PilotPlan, x: np.ndarray, want_pilots: bool = True, want_first: bool = True):
        """acnqp_pilots_host: the pilots of the schedules ``x`` (B, N, Tm) under ``plan`` (numpy arrays), computed on the
        GPU.  Returns ``(pilots (B, N, Tm) or None, first (B, N) or None, visits (B,) int32)``."""
        x = np.ascontiguousarray(x, np.float64)
        if x.ndim != 3 or x.shape[1] != plan.N:
            raise ValueError("x must have the shape (B, N, Tm) of the plan's site")
        B, N, Tm = x.shape
        pil = np.empty((B, N, Tm)) if want_pilots else None
        first = np.empty((B, N)) if want_first else None
        visits = np.empty(B, np.int32)
        p = plan._struct(B, Tm)
        out = _Pilots(_ptr(pil), _ptr(first), _ptr(visits))
        _check(self._lib.acnqp_pilots_host(self._h, C.byref(p), _ptr(x), C.byref(out)), "acnqp_pilots_host")
        return pil, first, visits

    def pilots_device(self, plan: PilotPlan, x, pilots=None, first=None, visits=None, stream: int = 0) -> None:
        """acnqp_pilots_device: the same on device memory -- ``plan`` from ``PilotPlan.to_device``, ``x`` (B, N, Tm) and the
        outputs ``pilots`` (B, N, Tm), ``first`` (B, N) (float64) and ``visits`` (B,) (int32) torch tensors on the handle's
        GPU; at least one of ``pilots`` / ``first``.  Asynchronous on ``stream``."""
        import torch

        here = torch.device("cuda", self.device)

        def want(t, name, dtype, shape=None):
            if t is None:
                return
            if not isinstance(t, torch.Tensor) or t.device != here or t.dtype != dtype or not t.is_contiguous() or (
                    shape is not None and tuple(t.shape) != tuple(shape)):
                raise ValueError(f"{name} must be a contiguous {dtype} tensor on {here}" + ("" if shape is None else f" of shape {tuple(shape)}"))

        want(x, "x", torch.float64)
        if x.dim() != 3 or x.shape[1] != plan.N:
            raise ValueError("x must have the shape (B, N, Tm) of the plan's site")
        B, N, Tm = x.shape
        want(pilots, "pilots", torch.float64, (B, N, Tm))
        want(first, "first", torch.float64, (B, N))
        want(visits, "visits", torch.int32, (B,))
        M = 0 if plan.cre is None else int(plan.cre.shape[0])
        L = 0 if plan.levels is None else int(plan.levels.shape[1])
        want(plan.max_pilot, "plan.max_pilot", torch.float64, (N,))
        want(plan.levels, "plan.levels", torch.float64, (N, L))
        want(plan.cre, "plan.cre", torch.float64, (M, N))
        want(plan.cim, "plan.cim", torch.float64, (M, N))
        want(plan.limits, "plan.limits", torch.float64, (M,))
        want(plan.sess_seg, "plan.sess_seg", torch.int32, (B + 1,))
        S = 0 if plan.s_evse is None else int(plan.s_evse.shape[0])
        want(plan.s_evse, "plan.s_evse", torch.int32, (S,))
        want(plan.s_arrived, "plan.s_arrived", torch.uint8, (S,))
        want(plan.s_cap, "plan.s_cap", torch.float64, (S,))
        p = plan._struct(B, Tm)
        out = _Pilots(_dptr(pilots), _dptr(first), _dptr(visits))
        _check(self._lib.acnqp_pilots_device(self._h, C.byref(p), _dptr(x), C.byref(out), C.c_void_p(stream)), "acnqp_pilots_device")

    # -- time passes (acn_qp_advance.hpp) -------------------------------------------------------------------------------
    _NEXT = ("horizon", "lb", "ub", "q", "pdiag", "s_off", "s_len", "s_cap", "peak", "lf", "dc", "dfloor")

    def advance(self, cur: dict, applied, plan: AdvancePlan, step: int, status=None, x=None, y=None, want_warm: bool = False,
                seg_row: int = 0) -> dict:
        """acnqp_advance_host: the next period's problems of the state ``cur`` -- a dict of numpy arrays ``lb, ub`` (B, N, Tm),
        ``s_off, s_len, s_cap`` (B, K, N) and, on a site with a max row, ``dfloor`` (B,) -- after the pilots ``applied`` (B, N)
        of period ``step``, under ``plan`` (numpy arrays).  Returns a dict of the same layout with ``horizon, q, pdiag, lf, dc,
        peak, flags`` added and, with ``want_warm``, ``warm_x`` / ``warm_y`` shifted from ``x`` (B, N, Tm) / ``y`` (B, Mg, Tm)."""
        f8 = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
        i4 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
        lb, ub, off, ln, cap = f8(cur["lb"]), f8(cur["ub"]), i4(cur["s_off"]), i4(cur["s_len"]), f8(cur["s_cap"])
        if lb.ndim != 3 or lb.shape[1] != self.site.N or ub.shape != lb.shape or off.ndim != 3 or off.shape != ln.shape or off.shape != cap.shape:
            raise ValueError("cur needs lb, ub of shape (B, N, Tm) and s_off, s_len, s_cap of shape (B, K, N) for the handle's site")
        B, N, Tm = lb.shape
        K, Mg = off.shape[1], self.site.Mg
        dfl = f8(cur.get("dfloor")) if self.site.has_max else None
        app, stat, xs, ys = f8(applied), i4(status), f8(x) if want_warm else None, f8(y) if want_warm and Mg else None
        out = dict(horizon=np.empty(B, np.int32), lb=np.empty((B, N, Tm)), ub=np.empty((B, N, Tm)), q=np.empty((B, N, Tm)),
                   pdiag=np.empty(B), s_off=np.empty((B, K, N), np.int32), s_len=np.empty((B, K, N), np.int32), s_cap=np.empty((B, K, N)),
                   peak=np.empty((B, Tm)) if self.site.has_peak else None, lf=np.empty(B) if self.site.has_flat else None,
                   dc=np.empty(B) if self.site.has_max else None, dfloor=np.empty(B) if self.site.has_max else None,
                   warm_x=np.empty((B, N, Tm)) if xs is not None else None, warm_y=np.empty((B, Mg, Tm)) if ys is not None else None)
        flags = np.empty(B, np.int32)
        p = _Problems(B, Tm, K, None, _ptr(lb), _ptr(ub), None, None, _ptr(off), _ptr(ln), _ptr(cap), None, None, None, None, _ptr(dfl), None, None)
        keep = []
        pl = plan._struct(N, Mg, step, seg_row, keep)
        nx = _Next(*[_ptr(out[k]) for k in self._NEXT + ("warm_x", "warm_y")])
        cost = plan._cost_struct(N, keep)
        if cost is not None and plan.c_series.shape[0] != B:
            raise ValueError(f"c_series has {plan.c_series.shape[0]} rows, the batch has {B} problems")
        if cost is None:
            _check(self._lib.acnqp_advance_host(self._h, C.byref(p), _ptr(app), _ptr(stat), _ptr(xs), _ptr(ys), C.byref(pl), C.byref(nx),
                                                _ptr(flags)), "acnqp_advance_host")
        else:
            _check(self._lib.acnqp_advance_priced_host(self._h, C.byref(p), _ptr(app), _ptr(stat), _ptr(xs), _ptr(ys), C.byref(pl),
                                                       C.byref(cost), C.byref(nx), _ptr(flags)), "acnqp_advance_priced_host")
        del keep
        out["flags"] = flags
        return {k: v for k, v in out.items() if v is not None}

    def advance_device(self, cur: "DeviceBatch", nxt: "DeviceBatch", applied, plan: AdvancePlan, step: int, flags, use_status: bool = True,
                       warm_x=None, warm_y=None, stream: int = 0, seg_row: int = 0) -> None:
        """acnqp_advance_device: ``nxt`` (a second ``DeviceBatch`` of the same shape, e.g. ``DeviceBatch.empty``: the kernel
        ping-pongs between two buffer sets, nothing may alias) receives the next period's problems of ``cur`` after the pilots
        ``applied`` (B, N) of period ``step``; ``flags`` (B,) int32; ``plan`` from ``AdvancePlan.to_device``.  ``use_status``:
        a problem ``cur.status`` does not call solved delivers nothing.  ``warm_x`` / ``warm_y``: optional device tensors that
        receive ``cur.x`` / ``cur.y`` shifted by one period.  Asynchronous on ``stream``."""
        if (cur.B, cur.N, cur.Tm, cur.K) != (nxt.B, nxt.N, nxt.Tm, nxt.K):
            raise ValueError("cur and nxt must have the same shape (B, N, Tm, K)")
        if warm_y is not None and cur.y is None:
            raise ValueError("warm_y needs the site-row multipliers: DeviceBatch(..., want_y=True)")
        if tuple(applied.shape) != (cur.B, cur.N) or applied.element_size() != 8 or not applied.is_contiguous():
            raise ValueError(f"applied must be a contiguous float64 tensor of shape {(cur.B, cur.N)}")
        if tuple(flags.shape) != (cur.B,) or flags.element_size() != 4 or not flags.is_contiguous():
            raise ValueError(f"flags must be a contiguous int32 tensor of shape {(cur.B,)}")
        p = _Problems(cur.B, cur.Tm, cur.K, _dptr(cur.horizon), _dptr(cur.lb), _dptr(cur.ub), _dptr(cur.q), _dptr(cur.pdiag), _dptr(cur.s_off),
                      _dptr(cur.s_len), _dptr(cur.s_cap), _dptr(cur.s_eq), _dptr(cur.peak), _dptr(cur.lf), _dptr(cur.dc), _dptr(cur.dfloor), None, None)
        pl = plan._struct(cur.N, self.site.Mg, step, seg_row)
        nx = _Next(*[_dptr(getattr(nxt, k)) for k in self._NEXT], _dptr(warm_x), _dptr(warm_y))
        cost = plan._cost_struct(cur.N)
        if cost is not None and plan.c_series.shape[0] != cur.B:
            raise ValueError(f"c_series has {plan.c_series.shape[0]} rows, the batch has {cur.B} problems")
        head = (self._h, C.byref(p), _dptr(applied), _dptr(cur.status) if use_status else None,
                _dptr(cur.x) if warm_x is not None else None, _dptr(cur.y) if warm_y is not None else None, C.byref(pl))
        if cost is None:
            _check(self._lib.acnqp_advance_device(*head, C.byref(nx), _dptr(flags), C.c_void_p(stream)), "acnqp_advance_device")
        else:
            _check(self._lib.acnqp_advance_priced_device(*head, C.byref(cost), C.byref(nx), _dptr(flags), C.c_void_p(stream)),
                   "acnqp_advance_priced_device")

    # -- before the solve (acn_qp_prepare.hpp) ---------------------------------------------------------------------------
    def prepare_host(self, cur: dict, plan: PreparePlan, want_view: bool = True, min_rates: bool = True, key_row=None) -> dict:
        """acnqp_prepare_host: the state ``cur`` -- numpy arrays ``lb, ub`` (B, N, Tm) and ``s_off, s_len, s_cap`` (B, 1, N) or
        (B, N) -- under ``plan`` (numpy arrays).  Returns ``lb, ub`` (copies, period 0 changed when the plan has ``min_pilot``
        and ``min_rates``), ``flags`` (B,) and, with ``want_view``, ``v_evse, v_arrived, v_cap`` (B, N)."""
        f8 = lambda a: np.array(a, np.float64, order="C")
        i4 = lambda a: np.ascontiguousarray(a, np.int32)
        lb, ub, off, ln, cap = f8(cur["lb"]), f8(cur["ub"]), i4(cur["s_off"]), i4(cur["s_len"]), np.ascontiguousarray(cur["s_cap"], np.float64)
        if lb.ndim != 3 or lb.shape[1] != self.site.N or ub.shape != lb.shape:
            raise ValueError("cur needs lb, ub of shape (B, N, Tm) for the handle's site")
        B, N, Tm = lb.shape
        K = off.shape[1] if off.ndim == 3 else 1
        if off.size != B * K * N or ln.size != off.size or cap.size != off.size:
            raise ValueError("cur needs s_off, s_len, s_cap of shape (B, K, N)")
        view = dict(v_evse=np.empty((B, N), np.int32), v_arrived=np.empty((B, N), np.uint8), v_cap=np.empty((B, N))) if want_view else {}
        flags = np.empty(B, np.int32)
        p = _Problems(B, Tm, K, None, None, None, None, None, _ptr(off), _ptr(ln), _ptr(cap), None, None, None, None, None, None, None)
        keep = []
        pl = plan._struct(N, key_row, min_rates, keep)
        v = _PrepareView(*[_ptr(view.get(k)) for k in ("v_evse", "v_arrived", "v_cap")])
        _check(self._lib.acnqp_prepare_host(self._h, C.byref(p), C.byref(pl), _ptr(lb), _ptr(ub), C.byref(v), _ptr(flags)), "acnqp_prepare_host")
        del keep
        return dict(lb=lb, ub=ub, flags=flags, **view)

    def prepare_device(self, cur: "DeviceBatch", plan: PreparePlan, flags, v_evse=None, v_arrived=None, v_cap=None, min_rates: bool = True,
                       key_row=None, stream: int = 0) -> None:
        """acnqp_prepare_device: period 0 of ``cur.lb`` / ``cur.ub`` gets the minimum rates (when the plan has ``min_pilot`` and
        ``min_rates``), and ``v_evse`` (B, N) int32, ``v_arrived`` (B, N) uint8 and ``v_cap`` (B, N) float64 -- all three or
        none -- the session view of ``cur`` in the order of ``plan.key``; ``flags`` (B,) int32.  ``plan`` from
        ``PreparePlan.to_device``.  Asynchronous on ``stream``."""
        import torch

        here = torch.device("cuda", self.device)

        def want(t, name, dtype, shape):
            if t is None:
                return
            if not isinstance(t, torch.Tensor) or t.device != here or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
                raise ValueError(f"{name} must be a contiguous {dtype} tensor on {here} of shape {tuple(shape)}")

        B, N, Tm = cur.B, cur.N, cur.Tm
        M = 0 if plan.cre is None else int(plan.cre.shape[0])
        if plan.key is None or not hasattr(plan.key, "dim"):
            raise ValueError("plan.key must be a tensor on the handle's GPU (PreparePlan.to_device)")
        want(plan.key, "plan.key", torch.int32, (B, N) if plan.key.dim() == 2 else (plan.key.shape[0], B, N))
        if plan.key.dim() == 3 and not 0 <= (0 if key_row is None else int(key_row)) < plan.key.shape[0]:
            raise ValueError("key_row is outside plan.key")
        want(plan.cre, "plan.cre", torch.float64, (M, N))
        want(plan.cim, "plan.cim", torch.float64, (M, N))
        want(plan.limits, "plan.limits", torch.float64, (M,))
        want(plan.min_pilot, "plan.min_pilot", torch.float64, (N,))
        want(cur.lb, "cur.lb", torch.float64, (B, N, Tm))
        want(cur.ub, "cur.ub", torch.float64, (B, N, Tm))
        want(cur.s_off, "cur.s_off", torch.int32, (B, cur.K, N))
        want(cur.s_len, "cur.s_len", torch.int32, (B, cur.K, N))
        want(cur.s_cap, "cur.s_cap", torch.float64, (B, cur.K, N))
        want(flags, "flags", torch.int32, (B,))
        if flags is None:
            raise ValueError("flags is required")
        want(v_evse, "v_evse", torch.int32, (B, N))
        want(v_arrived, "v_arrived", torch.uint8, (B, N))
        want(v_cap, "v_cap", torch.float64, (B, N))
        p = _Problems(B, Tm, cur.K, None, None, None, None, None, _dptr(cur.s_off), _dptr(cur.s_len), _dptr(cur.s_cap), None, None, None, None,
                      None, None, None)
        pl = plan._struct(N, key_row, min_rates)
        v = _PrepareView(_dptr(v_evse), _dptr(v_arrived), _dptr(v_cap))
        _check(self._lib.acnqp_prepare_device(self._h, C.byref(p), C.byref(pl), _dptr(cur.lb), _dptr(cur.ub), C.byref(v), _dptr(flags),
                                              C.c_void_p(stream)), "acnqp_prepare_device")

    def _kernel_ms_of_call(self) -> float:
        """Sum of the HIP-event durations of the launches since the previous ``kernel_times`` call; NaN when an event
        could not be read or when the call made more launches than the library's 64-entry event ring holds (the sum
        would silently under-report)."""
        before = int(self._lib.acnqp_launch_count(self._h))
        ms = self.kernel_times()
        if any(m < 0 for m in ms) or before - self._launches_seen > len(ms):
            self._launches_seen = before
            return float("nan")
        self._launches_seen = before
        return float(sum(ms))

    def polish_stats(self) -> dict:
        """Counters of the device-side polish over this handle's life (acnqp_polish_stats; synchronises)."""
        buf = (C.c_int64 * 16)()
        _check(self._lib.acnqp_polish_stats(self._h, buf, 16), "acnqp_polish_stats")
        out = dict(zip(("attempted", "solved", "gave_up_rows", "gave_up_pivot", "gave_up_rounds", "gave_up_kkt", "rounds"), [int(v) for v in buf[:7]]))
        out["phase_us"] = [int(v) // 100 for v in buf[8:16]]   # summed over the polish workgroups
        return out

    def polish_alongside(self) -> int:
        """Problems that polish launches running ALONGSIDE a solver launch have taken since the previous call
        (acnqp_debug_polish_alongside: introspection, not part of the ABI; synchronises)."""
        fn = self._lib.acnqp_debug_polish_alongside
        fn.restype, fn.argtypes = C.c_int64, [C.c_void_p]
        n = int(fn(self._h))
        if n < 0:
            raise RuntimeError("acnqp_debug_polish_alongside failed")
        return n

    def wave_rank(self) -> dict:
        """The site's live eigenpairs, the MFMA k-steps that hold them once compacted, and the eigen extent (k-steps) of
        the wave kernel's instantiation this handle runs (acnqp_debug_wave_rank: introspection, not part of the ABI)."""
        buf = (C.c_int32 * 3)()
        fn = self._lib.acnqp_debug_wave_rank
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]
        if fn(self._h, buf) != 0:
            raise RuntimeError("acnqp_debug_wave_rank failed")
        return dict(rank=int(buf[0]), eig_ksteps=int(buf[1]), extent=int(buf[2]))

    def wave_evse_extent(self) -> dict:
        """The site's EVSEs, the MFMA k-steps of P = Ghat r0 that hold one, and the EVSE k-steps the wave kernel's
        instantiation this handle runs sums over (acnqp_debug_wave_evse_extent: introspection, not part of the ABI)."""
        buf = (C.c_int32 * 3)()
        fn = self._lib.acnqp_debug_wave_evse_extent
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]
        if fn(self._h, buf) != 0:
            raise RuntimeError("acnqp_debug_wave_evse_extent failed")
        return dict(n_evse=int(buf[0]), evse_ksteps=int(buf[1]), extent=int(buf[2]))

    def ordered_launches(self) -> int:
        """Launches of this handle whose queue order was sorted by session count (acnqp_ordered_launch_count)."""
        return int(self._lib.acnqp_ordered_launch_count(self._h))

    def last_kernel_ms(self) -> float:
        return float(self._lib.acnqp_last_kernel_ms(self._h))

    def kernel_times(self, capacity: int = 64):
        """Durations (ms) of the launches since the previous call (at most the 64 most recent); blocks
        until they have finished."""
        buf = (C.c_float * int(capacity))()
        n = int(self._lib.acnqp_kernel_times(self._h, buf, int(capacity)))
        return [float(buf[k]) for k in range(n)]

    def route(self, t_max: int, k_sessions: int, batch: int = 1):
        """(family, polish): the kernel family (ROUTE_NAMES) a launch of ``batch`` problems of this padded shape runs,
        and whether it runs the polish phase under default options (acnqp_route; no device work)."""
        pol = C.c_int32(0)
        fam = int(self._lib.acnqp_route(self._h, int(t_max), int(k_sessions), int(batch), C.byref(pol)))
        if fam == 0:
            raise ValueError(f"acnqp_route: no route for t_max={t_max}, k_sessions={k_sessions}, batch={batch}")
        return ROUTE_NAMES[fam], bool(pol.value)

    def accel_columns(self, t_max: int, k_sessions: int, options: Options) -> int:
        """Anderson columns the kernels use for this problem shape under ``options`` (shape-only rule)."""
        return int(self._lib.acnqp_accel_columns(self._h, int(t_max), int(k_sessions), int(options.precision),
                                                 int(options.accel_mem)))


class DeviceBatch:
    """A ProblemBatch resident in HBM (torch tensors on one GPU) plus result
    tensors; torch is used for device memory only."""

    def __init__(self, batch: ProblemBatch, device, want_y: bool = False):
        import torch

        dev = torch.device(device)
        self.B, self.N, self.Tm, self.K = batch.B, batch.N, batch.Tm, batch.K
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev)
        self.horizon = t(batch.T, np.int32)
        self.lb = t(batch.lb, np.float64)
        self.ub = t(batch.ub, np.float64)
        self.q = t(batch.q, np.float64)
        self.pdiag = t(batch.pdiag, np.float64)
        self.s_off = t(batch.s_off, np.int32)
        self.s_len = t(batch.s_len, np.int32)
        self.s_cap = t(batch.s_cap, np.float64)
        self.s_eq = t(batch.s_eq, np.uint8)
        self.peak = None if batch.peak is None else t(batch.peak, np.float64)
        self.lf = t(batch.lf, np.float64)
        self.dc = t(batch.dc if batch.dc is not None else np.zeros(batch.B), np.float64)
        self.dfloor = t(batch.dfloor if batch.dfloor is not None else np.zeros(batch.B), np.float64)
        self.x = torch.zeros((self.B, self.N, self.Tm), dtype=torch.float64, device=dev)
        self.status = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.iters = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.pri_res = torch.zeros(self.B, dtype=torch.float64, device=dev)
        self.dua_res = torch.zeros(self.B, dtype=torch.float64, device=dev)
        self.obj = torch.zeros(self.B, dtype=torch.float64, device=dev)
        # site-row multipliers (B, Mg, Tm) when wanted (acnqp_results.y), else None
        self.y = torch.zeros((self.B, batch.site.Mg, self.Tm), dtype=torch.float64, device=dev) if want_y else None

    @classmethod
    def empty(cls, site: SiteData, B: int, Tm: int, K: int, device, want_y: bool = False, s_eq: int = 0, dfloor: float = 0.0,
              with_peak: Optional[bool] = None) -> "DeviceBatch":
        """An empty state of shape (B, N, Tm, K) in HBM: no session in any slot, zero bounds and cost, horizon 1, no peak limit.
        What ``SiteHandle.advance_device`` writes into, and -- with ``step = -1`` -- what a rollout starts from."""
        import torch

        dev = torch.device(device)
        self = cls.__new__(cls)
        self.B, self.N, self.Tm, self.K = int(B), site.N, int(Tm), int(K)
        z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
        self.horizon = torch.ones(self.B, dtype=torch.int32, device=dev)
        self.lb, self.ub, self.q = z((self.B, self.N, self.Tm)), z((self.B, self.N, self.Tm)), z((self.B, self.N, self.Tm))
        self.pdiag, self.lf, self.dc = z(self.B), z(self.B), z(self.B)
        self.dfloor = torch.full((self.B,), float(dfloor), dtype=torch.float64, device=dev)
        self.s_off, self.s_len = z((self.B, self.K, self.N), torch.int32), z((self.B, self.K, self.N), torch.int32)
        self.s_cap = z((self.B, self.K, self.N))
        self.s_eq = torch.full((self.B,), int(s_eq), dtype=torch.uint8, device=dev)
        self.peak = torch.full((self.B, self.Tm), float("inf"), dtype=torch.float64, device=dev) if (site.has_peak if with_peak is None else with_peak) else None
        self.x = z((self.B, self.N, self.Tm))
        self.status, self.iters = z(self.B, torch.int32), z(self.B, torch.int32)
        self.pri_res, self.dua_res, self.obj = z(self.B), z(self.B), z(self.B)
        self.y = z((self.B, site.Mg, self.Tm)) if want_y else None
        return self
