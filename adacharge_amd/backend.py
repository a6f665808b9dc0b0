"""ctypes binding of the C ABI in include/acn_qp.h (libacn_qp_hip.so).

There is exactly one compute path: the HIP library.  If it is missing or no GPU
is visible, everything here raises -- there is no CPU fallback by design
(the CPU implementations under oracle/ are test infrastructure and are never
imported from this package).

Each fact of the ABI is stated once: the arrays of a struct and their dtypes in one ``_*_ARRAYS``
map, from which the ctypes mirror, the marshallers and the plan classes are made; the entry points in ``_ABI``;
tests/test_abi.py holds every struct and constant to the header.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
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
PILOTS_CONTINUOUS, PILOTS_DISCRETE, PILOTS_REALLOCATE = 0, 1, 2
ADVANCE_REFUSED, ADVANCE_NO_ROW, ADVANCE_BAD_SLOT = 1, 2, 4
PREPARE_FUTURE = 1
PLANT_BAD_PLUG, PLANT_BAD_BATTERY = 1, 2
ESTIMATE_BAD_FRESH, ESTIMATE_BAD_SLOT = 1, 2
# kernel families of acnqp_route (ACNQP_ROUTE_* in include/acn_qp.h)
ROUTE_NAMES = {1: "wave1", 2: "wave2", 3: "wave3", 4: "wave4", 5: "wave5", 6: "tiled_ct1", 7: "tiled_ct2",
               8: "long_lds", 9: "long_ws", 10: "stream", 11: "general"}


class BackendUnavailable(RuntimeError):
    """The HIP library could not be loaded or no MI355X is visible."""


# ---- the structs of include/acn_qp.h -----------------------------------------------------------------------------------
# A struct's arrays, in the header's order, with the dtype the library reads or writes: the ctypes mirror, the host
# marshallers, DeviceBatch and the plan classes below are all made from these maps.
_I4, _F8, _U1 = np.int32, np.float64, np.uint8
_PROBLEM_ARRAYS = dict(horizon=_I4, lb=_F8, ub=_F8, q=_F8, pdiag=_F8, s_off=_I4, s_len=_I4, s_cap=_F8, s_eq=_U1, peak=_F8, lf=_F8,
                       dc=_F8, dfloor=_F8)
_NEXT_ARRAYS = tuple(k for k in _PROBLEM_ARRAYS if k != "s_eq")   # acnqp_next: the same, writable; s_eq does not change with time
_WARM = ("warm_x", "warm_y")
_TABLE_ARRAYS = dict(horizon=_I4, q_index=_I4, q_table=_F8, pdiag=_F8, s_eq=_U1, peak=_F8, lf=_F8, dc=_F8, dfloor=_F8, sess_seg=_I4,
                     s_evse=_I4, s_slot=_I4, s_off=_I4, s_len=_I4, s_cap=_F8, rate_seg=_I4, min_rates=_F8, max_rates=_F8)
_RESULT_ARRAYS = dict(x=_F8, status=_I4, iters=_I4, pri_res=_F8, dua_res=_F8, obj=_F8)   # then y and x_dev, both optional
_PILOT_ARRAYS = dict(cre=_F8, cim=_F8, limits=_F8, max_pilot=_F8, levels=_F8, sess_seg=_I4, s_evse=_I4, s_arrived=_U1, s_cap=_F8)
_ADVANCE_ARRAYS = dict(q_table=_F8, h_scal=_F8, h_row=_I4, peak_series=_F8, a_seg=_I4, a_evse=_I4, a_slot=_I4, a_len=_I4, a_cap=_F8,
                       a_rate_seg=_I4, a_min=_F8, a_max=_F8)
_COST_ARRAYS = dict(c_weight=_F8, c_series=_F8)   # weight and series of acnqp_clock_cost, under AdvancePlan's names
_PREPARE_ARRAYS = dict(key=_I4, cre=_F8, cim=_F8, limits=_F8, min_pilot=_F8)
_PLANT_ARRAYS = dict(t_room=_F8, t_amps=_F8, t_knee=_F8, t_slope=_F8, plug=_I4)   # the plant entries take them as plain arguments
_RESOLVE_ARRAYS = dict(sel_seg=_I4, sel_idx=_I4, pos=_I4)   # idx of the select entries and pos of the hold entries, for every step of a run
SELECT_BAD_INDEX = 1
HOLD_BAD_ROW = 1


def _ints(*names):
    return [(k, C.c_int32) for k in names]


def _doubles(*names):
    return [(k, C.c_double) for k in names]


def _ptrs(*names):
    return [(k, C.c_void_p) for k in names]


class _Site(C.Structure):
    _fields_ = _ints("n_evse", "n_infra", "n_rows", "cone", "has_peak", "has_flat", "has_max") + _ptrs("G", "limits")


class _Problems(C.Structure):
    """Mirror of ``acnqp_problems``: ``_Problems(B, Tm, K, s_off=..., s_len=...)`` leaves every array not named NULL."""

    _fields_ = _ints("batch", "t_max", "k_sessions") + _ptrs(*_PROBLEM_ARRAYS, *_WARM)


class _Table(C.Structure):
    _fields_ = _ints("batch", "t_max", "k_sessions", "n_sessions", "n_horizons") + _ptrs(*_TABLE_ARRAYS)


class _Results(C.Structure):
    _fields_ = _ptrs(*_RESULT_ARRAYS, "y", "x_dev")


class _Duals(C.Structure):
    _fields_ = _ptrs("mu", "z", "res")


class _PilotPlan(C.Structure):
    _fields_ = _ints("batch", "t_max", "n_evse", "n_infra", "n_levels", "n_sessions", "mode") + _ptrs(*_PILOT_ARRAYS)


class _Pilots(C.Structure):
    _fields_ = _ptrs("pilots", "first", "visits")


class _AdvancePlan(C.Structure):
    _fields_ = (_ints("n_evse", "n_rows", "n_horizons", "step", "peak_len", "n_arrivals", "n_rates")
                + _doubles("done_tol", "kw_per_amp", "warm_arrival_gain") + _ptrs(*_ADVANCE_ARRAYS))


class ClockCost(C.Structure):
    """Mirror of ``acnqp_clock_cost``: the clock cost of the advance's rule 6b."""

    _fields_ = _ints("n_evse", "series_len") + _doubles("coef") + _ptrs("weight", "series")


class _Next(C.Structure):
    _fields_ = _ptrs(*_NEXT_ARRAYS, *_WARM)


class _PreparePlan(C.Structure):
    _fields_ = _ints("n_evse", "n_infra") + _ptrs(*_PREPARE_ARRAYS)


class _PrepareView(C.Structure):
    _fields_ = _ptrs("v_evse", "v_arrived", "v_cap")


class Options(C.Structure):
    """Mirror of ``acnqp_options``; construct with ``default_options()``."""

    _fields_ = (_doubles("eps_abs", "eps_rel") + _ints("max_iter", "check_every", "adapt_every")
                + _doubles("rho", "sigma", "alpha", "adapt_tol", "reg_rel")
                + _ints("precision", "accel_mem", "stall_iters", "retry_passes", "retry_max_iter", "polish_iters")
                + _doubles("retry_rho", "inaccurate_floor") + _ints("polish_stall"))


# ---- the entry points --------------------------------------------------------------------------------------------------
def _abi():
    """(name, restype, argtypes, declared): the prototype of every entry the binding calls.  ``declared``: the header
    declares it, so every build exports it; the others are introspection that a build may lack."""
    P, ptr, i32, i64, rc = C.POINTER, C.c_void_p, C.c_int32, C.c_int64, C.c_int
    h = stream = ptr
    solve = [h, P(_Problems), P(Options), P(_Results)]
    advance = [h, P(_Problems), ptr, ptr, ptr, ptr, P(_AdvancePlan)]   # cur, applied, status, x, y, plan
    rows = [
        ("acnqp_create", rc, [P(_Site), i32, P(ptr)]),
        ("acnqp_destroy", None, [h]),
        ("acnqp_solve_batch", rc, solve),
        ("acnqp_solve_batch_device", rc, solve + [stream]),
        ("acnqp_solve_batches", rc, [h, i32, P(_Problems), P(Options), P(_Results)]),
        ("acnqp_solve_table", rc, [h, P(_Table), P(Options), P(_Results)]),
        ("acnqp_host_alloc", ptr, [C.c_size_t]),
        ("acnqp_host_free", None, [ptr]),
        ("acnqp_default_options", None, [P(Options)]),
        ("acnqp_last_error", C.c_char_p, []),
        ("acnqp_abi_version", i32, []),
        ("acnqp_last_kernel_ms", C.c_float, [h]),
        ("acnqp_kernel_times", i32, [h, P(C.c_float), i32]),
        ("acnqp_launch_count", i64, [h]),
        ("acnqp_ordered_launch_count", i64, [h]),
        ("acnqp_polish_stats", rc, [h, P(i64), i32]),
        ("acnqp_accel_columns", i32, [h, i32, i32, i32, i32]),
        ("acnqp_route", i32, [h, i32, i32, i32, P(i32)]),
        ("acnqp_set_long_polish", rc, [h, i32]),
        ("acnqp_set_wide_polish", rc, [h, i32]),
        ("acnqp_set_long_vjp", rc, [h, i32]),
    ]
    # acnqp_X_host takes these arguments, acnqp_X_device the same and the stream behind them
    for stem, args in (
        ("acnqp_duals", [h, P(_Problems), P(Options), ptr, ptr, ptr, P(_Duals)]),
        ("acnqp_pilots", [h, P(_PilotPlan), ptr, P(_Pilots)]),
        ("acnqp_advance", advance + [P(_Next), ptr]),
        ("acnqp_advance_priced", advance + [P(ClockCost), P(_Next), ptr]),
        ("acnqp_prepare", [h, P(_Problems), P(_PreparePlan), ptr, ptr, P(_PrepareView), ptr]),
        # cur, pilots, status, n_batteries, t_room, t_amps, t_knee, t_slope, plug, bat, room, actual, flags
        ("acnqp_plant", [h, P(_Problems), ptr, ptr, i32] + [ptr] * 9),
        # cur, fresh, pilots, actual, status, up_threshold, down_threshold, up_increment, est, ub_out, flags
        ("acnqp_estimate", [h, P(_Problems)] + [ptr] * 4 + [C.c_double] * 3 + [ptr] * 3),
        # cur, n_evse, n_rows, m, idx, out, s_eq, flags
        ("acnqp_select", [h, P(_Problems), i32, i32, i32, ptr, P(_Next), ptr, ptr]),
        # cur, n_evse, n_rows, m, pos, dense, held_x, held_y, prev_status, out, solved, flags
        ("acnqp_hold", [h, P(_Problems), i32, i32, i32, ptr, P(_Results), ptr, ptr, ptr, P(_Results), ptr, ptr]),
        # problems, options, x, y, status, gx, gq, gcap, grow, glb, gub, info, res
        ("acnqp_vjp", [h, P(_Problems), P(Options)] + [ptr] * 11),
        # cur, applied, status, x, plan, cost, max_pilot, gdir, gq_next, gcap_vjp_next, gcap_carry_next, horizon_next, flags_next,
        # gx, gcap_carry, garr, gprice
        ("acnqp_advance_vjp", [h, P(_Problems), ptr, ptr, ptr, P(_AdvancePlan), P(ClockCost)] + [ptr] * 11),
    ):
        rows += [(stem + "_host", rc, args), (stem + "_device", rc, args + [stream])]
    introspection = [
        ("acnqp_debug_polish_alongside", i64, [h]),
        ("acnqp_debug_direct_x", i64, [h]),
        ("acnqp_debug_direct_in", i64, [h]),
        ("acnqp_debug_wave_rank", rc, [h, P(i32)]),
        ("acnqp_debug_wave_evse_extent", rc, [h, P(i32)]),
        ("acnqp_debug_order_keys", rc, [h, P(_Problems), P(i32)]),
        ("acnqp_debug_copy_workspace", i64, [h, ptr, i64]),   # builds with -DACNQP_DEBUG_WS only (tools/gpu_long_race.py)
    ]
    return tuple(r + (True,) for r in rows) + tuple(r + (False,) for r in introspection)


_ABI = _abi()
# every symbol include/acn_qp.h declares; tests check the library exports all of them
EXPORTED_SYMBOLS = tuple(name for name, _, _, declared in _ABI if declared)

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
    for name, restype, argtypes, declared in _ABI:
        if declared or hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
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


# ---- arrays and tensors to pointers ------------------------------------------------------------------------------------
def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _addr(a: Optional[np.ndarray]):
    """the address of an array as an int (None stays None), for a struct field whose array the caller keeps alive: half the
    cost of ``_ptr``, whose c_void_p also holds on to the array"""
    return None if a is None else a.ctypes.data


def _dptr(t):
    """the device address of a torch tensor (None stays None)"""
    return None if t is None else C.c_void_p(t.data_ptr())


def _f8(a):
    return None if a is None else np.ascontiguousarray(a, np.float64)


def _i4(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


def _torch_dtype(dtype):
    import torch

    return getattr(torch, np.dtype(dtype).name)


def _want(t, name: str, dtype, shape=None, device=None) -> None:
    """The one check of a tensor argument; None passes.  With ``device``: a contiguous torch tensor of ``dtype`` there (and
    of ``shape``, when one is given).  Without: contiguity, shape and the ITEM SIZE of ``dtype`` only, on any device -- all
    the entries older than ``pilots_device`` ever asked, kept so that they refuse nothing they took."""
    if t is None:
        return
    if device is None:
        ok = t.element_size() == np.dtype(dtype).itemsize
    else:
        import torch

        ok = isinstance(t, torch.Tensor) and t.device == device and t.dtype == _torch_dtype(dtype)
    if not ok or not t.is_contiguous() or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{name} must be a contiguous torch.{np.dtype(dtype).name} tensor" + ("" if device is None else f" on {device}")
                         + ("" if shape is None else f" of shape {tuple(shape)}"))


def _absent(site: SiteData, peak: bool = False) -> tuple:
    """the optional arrays that are NULL for this site: those of a row it does not have (``peak``: the peak row's too)"""
    return (() if site.has_flat else ("lf",)) + (() if site.has_max else ("dc", "dfloor")) + (("peak",) if peak and not site.has_peak else ())


def _host_arrays(src, arrays: dict, absent) -> dict:
    """{name: array or None} of a struct's ``arrays`` from the attributes of ``src`` (a ProblemBatch or TablePlan, which call the
    horizons T): C-contiguous with the ABI's dtype -- the attribute itself when it already is (e.g. pinned arrays from
    ``pinned_empty``), else a copy; None for a name in ``absent`` and for an attribute that is None."""
    return {k: None if k in absent or (a := getattr(src, "T" if k == "horizon" else k)) is None else np.ascontiguousarray(a, dt)
            for k, dt in arrays.items()}


def _new_results(B: int, N: int, Tm: int, Mg: int, pinned: bool, want_y: bool, x_dev=None, out: Optional["BatchResult"] = None):
    """(BatchResult, _Results pointing into it): ``out`` when its arrays have the shapes asked for, else new arrays (pinned
    or not).  ``x_dev``: the device address for acnqp_results.x_dev, or None."""
    if out is not None and out.x.shape == (B, N, Tm) and (not want_y or (out.y is not None and out.y.shape == (B, Mg, Tm))):
        res = out
    else:
        new = pinned_empty if pinned else np.zeros
        res = BatchResult(*[new((B, N, Tm) if k == "x" else B, dt) for k, dt in _RESULT_ARRAYS.items()])
        if want_y:
            res.y = new((B, Mg, Tm))
    r = _Results(*[_addr(getattr(res, k)) for k in _RESULT_ARRAYS], _addr(res.y) if want_y else None,
                 None if x_dev is None else C.c_void_p(int(x_dev)))
    return res, r


def _marshal_batch(site: SiteData, batch: ProblemBatch, pinned: bool, x_dev=None, warm=None, want_y=False):
    """ctypes views of one batch of host arrays for ``site``: (_Problems, _Results, BatchResult, keep-alive).  lf, dc and
    dfloor are NULL where the site has no such row: that skips a copy in the library."""
    B, N, Tm = batch.B, batch.N, batch.Tm
    arrs = _host_arrays(batch, _PROBLEM_ARRAYS, _absent(site))
    wx = wy = None
    if warm is not None:
        wx, wy = _f8(warm[0]), _f8(warm[1])
        if wx.shape != (B, N, Tm) or wy.shape != (B, site.Mg, Tm):
            raise ValueError(f"warm start arrays must have shapes {(B, N, Tm)} and {(B, site.Mg, Tm)}")
    p = _Problems(B, Tm, batch.K, *[_addr(a) for a in arrs.values()], _addr(wx), _addr(wy))
    res, r = _new_results(B, N, Tm, site.Mg, pinned, want_y, x_dev)
    return p, r, res, (arrs, wx, wy)


def _device_problems(dev: "DeviceBatch", warm_x=None, warm_y=None) -> _Problems:
    """The ``acnqp_problems`` of a ``DeviceBatch``: the address of every tensor it holds, NULL for a peak it does not have
    and for a warm start that is not given.  lf, dc and dfloor are always passed, because a ``DeviceBatch`` always holds
    them, also for a site without a flat or max row: the library reads them only under has_flat / has_max (``tiled_args``
    in acn_qp_api.hip, ``check_problem_shapes`` and the duals entry in acn_qp_post.hpp) and refuses a NULL only where the row
    exists, so the extra addresses are never looked at."""
    return _Problems(dev.B, dev.Tm, dev.K, *[_dptr(getattr(dev, k)) for k in _PROBLEM_ARRAYS], _dptr(warm_x), _dptr(warm_y))


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
class VjpResult:
    """The gradients through the solve of a batch of answers (acnqp_vjp_host / acnqp_vjp_device, include/acn_qp.h), for a
    scalar L of the schedules with dL/dx given, in the units of the C ABI (minimisation form, energy rows in A-periods)."""
    q: np.ndarray                # (B, N, Tm) dL/dq; exact 0 on fixed variables and dead periods
    cap: np.ndarray              # (B, K, N) dL/d(s_cap): layout of s_cap; 0 for a slack row or an empty slot
    rows: np.ndarray             # (B, M + has_peak, Tm) dL/d(limit of a site row at a period); row M: the peak's periods
    lb: Optional[np.ndarray]     # (B, N, Tm) dL/dlb, non-zero where the variable sits on lb (None: not asked for)
    ub: Optional[np.ndarray]     # (B, N, Tm) dL/dub
    info: np.ndarray             # (B, 4) int32: verdict (0 done), rows of the Schur system, weak members, free variables
    res: np.ndarray              # (B, 2): residual of the adjoint solve; the primal point's stationarity on free variables


class _PlanArrays:
    """What the plan classes share.  ``_DTYPES``: {array field: the dtype the ABI reads}."""

    _DTYPES = {}

    def to_device(self, device):
        """the same plan with every array a torch tensor of the ABI's dtype on ``device``"""
        import torch

        moved = {k: None if getattr(self, k) is None else torch.from_numpy(np.ascontiguousarray(getattr(self, k), dt)).to(device)
                 for k, dt in self._DTYPES.items()}
        return dataclasses.replace(self, **moved)

    def _p(self, k: str, keep=None, row: int = 0, stacked: Optional[int] = None):
        """The pointer of field ``k`` for the struct: NULL when it is None or empty; a tensor's ``data_ptr()``; for an
        array, the address of a C-contiguous array of the field's dtype -- the array itself when it is one, else a copy --
        which is appended to ``keep`` so that it outlives the call.  A field with ``stacked`` dimensions holds one block per
        step: ``row`` picks the step's."""
        a = getattr(self, k)
        if a is None or (a.numel() if hasattr(a, "numel") else a.size) == 0:
            return None
        if a.ndim == stacked:
            a = a[row]
        if hasattr(a, "data_ptr"):
            return C.c_void_p(a.data_ptr())
        a = np.ascontiguousarray(a, self._DTYPES[k])
        if keep is not None:
            keep.append(a)
        return _ptr(a)

    def _len(self, k: str, axis: int = 0) -> int:
        return 0 if getattr(self, k) is None else int(getattr(self, k).shape[axis])


@dataclass
class PilotPlan(_PlanArrays):
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

    _DTYPES = _PILOT_ARRAYS
    _ARRAYS = tuple(_PILOT_ARRAYS)

    def _struct(self, batch=None, t_max=None, keep=None) -> "_PilotPlan":
        return _PilotPlan(int(self.B if batch is None else batch), int(self.Tm if t_max is None else t_max), self.N, self._len("cre"),
                          self._len("levels", 1), self._len("s_evse"), self.mode, *[self._p(k, keep) for k in _PILOT_ARRAYS])


@dataclass
class AdvancePlan(_PlanArrays):
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

    _DTYPES = {**_ADVANCE_ARRAYS, **_COST_ARRAYS}
    _ARRAYS = tuple(_ADVANCE_ARRAYS)

    def _struct(self, N: int, Mg: int, step: int, seg_row: int = 0, keep=None) -> "_AdvancePlan":
        A = self._len("a_evse")
        ptrs = [self._p(k, keep, seg_row, 2 if k == "a_seg" else None) for k in _ADVANCE_ARRAYS]
        if not A:   # a_seg is NULL iff there is no arrival
            ptrs[self._ARRAYS.index("a_seg")] = None
        return _AdvancePlan(int(N), int(Mg), int(self.q_table.shape[0]), int(step), self._len("peak_series", 1), A, self._len("a_min"),
                            float(self.done_tol), float(self.kw_per_amp), float(self.warm_arrival_gain), *ptrs)

    def _cost_struct(self, N: int, keep=None) -> Optional["ClockCost"]:
        """the ``acnqp_clock_cost`` of the plan, or None (the plain advance) when no c_ field is set"""
        given = [self.c_coef is not None, self.c_weight is not None, self.c_series is not None]
        if not any(given):
            return None
        if not all(given):
            raise ValueError("a clock cost needs c_coef, c_weight and c_series")
        if self.c_series.ndim != 2:
            raise ValueError("c_series must have shape (B, P)")
        for k, dt in _COST_ARRAYS.items():
            if hasattr(getattr(self, k), "data_ptr"):
                _want(getattr(self, k), k, dt)
        return ClockCost(int(N), int(self.c_series.shape[1]), float(self.c_coef), *[self._p(k, keep) for k in _COST_ARRAYS])


@dataclass
class PreparePlan(_PlanArrays):
    """The arrays of ``acnqp_prepare_plan`` (include/acn_qp.h): numpy arrays for ``SiteHandle.prepare_host``, torch tensors on the
    handle's GPU (``to_device``) for ``SiteHandle.prepare_device``.  ``key`` may hold one (B, N) block per step
    (``(steps, B, N)``): ``key_row`` picks the step's.  ``min_pilot=None``: no minimum-rate step."""
    key: object                          # (B, N) or (rows, B, N) int32: list position of the session on each EVSE
    cre: Optional[object] = None         # (M, N) the site in the SOC form of ``PilotPlan``
    cim: Optional[object] = None
    limits: Optional[object] = None      # (M,)
    min_pilot: Optional[object] = None   # (N,)

    _DTYPES = _PREPARE_ARRAYS
    _ARRAYS = tuple(_PREPARE_ARRAYS)

    def _struct(self, N: int, key_row=None, min_rates: bool = True, keep=None) -> "_PreparePlan":
        return _PreparePlan(int(N), self._len("cre"), self._p("key", keep, 0 if key_row is None else key_row, 3), self._p("cre", keep),
                            self._p("cim", keep), self._p("limits", keep), self._p("min_pilot", keep) if min_rates else None)


@dataclass
class PlantPlan(_PlanArrays):
    """The battery table and the plug-in rows of ``acnqp_plant_device / _host`` (include/acn_qp.h, "the plant"): numpy arrays
    for ``SiteHandle.plant_host``, torch tensors on the handle's GPU (``to_device``) for ``SiteHandle.plant_device``.  ``plug``
    may hold one (B, N) block per step (``(steps, B, N)``): ``plug_row`` picks the step's.  ``rollout.FleetTable`` builds one."""
    t_room: object    # (R,) room left at plug-in, A-periods
    t_amps: object    # (R,) the battery's current limit, A
    t_knee: object    # (R,) room at which the tail begins; 0: no tail
    t_slope: object   # (R,) t_amps / t_knee where t_knee > 0, else 0
    plug: object      # (B, N) or (rows, B, N) int32: the row plugged in at the step, -1 elsewhere

    _DTYPES = _PLANT_ARRAYS
    _ARRAYS = tuple(_PLANT_ARRAYS)

    def _args(self, plug_row=None, keep=None) -> list:
        """n_batteries and the five pointers, in the order of the entries' arguments"""
        return [C.c_int32(self._len("t_room"))] + [self._p(k, keep, 0 if plug_row is None else plug_row, 3 if k == "plug" else None)
                                                   for k in _PLANT_ARRAYS]


@dataclass
class ResolvePlan(_PlanArrays):
    """Which scenarios of a closed loop are solved afresh at which step (``rollout.FleetTable.resolve_plan``), as
    ``SiteHandle.select_device`` and ``SiteHandle.hold_device`` read it: numpy arrays, or torch tensors on the handle's GPU
    (``to_device``).  Step s resolves the ``m_s = sel_seg[s + 1] - sel_seg[s]`` scenarios ``sel_idx[sel_seg[s]: sel_seg[s + 1]]``,
    ascending; ``pos[s, b]`` is the row of scenario b in the step's dense batch, or -1 where b keeps the schedule it holds."""
    sel_seg: object   # (steps + 1,) int32
    sel_idx: object   # (sum of m_s,) int32
    pos: object       # (steps, B) int32

    _DTYPES = _RESOLVE_ARRAYS
    _ARRAYS = tuple(_RESOLVE_ARRAYS)

    def counts(self) -> list:
        """m_s of every step, as Python ints (read from the host copy or, once, from the device)"""
        seg = self.sel_seg.cpu().numpy() if hasattr(self.sel_seg, "cpu") else np.asarray(self.sel_seg)
        return [int(v) for v in np.diff(seg)]


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

    def __init__(self, site: SiteData, device: int = 0, polish_long: bool = False, polish_wide: bool = False, vjp_long: bool = False):
        """``polish_long``: the Newton polish also takes over at horizons 33 ... 288 (N <= 64; ``acnqp_set_long_polish``).
        ``polish_wide``: on sites of 65 ... 1,024 EVSEs (horizons <= 48) the Newton polish runs behind the solver launch on
        what it ended MAX_ITER or SOLVED_INACCURATE (``acnqp_set_wide_polish``).
        Both off by default: launches then do exactly what they did before there was such a polish.
        ``vjp_long``: ``vjp`` / ``vjp_device`` also serve horizons 33 ... 288 (N <= 64, a site with rows; ``acnqp_set_long_vjp``).
        Off by default: longer horizons are then refused as before; at horizons <= 32 the switch changes nothing."""
        self._lib = load_library()
        self.site = site
        self.device = int(device)
        self.polish_long = bool(polish_long)
        self.polish_wide = bool(polish_wide)
        self.vjp_long = bool(vjp_long)
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
        if self.polish_long:
            _check(self._lib.acnqp_set_long_polish(self._h, 1), "acnqp_set_long_polish")
        if self.polish_wide:
            _check(self._lib.acnqp_set_wide_polish(self._h, 1), "acnqp_set_wide_polish")
        if self.vjp_long:
            _check(self._lib.acnqp_set_long_vjp(self._h, 1), "acnqp_set_long_vjp")

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
        """ctypes views of one batch: (_Problems, _Results, BatchResult, keep-alive) -- ``_marshal_batch`` for this site"""
        return _marshal_batch(self.site, batch, pinned, x_dev, warm, want_y)

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
        _want(x_dev, "x_dev", _F8, (B, N, Tm))
        keep = _host_arrays(plan, _TABLE_ARRAYS, _absent(self.site, peak=True))
        t = _Table(B, Tm, plan.K, plan.S, len(plan.q_table), *[_addr(a) for a in keep.values()])
        res, r = _new_results(B, N, Tm, self.site.Mg, pinned_results, want_y, None if x_dev is None else x_dev.data_ptr(), out)
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

    def prepare_many(self, batches, pinned_results=True, x_dev_ptrs=None, warm=None):
        """Marshal once, solve repeatedly (bench.py): returns a callable ``run(options)`` that re-submits the same
        host buffers through acnqp_solve_batches and the list of BatchResults it fills.  ``pinned_results``: one choice
        for all batches, or one per batch.  ``x_dev_ptrs[g]``: optional device address that also receives batch g's
        schedules (acnqp_results.x_dev).  ``warm[g]``: optional warm start of batch g, as ``solve`` takes it."""
        n = len(batches)
        warm = [None] * n if warm is None else list(warm)
        pinned = [bool(pinned_results)] * n if isinstance(pinned_results, (bool, np.bool_)) else [bool(v) for v in pinned_results]
        if len(pinned) != n or len(warm) != n:
            raise ValueError("pinned_results and warm need one entry per batch")
        P, R = (_Problems * n)(), (_Results * n)()
        results, keep = [], []
        for g, batch in enumerate(batches):
            self._check_site(batch)
            P[g], R[g], res, k = self._marshal(batch, pinned[g], None if x_dev_ptrs is None else x_dev_ptrs[g], warm=warm[g])
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
        _want(warm_x, "warm_x", _F8, (dev.B, dev.N, dev.Tm))
        _want(warm_y, "warm_y", _F8, (dev.B, self.site.Mg, dev.Tm))
        p = _device_problems(dev, warm_x, warm_y)
        r = _Results(*[_dptr(getattr(dev, k)) for k in _RESULT_ARRAYS], _dptr(dev.y), None)
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
        x, y, st = _f8(res.x), _f8(res.y), _i4(res.status)
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
        p = _device_problems(dev)
        d = _Duals(mu.data_ptr(), None if z is None else z.data_ptr(), res.data_ptr())
        _check(
            self._lib.acnqp_duals_device(self._h, C.byref(p), C.byref(o), _dptr(dev.x), _dptr(dev.y),
                                         _dptr(dev.status) if use_status else None, C.byref(d), C.c_void_p(stream)),
            "acnqp_duals_device",
        )

    # -- gradients through the solve (acn_qp_vjp.hpp) -----------------------------------------------------------------
    def vjp(self, batch: ProblemBatch, result: "BatchResult", grad_x, want_bounds: bool = True,
            options: Optional[Options] = None) -> VjpResult:
        """acnqp_vjp_host: for the answers ``result`` (a BatchResult with ``y``) to ``batch`` and ``grad_x`` (B, N, Tm) =
        dL/dx of a scalar L of the schedules, the gradients of L with respect to q, s_cap, the site rows' limits and -- with
        ``want_bounds`` -- lb and ub, by one adjoint solve per problem on the GPU.  ``options``: those of the solve
        (``reg_rel`` is read).  Served: N <= 64, horizons <= 32 (to 288 on a ``vjp_long=True`` handle whose site has a
        row), K <= 4, no load-flattening or demand-charge row; anything else raises ValueError with the reason."""
        self._check_site(batch)
        B, N, Tm, K = batch.B, batch.N, batch.Tm, batch.K
        if self.site.Mg > 0 and result.y is None:
            raise ValueError("gradients need the site-row multipliers: solve with want_y=True")
        o = options if options is not None else default_options()
        p, _, _, keep = self._marshal(batch, False)
        x, y, st, gx = _f8(result.x), _f8(result.y), _i4(result.status), _f8(grad_x)
        if x.shape != (B, N, Tm) or st.shape != (B,) or gx.shape != (B, N, Tm) or (y is not None and y.shape != (B, self.site.Mg, Tm)):
            raise ValueError("result arrays and grad_x do not match the batch")
        nrow = self.site.M + (1 if self.site.has_peak else 0)
        out = VjpResult(np.zeros((B, N, Tm)), np.zeros((B, K, N)), np.zeros((B, nrow, Tm)), np.zeros((B, N, Tm)) if want_bounds else None,
                        np.zeros((B, N, Tm)) if want_bounds else None, np.zeros((B, 4), np.int32), np.zeros((B, 2)))
        _check(self._lib.acnqp_vjp_host(self._h, C.byref(p), C.byref(o), _ptr(x), _ptr(y), _ptr(st), _ptr(gx), _ptr(out.q), _ptr(out.cap),
                                        _ptr(out.rows) if nrow else None, _ptr(out.lb), _ptr(out.ub), _ptr(out.info), _ptr(out.res)),
               "acnqp_vjp_host")
        del keep
        return out

    def vjp_device(self, dev: "DeviceBatch", grad_x, gq, gcap, grow, info, res, glb=None, gub=None, options: Optional[Options] = None,
                   stream: int = 0, use_status: bool = True) -> None:
        """acnqp_vjp_device: the same for a ``DeviceBatch`` after ``solve_device`` (``want_y=True`` on a site with rows).
        ``grad_x``, ``gq`` (B, N, Tm), ``gcap`` (B, K, N), ``grow`` (B, M + has_peak, Tm), ``res`` (B, 2) and the optional
        ``glb``, ``gub`` (B, N, Tm) are float64 device tensors, ``info`` (B, 4) int32.  Asynchronous on ``stream``."""
        o = options if options is not None else default_options()
        if self.site.Mg > 0 and dev.y is None:
            raise ValueError("gradients need the site-row multipliers: DeviceBatch(..., want_y=True)")
        B, N, Tm, K = dev.B, dev.N, dev.Tm, dev.K
        nrow = self.site.M + (1 if self.site.has_peak else 0)
        d = dev.x.device
        for t, name, dt, shape in ((grad_x, "grad_x", _F8, (B, N, Tm)), (gq, "gq", _F8, (B, N, Tm)), (gcap, "gcap", _F8, (B, K, N)),
                                   (grow, "grow", _F8, (B, nrow, Tm)), (glb, "glb", _F8, (B, N, Tm)), (gub, "gub", _F8, (B, N, Tm)),
                                   (info, "info", _I4, (B, 4)), (res, "res", _F8, (B, 2))):
            _want(t, name, dt, shape, d)
        p = _device_problems(dev)
        _check(
            self._lib.acnqp_vjp_device(self._h, C.byref(p), C.byref(o), _dptr(dev.x), _dptr(dev.y), _dptr(dev.status) if use_status else None,
                                       _dptr(grad_x), _dptr(gq), _dptr(gcap), _dptr(grow) if nrow else None, _dptr(glb), _dptr(gub),
                                       _dptr(info), _dptr(res), C.c_void_p(stream)),
            "acnqp_vjp_device",
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
        keep = []
        p = plan._struct(B, Tm, keep)
        out = _Pilots(_ptr(pil), _ptr(first), _ptr(visits))
        _check(self._lib.acnqp_pilots_host(self._h, C.byref(p), _ptr(x), C.byref(out)), "acnqp_pilots_host")
        del keep
        return pil, first, visits

    def pilots_device(self, plan: PilotPlan, x, pilots=None, first=None, visits=None, stream: int = 0) -> None:
        """acnqp_pilots_device: the same on device memory -- ``plan`` from ``PilotPlan.to_device``, ``x`` (B, N, Tm) and the
        outputs ``pilots`` (B, N, Tm), ``first`` (B, N) (float64) and ``visits`` (B,) (int32) torch tensors on the handle's
        GPU; at least one of ``pilots`` / ``first``.  Asynchronous on ``stream``."""
        import torch

        here = torch.device("cuda", self.device)
        _want(x, "x", _F8, None, here)
        if x.dim() != 3 or x.shape[1] != plan.N:
            raise ValueError("x must have the shape (B, N, Tm) of the plan's site")
        B, N, Tm = x.shape
        M, L, S = plan._len("cre"), plan._len("levels", 1), plan._len("s_evse")
        shapes = dict(max_pilot=(N,), levels=(N, L), cre=(M, N), cim=(M, N), limits=(M,), sess_seg=(B + 1,), s_evse=(S,), s_arrived=(S,),
                      s_cap=(S,))
        for t, name, dt, shape in ((pilots, "pilots", _F8, (B, N, Tm)), (first, "first", _F8, (B, N)), (visits, "visits", _I4, (B,))):
            _want(t, name, dt, shape, here)
        for k, shape in shapes.items():
            _want(getattr(plan, k), "plan." + k, _PILOT_ARRAYS[k], shape, here)
        p = plan._struct(B, Tm)
        out = _Pilots(_dptr(pilots), _dptr(first), _dptr(visits))
        _check(self._lib.acnqp_pilots_device(self._h, C.byref(p), _dptr(x), C.byref(out), C.c_void_p(stream)), "acnqp_pilots_device")

    # -- time passes (acn_qp_advance.hpp) -------------------------------------------------------------------------------
    _NEXT = _NEXT_ARRAYS

    def advance(self, cur: dict, applied, plan: AdvancePlan, step: int, status=None, x=None, y=None, want_warm: bool = False,
                seg_row: int = 0) -> dict:
        """acnqp_advance_host: the next period's problems of the state ``cur`` -- a dict of numpy arrays ``lb, ub`` (B, N, Tm),
        ``s_off, s_len, s_cap`` (B, K, N) and, on a site with a max row, ``dfloor`` (B,) -- after the pilots ``applied`` (B, N)
        of period ``step``, under ``plan`` (numpy arrays).  Returns a dict of the same layout with ``horizon, q, pdiag, lf, dc,
        peak, flags`` added and, with ``want_warm``, ``warm_x`` / ``warm_y`` shifted from ``x`` (B, N, Tm) / ``y`` (B, Mg, Tm)."""
        lb, ub, off, ln, cap = _f8(cur["lb"]), _f8(cur["ub"]), _i4(cur["s_off"]), _i4(cur["s_len"]), _f8(cur["s_cap"])
        if lb.ndim != 3 or lb.shape[1] != self.site.N or ub.shape != lb.shape or off.ndim != 3 or off.shape != ln.shape or off.shape != cap.shape:
            raise ValueError("cur needs lb, ub of shape (B, N, Tm) and s_off, s_len, s_cap of shape (B, K, N) for the handle's site")
        B, N, Tm = lb.shape
        K, Mg = off.shape[1], self.site.Mg
        dfl = _f8(cur.get("dfloor")) if self.site.has_max else None
        app, stat, xs, ys = _f8(applied), _i4(status), _f8(x) if want_warm else None, _f8(y) if want_warm and Mg else None
        out = dict(horizon=np.empty(B, np.int32), lb=np.empty((B, N, Tm)), ub=np.empty((B, N, Tm)), q=np.empty((B, N, Tm)),
                   pdiag=np.empty(B), s_off=np.empty((B, K, N), np.int32), s_len=np.empty((B, K, N), np.int32), s_cap=np.empty((B, K, N)),
                   peak=np.empty((B, Tm)) if self.site.has_peak else None, lf=np.empty(B) if self.site.has_flat else None,
                   dc=np.empty(B) if self.site.has_max else None, dfloor=np.empty(B) if self.site.has_max else None,
                   warm_x=np.empty((B, N, Tm)) if xs is not None else None, warm_y=np.empty((B, Mg, Tm)) if ys is not None else None)
        flags = np.empty(B, np.int32)
        p = _Problems(B, Tm, K, lb=_ptr(lb), ub=_ptr(ub), s_off=_ptr(off), s_len=_ptr(ln), s_cap=_ptr(cap), dfloor=_ptr(dfl))
        keep = []
        pl = plan._struct(N, Mg, step, seg_row, keep)
        nx = _Next(*[_ptr(out[k]) for k in _NEXT_ARRAYS + _WARM])
        cost = plan._cost_struct(N, keep)
        if cost is not None and plan.c_series.shape[0] != B:
            raise ValueError(f"c_series has {plan.c_series.shape[0]} rows, the batch has {B} problems")
        head = (self._h, C.byref(p), _ptr(app), _ptr(stat), _ptr(xs), _ptr(ys), C.byref(pl))
        if cost is None:
            _check(self._lib.acnqp_advance_host(*head, C.byref(nx), _ptr(flags)), "acnqp_advance_host")
        else:
            _check(self._lib.acnqp_advance_priced_host(*head, C.byref(cost), C.byref(nx), _ptr(flags)), "acnqp_advance_priced_host")
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
        _want(applied, "applied", _F8, (cur.B, cur.N))
        _want(flags, "flags", _I4, (cur.B,))
        p = _device_problems(cur)
        pl = plan._struct(cur.N, self.site.Mg, step, seg_row)
        nx = _Next(*[_dptr(getattr(nxt, k)) for k in _NEXT_ARRAYS], _dptr(warm_x), _dptr(warm_y))
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

    # -- the adjoint of time passes (acn_qp_advance_vjp.hpp) -----------------------------------------------------------------
    def _advance_vjp_plan(self, plan: AdvancePlan, step: int, seg_row, keep=None):
        """(the plan's struct for the call of step ``step``, its clock cost or None); ``seg_row`` None: no arrival"""
        pl = plan._struct(self.site.N, self.site.Mg, step, 0 if seg_row is None else seg_row, keep)
        if seg_row is None:
            pl.a_seg = None
        return pl, plan._cost_struct(self.site.N, keep)

    def advance_vjp(self, cur: dict, plan: AdvancePlan, step: int, applied=None, status=None, x=None, max_pilot=None, gdir=None,
                    gq_next=None, gcap_vjp_next=None, gcap_carry_next=None, horizon_next=None, flags_next=None, garr=None, gprice=None,
                    seg_row=0) -> dict:
        """acnqp_advance_vjp_host: one call of the backward sweep through the closed loop (include/acn_qp.h, "the adjoint of
        time passes") for the state ``cur`` of step ``step`` -- a dict with ``s_off, s_len, s_cap`` (B, K, N) -- under ``plan``
        (numpy arrays).  ``applied``, ``gdir`` (B, N), ``status`` (B,), ``x`` (B, N, Tm), ``max_pilot`` (N,): what the step's
        advance saw and dL/d applied; the ``*_next`` arrays are the adjoints of the next state, None counting as zeros.
        ``garr`` (A,) and ``gprice`` (B, P) are accumulated across calls: pass the arrays of the previous call, or None to start
        from zeros (``gprice`` only with a clock cost).  ``seg_row`` None: no arrival in this step.  Returns a dict with
        ``gcap_carry`` (B, K, N), ``garr``, and, where they apply, ``gx`` (B, N, Tm; not at step -1) and ``gprice``."""
        off, ln, cap = _i4(cur["s_off"]), _i4(cur["s_len"]), _f8(cur["s_cap"])
        if off.ndim != 3 or off.shape[2] != self.site.N or off.shape != ln.shape or off.shape != cap.shape:
            raise ValueError("cur needs s_off, s_len, s_cap of shape (B, K, N) for the handle's site")
        B, K, N = off.shape
        xs = _f8(x)
        if xs is not None and (xs.ndim != 3 or xs.shape[:2] != (B, N)):
            raise ValueError("x must have shape (B, N, Tm)")
        Tm =xs.shape[2] if xs is not None else (np.shape(gq_next)[2] if gq_next is not None else int(plan.q_table.shape[2]))
        keep = []
        pl, cost = self._advance_vjp_plan(plan, step, seg_row, keep)
        out = dict(gx=np.zeros((B, N, Tm)) if step >= 0 else None, gcap_carry=np.zeros((B, K, N)),
                   garr=np.zeros(plan._len("a_evse")) if garr is None else np.ascontiguousarray(garr, np.float64),
                   gprice=(np.zeros((B, plan.c_series.shape[1])) if gprice is None else np.ascontiguousarray(gprice, np.float64))
                   if cost is not None else gprice)
        p = _Problems(B, Tm, K, s_off=_ptr(off), s_len=_ptr(ln), s_cap=_ptr(cap))
        ins = [_f8(applied), _i4(status), xs]
        adj = [_f8(max_pilot), _f8(gdir), _f8(gq_next), _f8(gcap_vjp_next), _f8(gcap_carry_next), _i4(horizon_next), _i4(flags_next)]
        _check(self._lib.acnqp_advance_vjp_host(self._h, C.byref(p), *[_ptr(a) for a in ins], C.byref(pl),
                                                None if cost is None else C.byref(cost), *[_ptr(a) for a in adj], _ptr(out["gx"]),
                                                _ptr(out["gcap_carry"]), _ptr(out["garr"]) if out["garr"].size else None,
                                                _ptr(_f8(out["gprice"]))),
               "acnqp_advance_vjp_host")
        del keep
        return {k: v for k, v in out.items() if v is not None}

    def advance_vjp_device(self, cur: "DeviceBatch", plan: AdvancePlan, step: int, gcap_carry, applied=None, max_pilot=None, gdir=None,
                           gx=None, gq_next=None, gcap_vjp_next=None, gcap_carry_next=None, horizon_next=None, flags_next=None,
                           garr=None, gprice=None, use_status: bool = True, stream: int = 0, seg_row=0) -> None:
        """acnqp_advance_vjp_device: the same on device memory, for the ``DeviceBatch`` ``cur`` of step ``step`` after its solve
        (``cur.x``, ``cur.status`` are read at step >= 0) and ``plan`` from ``AdvancePlan.to_device``.  Float64 device tensors:
        ``applied``, ``gdir`` (B, N), ``max_pilot`` (N,), ``gq_next`` (B, N, Tm), ``gcap_vjp_next``, ``gcap_carry_next`` and the
        output ``gcap_carry`` (B, K, N), the outputs ``gx`` (B, N, Tm), ``garr`` (A,) and ``gprice`` (B, P); int32:
        ``horizon_next``, ``flags_next`` (B,).  ``garr`` and ``gprice`` are accumulated over a sweep: zero them once.
        Asynchronous on ``stream``."""
        B, N, Tm, K = cur.B, cur.N, cur.Tm, cur.K
        d = cur.s_cap.device
        P = None if plan.c_series is None else int(plan.c_series.shape[1])
        for t, name, dt, shape in ((applied, "applied", _F8, (B, N)), (max_pilot, "max_pilot", _F8, (N,)), (gdir, "gdir", _F8, (B, N)),
                                   (gx, "gx", _F8, (B, N, Tm)), (gq_next, "gq_next", _F8, (B, N, Tm)),
                                   (gcap_vjp_next, "gcap_vjp_next", _F8, (B, K, N)), (gcap_carry_next, "gcap_carry_next", _F8, (B, K, N)),
                                   (horizon_next, "horizon_next", _I4, (B,)), (flags_next, "flags_next", _I4, (B,)),
                                   (gcap_carry, "gcap_carry", _F8, (B, K, N)), (garr, "garr", _F8, (plan._len("a_evse"),)),
                                   (gprice, "gprice", _F8, None if P is None else (B, P))):
            _want(t, name, dt, shape, d)
        if gcap_carry is None:
            raise ValueError("gcap_carry must be given")
        pl, cost = self._advance_vjp_plan(plan, step, seg_row)
        p = _device_problems(cur)
        at = step >= 0
        _check(
            self._lib.acnqp_advance_vjp_device(self._h, C.byref(p), _dptr(applied), _dptr(cur.status) if use_status and at else None,
                                               _dptr(cur.x) if at else None, C.byref(pl), None if cost is None else C.byref(cost),
                                               _dptr(max_pilot), _dptr(gdir), _dptr(gq_next), _dptr(gcap_vjp_next), _dptr(gcap_carry_next),
                                               _dptr(horizon_next), _dptr(flags_next), _dptr(gx), _dptr(gcap_carry),
                                               _dptr(garr) if garr is not None and garr.numel() else None, _dptr(gprice), C.c_void_p(stream)),
            "acnqp_advance_vjp_device",
        )

    # -- before the solve (acn_qp_prepare.hpp) ---------------------------------------------------------------------------
    def prepare_host(self, cur: dict, plan: PreparePlan, want_view: bool = True, min_rates: bool = True, key_row=None) -> dict:
        """acnqp_prepare_host: the state ``cur`` -- numpy arrays ``lb, ub`` (B, N, Tm) and ``s_off, s_len, s_cap`` (B, 1, N) or
        (B, N) -- under ``plan`` (numpy arrays).  Returns ``lb, ub`` (copies, period 0 changed when the plan has ``min_pilot``
        and ``min_rates``), ``flags`` (B,) and, with ``want_view``, ``v_evse, v_arrived, v_cap`` (B, N)."""
        lb, ub = np.array(cur["lb"], np.float64, order="C"), np.array(cur["ub"], np.float64, order="C")   # copies: the entry writes them
        off, ln, cap = _i4(cur["s_off"]), _i4(cur["s_len"]), _f8(cur["s_cap"])
        if lb.ndim != 3 or lb.shape[1] != self.site.N or ub.shape != lb.shape:
            raise ValueError("cur needs lb, ub of shape (B, N, Tm) for the handle's site")
        B, N, Tm = lb.shape
        K = off.shape[1] if off.ndim == 3 else 1
        if off.size != B * K * N or ln.size != off.size or cap.size != off.size:
            raise ValueError("cur needs s_off, s_len, s_cap of shape (B, K, N)")
        view = dict(v_evse=np.empty((B, N), np.int32), v_arrived=np.empty((B, N), np.uint8), v_cap=np.empty((B, N))) if want_view else {}
        flags = np.empty(B, np.int32)
        p = _Problems(B, Tm, K, s_off=_ptr(off), s_len=_ptr(ln), s_cap=_ptr(cap))
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
        B, N, Tm, K = cur.B, cur.N, cur.Tm, cur.K
        M = plan._len("cre")
        if plan.key is None or not hasattr(plan.key, "dim"):
            raise ValueError("plan.key must be a tensor on the handle's GPU (PreparePlan.to_device)")
        _want(plan.key, "plan.key", _I4, (B, N) if plan.key.dim() == 2 else (plan.key.shape[0], B, N), here)
        if plan.key.dim() == 3 and not 0 <= (0 if key_row is None else int(key_row)) < plan.key.shape[0]:
            raise ValueError("key_row is outside plan.key")
        for k, shape in dict(cre=(M, N), cim=(M, N), limits=(M,), min_pilot=(N,)).items():
            _want(getattr(plan, k), "plan." + k, _PREPARE_ARRAYS[k], shape, here)
        for k, shape in dict(lb=(B, N, Tm), ub=(B, N, Tm), s_off=(B, K, N), s_len=(B, K, N), s_cap=(B, K, N)).items():
            _want(getattr(cur, k), "cur." + k, _PROBLEM_ARRAYS[k], shape, here)
        _want(flags, "flags", _I4, (B,), here)
        if flags is None:
            raise ValueError("flags is required")
        for t, name, dt in ((v_evse, "v_evse", _I4), (v_arrived, "v_arrived", _U1), (v_cap, "v_cap", _F8)):
            _want(t, name, dt, (B, N), here)
        p = _Problems(B, Tm, K, s_off=_dptr(cur.s_off), s_len=_dptr(cur.s_len), s_cap=_dptr(cur.s_cap))
        pl = plan._struct(N, key_row, min_rates)
        v = _PrepareView(_dptr(v_evse), _dptr(v_arrived), _dptr(v_cap))
        _check(self._lib.acnqp_prepare_device(self._h, C.byref(p), C.byref(pl), _dptr(cur.lb), _dptr(cur.ub), C.byref(v), _dptr(flags),
                                              C.c_void_p(stream)), "acnqp_prepare_device")

    # -- the plant (acn_qp_plant.hpp) -----------------------------------------------------------------------------------
    def plant_host(self, cur: dict, plan: PlantPlan, pilots, bat, room, status=None, plug_row=None) -> dict:
        """acnqp_plant_host: what the EVs of the state ``cur`` -- numpy arrays ``s_off, s_len`` (B, 1, N) or (B, N) -- draw of
        ``pilots`` (B, N) under ``plan`` (numpy arrays), from the plant state ``bat`` (B, N) int32 and ``room`` (B, N).  Returns
        ``bat, room`` (copies, advanced), ``actual`` (B, N) and ``flags`` (B,)."""
        off, ln, pil, stat = _i4(cur["s_off"]), _i4(cur["s_len"]), _f8(pilots), _i4(status)
        bat, room = np.array(bat, np.int32, order="C"), np.array(room, np.float64, order="C")   # copies: the entry writes them
        if pil.ndim != 2 or pil.shape[1] != self.site.N:
            raise ValueError("pilots must have the shape (B, N) of the handle's site")
        B, N = pil.shape
        K = off.shape[1] if off.ndim == 3 else 1
        if off.size != B * K * N or ln.size != off.size or bat.shape != (B, N) or room.shape != (B, N):
            raise ValueError("cur needs s_off, s_len of shape (B, K, N); bat and room have the shape (B, N)")
        plug = plan.plug if plan.plug.ndim == 2 else plan.plug[0 if plug_row is None else plug_row]
        if plug.shape != (B, N) or (stat is not None and stat.shape != (B,)):
            raise ValueError("plan.plug needs one (B, N) block per step and status the shape (B,)")
        actual, flags = np.empty((B, N)), np.empty(B, np.int32)
        p = _Problems(B, 1, K, s_off=_ptr(off), s_len=_ptr(ln))
        keep = []
        _check(self._lib.acnqp_plant_host(self._h, C.byref(p), _ptr(pil), _ptr(stat), *plan._args(plug_row, keep), _ptr(bat), _ptr(room),
                                          _ptr(actual), _ptr(flags)), "acnqp_plant_host")
        del keep
        return dict(bat=bat, room=room, actual=actual, flags=flags)

    def plant_device(self, cur: "DeviceBatch", plan: PlantPlan, pilots, bat, room, actual, flags, status=None, plug_row=None,
                     stream: int = 0) -> None:
        """acnqp_plant_device: ``actual`` (B, N) float64 receives what the EVs of ``cur`` draw of ``pilots`` (B, N); the plant
        state ``bat`` (B, N) int32 and ``room`` (B, N) float64 is advanced in place; ``flags`` (B,) int32.  ``status``: (B,)
        int32 (a problem it does not call solved draws nothing) or None.  ``plan`` from ``PlantPlan.to_device``.  Asynchronous
        on ``stream``."""
        import torch

        here = torch.device("cuda", self.device)
        B, N, K = cur.B, cur.N, cur.K
        R = plan._len("t_room")
        if plan.plug is None or not hasattr(plan.plug, "dim"):
            raise ValueError("plan.plug must be a tensor on the handle's GPU (PlantPlan.to_device)")
        _want(plan.plug, "plan.plug", _I4, (B, N) if plan.plug.dim() == 2 else (plan.plug.shape[0], B, N), here)
        if plan.plug.dim() == 3 and not 0 <= (0 if plug_row is None else int(plug_row)) < plan.plug.shape[0]:
            raise ValueError("plug_row is outside plan.plug")
        for k in ("t_room", "t_amps", "t_knee", "t_slope"):
            _want(getattr(plan, k), "plan." + k, _F8, (R,), here)
        for k in ("s_off", "s_len"):
            _want(getattr(cur, k), "cur." + k, _I4, (B, K, N), here)
        for t, name, dt, shape in ((pilots, "pilots", _F8, (B, N)), (bat, "bat", _I4, (B, N)), (room, "room", _F8, (B, N)),
                                   (actual, "actual", _F8, (B, N)), (flags, "flags", _I4, (B,)), (status, "status", _I4, (B,))):
            if t is None and name != "status":
                raise ValueError(f"{name} is required")
            _want(t, name, dt, shape, here)
        p = _Problems(B, cur.Tm, K, s_off=_dptr(cur.s_off), s_len=_dptr(cur.s_len))
        _check(self._lib.acnqp_plant_device(self._h, C.byref(p), _dptr(pilots), _dptr(status), *plan._args(plug_row), _dptr(bat), _dptr(room),
                                            _dptr(actual), _dptr(flags), C.c_void_p(stream)), "acnqp_plant_device")

    # -- the ramp-down estimator (acn_qp_estimate.hpp) ---------------------------------------------------------------------
    def estimate_host(self, cur: dict, fresh, est, pilots=None, actual=None, status=None, up_threshold: float = 1.0,
                      down_threshold: float = 1.0, up_increment: float = 1.0, fresh_row=None) -> dict:
        """acnqp_estimate_host: the estimate ``est`` (B, N) of what the EVs of the state ``cur`` -- numpy arrays ``lb, ub``
        (B, N, Tm) and ``s_off, s_len`` (B, 1, N) or (B, N) -- accept, moved on by the history of the period before: ``pilots``
        (B, N) or None (no history), ``actual`` (B, N) or None (what was offered was drawn), ``status`` (B,) or None.  ``fresh``:
        (B, N) int32, or (steps, B, N) with ``fresh_row``.  Returns ``est`` (a copy, moved on), ``ub`` (B, N, Tm), the bounds of
        ``cur`` capped with it, and ``flags`` (B,)."""
        lb, ub = _f8(cur["lb"]), _f8(cur["ub"])
        off, ln, fr = _i4(cur["s_off"]), _i4(cur["s_len"]), _i4(fresh)
        pil, act, stat = _f8(pilots), _f8(actual), _i4(status)
        est = np.array(est, np.float64, order="C")   # a copy: the entry writes it
        if ub.ndim != 3 or ub.shape[1] != self.site.N or lb.shape != ub.shape:
            raise ValueError("cur needs lb, ub of shape (B, N, Tm) for the handle's site")
        B, N, Tm = ub.shape
        K = off.shape[1] if off.ndim == 3 else 1
        if fr.ndim == 3:
            fr = fr[0 if fresh_row is None else fresh_row]
        if off.size != B * K * N or ln.size != off.size or fr.shape != (B, N) or est.shape != (B, N):
            raise ValueError("cur needs s_off, s_len of shape (B, K, N); fresh needs one (B, N) block per step and est the shape (B, N)")
        for a, name, shape in ((pil, "pilots", (B, N)), (act, "actual", (B, N)), (stat, "status", (B,))):
            if a is not None and a.shape != shape:
                raise ValueError(f"{name} must have the shape {shape}")
        fr = np.ascontiguousarray(fr)
        ub_out, flags = np.empty((B, N, Tm)), np.empty(B, np.int32)
        p = _Problems(B, Tm, K, s_off=_ptr(off), s_len=_ptr(ln), lb=_ptr(lb), ub=_ptr(ub))
        _check(self._lib.acnqp_estimate_host(self._h, C.byref(p), _ptr(fr), _ptr(pil), _ptr(act), _ptr(stat), float(up_threshold),
                                             float(down_threshold), float(up_increment), _ptr(est), _ptr(ub_out), _ptr(flags)),
               "acnqp_estimate_host")
        return dict(est=est, ub=ub_out, flags=flags)

    def estimate_device(self, cur: "DeviceBatch", fresh, est, ub_out, flags, pilots=None, actual=None, status=None, up_threshold: float = 1.0,
                        down_threshold: float = 1.0, up_increment: float = 1.0, fresh_row=None, stream: int = 0) -> None:
        """acnqp_estimate_device: ``est`` (B, N) float64 is moved on in place by the history of the period before -- ``pilots``,
        ``actual`` (B, N) float64 and ``status`` (B,) int32, each may be None -- and ``ub_out`` (B, N, Tm) float64 receives
        ``cur.ub`` capped with it (``cur.lb``, ``cur.ub`` are read only; ``ub_out`` must be another tensor); ``flags`` (B,)
        int32.  ``fresh``: (B, N) int32, or (steps, B, N) with ``fresh_row``.  Asynchronous on ``stream``."""
        import torch

        here = torch.device("cuda", self.device)
        B, N, Tm, K = cur.B, cur.N, cur.Tm, cur.K
        if fresh is None or not hasattr(fresh, "dim"):
            raise ValueError("fresh must be a tensor on the handle's GPU")
        _want(fresh, "fresh", _I4, (B, N) if fresh.dim() == 2 else (fresh.shape[0], B, N), here)
        row = 0
        if fresh.dim() == 3:
            row = 0 if fresh_row is None else int(fresh_row)
            if not 0 <= row < fresh.shape[0]:
                raise ValueError("fresh_row is outside fresh")
        for k, shape in dict(lb=(B, N, Tm), ub=(B, N, Tm), s_off=(B, K, N), s_len=(B, K, N)).items():
            _want(getattr(cur, k), "cur." + k, _PROBLEM_ARRAYS[k], shape, here)
        for t, name, dt, shape in ((est, "est", _F8, (B, N)), (ub_out, "ub_out", _F8, (B, N, Tm)), (flags, "flags", _I4, (B,)),
                                   (pilots, "pilots", _F8, (B, N)), (actual, "actual", _F8, (B, N)), (status, "status", _I4, (B,))):
            if t is None and name in ("est", "ub_out", "flags"):
                raise ValueError(f"{name} is required")
            _want(t, name, dt, shape, here)
        p = _Problems(B, Tm, K, s_off=_dptr(cur.s_off), s_len=_dptr(cur.s_len), lb=_dptr(cur.lb), ub=_dptr(cur.ub))
        fr = C.c_void_p(fresh.data_ptr() + row * B * N * 4)
        _check(self._lib.acnqp_estimate_device(self._h, C.byref(p), fr, _dptr(pilots), _dptr(actual), _dptr(status), float(up_threshold),
                                               float(down_threshold), float(up_increment), _dptr(est), _dptr(ub_out), _dptr(flags),
                                               C.c_void_p(stream)), "acnqp_estimate_device")

    # -- select and hold (acn_qp_hold.hpp) -------------------------------------------------------------------------------
    def select_device(self, cur: "DeviceBatch", dense: "DeviceBatch", idx, flags, m: Optional[int] = None, warm_x=None, warm_y=None,
                      out_warm_x=None, out_warm_y=None, stream: int = 0) -> None:
        """acnqp_select_device: the first ``m`` problems of ``dense`` (a ``DeviceBatch`` of the same N, Tm, K with room for at
        least m problems; m = len(idx) when None) receive the problems ``idx[0:m]`` of ``cur``; ``idx`` and ``flags`` int32
        device tensors of at least m entries.  ``out_warm_x`` / ``out_warm_y`` (at least m rows): optional float64 device
        tensors that receive rows ``idx`` of ``warm_x`` (B, N, Tm) / ``warm_y`` (B, Mg, Tm).  Asynchronous on ``stream``; m == 0
        launches nothing."""
        m = int(idx.shape[0] if m is None else m)
        if (cur.N, cur.Tm, cur.K) != (dense.N, dense.Tm, dense.K):
            raise ValueError("cur and dense must have the same shape (N, Tm, K)")
        if m > dense.B or m > idx.shape[0] or m > flags.shape[0]:
            raise ValueError(f"dense, idx and flags need room for m = {m} problems")
        for t, name, rows in ((out_warm_x, "out_warm_x", (cur.N, cur.Tm)), (out_warm_y, "out_warm_y", (self.site.Mg, cur.Tm))):
            if t is not None and (t.shape[0] < m or tuple(t.shape[1:]) != rows):
                raise ValueError(f"{name} needs at least m = {m} rows of shape {rows}")
        _want(idx, "idx", _I4)
        _want(flags, "flags", _I4)
        _want(warm_x, "warm_x", _F8, (cur.B, cur.N, cur.Tm))
        _want(warm_y, "warm_y", _F8, (cur.B, self.site.Mg, cur.Tm))
        _want(out_warm_x, "out_warm_x", _F8)
        _want(out_warm_y, "out_warm_y", _F8)
        p = _device_problems(cur, warm_x, warm_y)
        nx = _Next(*[_dptr(getattr(dense, k)) for k in _NEXT_ARRAYS], _dptr(out_warm_x), _dptr(out_warm_y))
        _check(self._lib.acnqp_select_device(self._h, C.byref(p), cur.N, self.site.Mg, m, _dptr(idx), C.byref(nx), _dptr(dense.s_eq),
                                             _dptr(flags), C.c_void_p(stream)), "acnqp_select_device")

    def hold_device(self, cur: "DeviceBatch", dense: Optional["DeviceBatch"], pos, m: int, held_x, prev_status, solved, flags, held_y=None,
                    stream: int = 0) -> None:
        """acnqp_hold_device: ``cur.x, cur.status, cur.iters`` (and ``cur.y`` when ``held_y`` is given) receive the first ``m``
        results of ``dense`` where ``pos`` (B,) int32 names a row, and elsewhere the held schedule ``held_x`` (B, N, Tm) clipped
        into ``cur.lb, cur.ub``, ``held_y`` (B, Mg, Tm), ``prev_status`` (B,) int32 and zero iterations; ``solved`` (B,) uint8,
        ``flags`` (B,) int32.  ``dense`` may be None when m == 0 (everyone is held).  Asynchronous on ``stream``."""
        B, N, Tm, Mg = cur.B, cur.N, cur.Tm, self.site.Mg
        want_y = held_y is not None
        if want_y and (cur.y is None or (dense is not None and dense.y is None)):
            raise ValueError("held_y needs the site-row multipliers: DeviceBatch(..., want_y=True)")
        if dense is None and m != 0:
            raise ValueError("dense is required when m > 0")
        if dense is not None and ((dense.N, dense.Tm) != (N, Tm) or dense.B < m):
            raise ValueError(f"dense must have the shape (N, Tm) of cur and hold at least m = {m} problems")
        for t, name, dt, shape in ((pos, "pos", _I4, (B,)), (held_x, "held_x", _F8, (B, N, Tm)), (held_y, "held_y", _F8, (B, Mg, Tm)),
                                   (prev_status, "prev_status", _I4, (B,)), (solved, "solved", _U1, (B,)), (flags, "flags", _I4, (B,))):
            _want(t, name, dt, shape)
        p = _Problems(B, Tm, cur.K, lb=_dptr(cur.lb), ub=_dptr(cur.ub))
        r = _Results() if dense is None else _Results(x=_dptr(dense.x), status=_dptr(dense.status), iters=_dptr(dense.iters),
                                                      y=_dptr(dense.y) if want_y else None)
        o = _Results(x=_dptr(cur.x), status=_dptr(cur.status), iters=_dptr(cur.iters), y=_dptr(cur.y) if want_y else None)
        _check(self._lib.acnqp_hold_device(self._h, C.byref(p), N, Mg, int(m), _dptr(pos), C.byref(r), _dptr(held_x), _dptr(held_y),
                                           _dptr(prev_status), C.byref(o), _dptr(solved), _dptr(flags), C.c_void_p(stream)),
               "acnqp_hold_device")

    def select_host(self, cur: dict, idx, warm_x=None, warm_y=None) -> dict:
        """acnqp_select_host: the dense batch of the problems ``idx`` of the state ``cur`` -- a dict of numpy arrays named as the
        fields of ``acnqp_problems`` -- as a dict of the same layout with ``flags``, and ``warm_x`` / ``warm_y`` when given."""
        src = {k: np.ascontiguousarray(cur[k], dt) for k, dt in _PROBLEM_ARRAYS.items() if cur.get(k) is not None and k not in _absent(self.site, peak=True)}
        idx = _i4(idx)
        wx, wy = _f8(warm_x), _f8(warm_y)
        B, N, Tm = src["lb"].shape
        K, m = src["s_off"].shape[1], len(idx)
        out = {k: np.empty((m,) + a.shape[1:], a.dtype) for k, a in src.items()}
        if wx is not None:
            out["warm_x"] = np.empty((m, N, Tm))
        if wy is not None:
            out["warm_y"] = np.empty((m,) + wy.shape[1:])
        out["flags"] = np.empty(m, np.int32)
        p = _Problems(B, Tm, K, *[_ptr(src.get(k)) for k in _PROBLEM_ARRAYS], _ptr(wx), _ptr(wy))
        nx = _Next(*[_ptr(out.get(k)) for k in _NEXT_ARRAYS + _WARM])
        _check(self._lib.acnqp_select_host(self._h, C.byref(p), N, self.site.Mg, m, _ptr(idx), C.byref(nx), _ptr(out["s_eq"]),
                                           _ptr(out["flags"])), "acnqp_select_host")
        return out

    def hold_host(self, pos, m: int, rx, rstatus, riters, held_x, prev_status, lb, ub, ry=None, held_y=None) -> dict:
        """acnqp_hold_host on numpy arrays, in the argument order of tests/hold_spec.py's ``hold``: a dict of ``x, status,
        iters, solved, flags`` and, with ``held_y``, ``y``."""
        pos, rst, rit, pst = _i4(pos), _i4(rstatus), _i4(riters), _i4(prev_status)
        rx, ry, hx, hy, lb, ub = _f8(rx), _f8(ry), _f8(held_x), _f8(held_y), _f8(lb), _f8(ub)
        B, N, Tm = hx.shape
        out = dict(x=np.empty((B, N, Tm)), status=np.empty(B, np.int32), iters=np.empty(B, np.int32), solved=np.empty(B, np.uint8),
                   flags=np.empty(B, np.int32))
        if hy is not None:
            out["y"] = np.empty(hy.shape)
        nul = lambda a: None if a is None or a.size == 0 else _ptr(a)
        p = _Problems(B, Tm, 1, lb=_ptr(lb), ub=_ptr(ub))
        r = _Results(x=nul(rx), status=nul(rst), iters=nul(rit), y=nul(ry))
        o = _Results(x=_ptr(out["x"]), status=_ptr(out["status"]), iters=_ptr(out["iters"]), y=_ptr(out.get("y")))
        _check(self._lib.acnqp_hold_host(self._h, C.byref(p), N, self.site.Mg, int(m), _ptr(pos), C.byref(r), _ptr(hx), _ptr(hy), _ptr(pst),
                                         C.byref(o), _ptr(out["solved"]), _ptr(out["flags"])), "acnqp_hold_host")
        return out

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
        n = int(self._lib.acnqp_debug_polish_alongside(self._h))
        if n < 0:
            raise RuntimeError("acnqp_debug_polish_alongside failed")
        return n

    def wave_rank(self) -> dict:
        """The site's live eigenpairs, the MFMA k-steps that hold them once compacted, and the eigen extent (k-steps) of
        the wave kernel's instantiation this handle runs (acnqp_debug_wave_rank: introspection, not part of the ABI)."""
        buf = (C.c_int32 * 3)()
        if self._lib.acnqp_debug_wave_rank(self._h, buf) != 0:
            raise RuntimeError("acnqp_debug_wave_rank failed")
        return dict(rank=int(buf[0]), eig_ksteps=int(buf[1]), extent=int(buf[2]))

    def wave_evse_extent(self) -> dict:
        """The site's EVSEs, the MFMA k-steps of P = Ghat r0 that hold one, and the EVSE k-steps the wave kernel's
        instantiation this handle runs sums over (acnqp_debug_wave_evse_extent: introspection, not part of the ABI)."""
        buf = (C.c_int32 * 3)()
        if self._lib.acnqp_debug_wave_evse_extent(self._h, buf) != 0:
            raise RuntimeError("acnqp_debug_wave_evse_extent failed")
        return dict(n_evse=int(buf[0]), evse_ksteps=int(buf[1]), extent=int(buf[2]))

    def order_keys(self, dev: "DeviceBatch") -> np.ndarray:
        """The launch-order keys (B,) int32 of a ``DeviceBatch`` of any size: what a launch of 768 problems or more is
        sorted by, largest first (acnqp_debug_order_keys: introspection, not part of the ABI; synchronises)."""
        keys = np.empty(dev.B, np.int32)
        p = _device_problems(dev)
        if self._lib.acnqp_debug_order_keys(self._h, C.byref(p), keys.ctypes.data_as(C.POINTER(C.c_int32))) != 0:
            raise RuntimeError("acnqp_debug_order_keys failed")
        return keys

    def direct_x(self) -> int:
        """Problems of this handle's last host-entry call whose schedule the kernel stored straight into the caller's pinned
        result array instead of a copy (acnqp_debug_direct_x: introspection, not part of the ABI)."""
        return int(self._lib.acnqp_debug_direct_x(self._h))

    def direct_in(self) -> int:
        """Problems of this handle's last host-entry call whose lb, ub and q the kernel loaded straight from the caller's
        pinned arrays instead of a copy (acnqp_debug_direct_in: introspection, not part of the ABI)."""
        return int(self._lib.acnqp_debug_direct_in(self._h))

    def ordered_launches(self) -> int:
        """Launches of this handle whose queue order was sorted by a key (acnqp_ordered_launch_count)."""
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
        for k, dt in _PROBLEM_ARRAYS.items():
            a = getattr(batch, "T" if k == "horizon" else k)
            if a is None and k in ("lf", "dc", "dfloor"):   # a batch without the term: the tensor is there all the same
                a = np.zeros(batch.B)
            setattr(self, k, None if a is None else torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev))
        self._alloc_results(batch.site.Mg, want_y, dev)

    def _alloc_results(self, Mg: int, want_y: bool, dev) -> None:
        """zeroed result tensors: those of ``_RESULT_ARRAYS`` and, when wanted, the site-row multipliers y (B, Mg, Tm)
        (acnqp_results.y), else None"""
        import torch

        for k, dt in _RESULT_ARRAYS.items():
            setattr(self, k, torch.zeros((self.B, self.N, self.Tm) if k == "x" else self.B, dtype=_torch_dtype(dt), device=dev))
        self.y = torch.zeros((self.B, Mg, self.Tm), dtype=torch.float64, device=dev) if want_y else None

    def head(self, m: int) -> "DeviceBatch":
        """The first ``m`` problems as a ``DeviceBatch`` of their own: views, no copy (every array leads with the problem)."""
        if not 0 <= m <= self.B:
            raise ValueError(f"m must be in [0, {self.B}]")
        view = self.__class__.__new__(self.__class__)
        view.B, view.N, view.Tm, view.K = int(m), self.N, self.Tm, self.K
        for k in (*_PROBLEM_ARRAYS, *_RESULT_ARRAYS, "y"):
            t = getattr(self, k)
            setattr(view, k, None if t is None else t[:m])
        return view

    @classmethod
    def empty(cls, site: SiteData, B: int, Tm: int, K: int, device, want_y: bool = False, s_eq: int = 0, dfloor: float = 0.0,
              with_peak: Optional[bool] = None) -> "DeviceBatch":
        """An empty state of shape (B, N, Tm, K) in HBM: no session in any slot, zero bounds and cost, horizon 1, no peak limit.
        What ``SiteHandle.advance_device`` writes into, and -- with ``step = -1`` -- what a rollout starts from."""
        import torch

        dev = torch.device(device)
        self = cls.__new__(cls)
        self.B, self.N, self.Tm, self.K = int(B), site.N, int(Tm), int(K)
        shapes = dict(lb=(self.B, self.N, self.Tm), ub=(self.B, self.N, self.Tm), q=(self.B, self.N, self.Tm), s_off=(self.B, self.K, self.N),
                      s_len=(self.B, self.K, self.N), s_cap=(self.B, self.K, self.N), peak=(self.B, self.Tm))
        fill = dict(horizon=1, dfloor=float(dfloor), s_eq=int(s_eq), peak=float("inf"))
        no_peak = not (site.has_peak if with_peak is None else with_peak)
        for k, dt in _PROBLEM_ARRAYS.items():
            setattr(self, k, None if k == "peak" and no_peak else
                    torch.full(shapes.get(k, (self.B,)), fill.get(k, 0), dtype=_torch_dtype(dt), device=dev))
        self._alloc_results(site.Mg, want_y, dev)
        return self
