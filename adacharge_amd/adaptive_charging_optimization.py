"""Host-side mirror of the reference's optimisation surface
(/root/reference/adacharge/adaptive_charging_optimization.py).

Same names, arguments and error behaviour as the reference:
``AdaptiveChargingOptimization(objective, interface, constraint_type="SOC",
enforce_energy_equality=False, solver="ECOS")`` and ``.solve(active_sessions,
infrastructure, peak_limit=None, prev_peak=0, verbose=False) -> (N, T)`` array
(aco.py:31-43, 286-321); ``ObjectiveComponent`` (aco.py:12-15);
``InfeasibilityException`` (aco.py:8-9); the objective library (aco.py:336-408).

What changes is what sits underneath: the cvxpy ``Problem.solve`` call
(aco.py:315-318) is replaced by the structured builder (builder.py) and the
HIP batched ADMM solver behind the C-ABI (include/acn_qp.h).  There is no CPU
fallback: if the HIP library is missing, ``solve`` raises.

Deviations that cannot be avoided without cvxpy:
objective functions return ``QuadObjective`` descriptors, not cvxpy
expressions, so user-defined objectives must be built from the helpers here;
``build_problem`` returns the structured ``ProblemBatch`` instead of cvxpy
objects.
"""
from __future__ import annotations

from collections import namedtuple
from typing import List, Optional, Sequence, Union

import numpy as np


class InfeasibilityException(Exception):
    pass


ObjectiveComponent = namedtuple("ObjectiveComponent", ["function", "coefficient", "kwargs"])
ObjectiveComponent.__new__.__defaults__ = (1, {})


# ---------------------------------------------------------------------------
# Descriptor algebra standing in for cvxpy expressions
# ---------------------------------------------------------------------------
class Rates:
    """Symbolic handle for the (N, T) rates variable (cp.Variable at aco.py:247)."""

    def __init__(self, shape):
        self.shape = tuple(shape)


class QuadObjective:
    """A concave objective term in the reference's *maximisation* convention:

        value(r) = <lin, r>  -  sq * sum(r^2)  -  flat * sum_t (v' r[:, t])^2  +  const

    with v = voltages / 1e3.  Closed under ``+`` and scalar ``*`` exactly like
    the cvxpy expressions it replaces (aco.py:210-218)."""

    __array_priority__ = 1000

    def __init__(self, lin, sq=0.0, flat=0.0, const=0.0, epigraph=None):
        self.lin = np.asarray(lin, float)
        self.sq = float(sq)
        self.flat = float(flat)
        self.const = float(const)
        self.epigraph = list(epigraph) if epigraph else []

    @classmethod
    def zero(cls, shape):
        return cls(np.zeros(shape))

    def __add__(self, other):
        if np.isscalar(other):
            return QuadObjective(self.lin, self.sq, self.flat, self.const + other, self.epigraph)
        return QuadObjective(
            self.lin + other.lin, self.sq + other.sq, self.flat + other.flat,
            self.const + other.const, self.epigraph + other.epigraph,
        )

    __radd__ = __add__

    def __mul__(self, c):
        c = float(c)
        return QuadObjective(
            c * self.lin, c * self.sq, c * self.flat, c * self.const,
            [(c * w, spec) for w, spec in self.epigraph],
        )

    __rmul__ = __mul__

    def __neg__(self):
        return self * -1.0

    def __sub__(self, other):
        return self + (-other)


# ---------------------------------------------------------------------------
#  Objective functions -- same signatures as aco.py:336-408.  All take rates as
#  first positional argument and swallow unknown keyword arguments.
# ---------------------------------------------------------------------------
def _volt_kw(infrastructure):
    return np.asarray(infrastructure.voltages, float) / 1e3


def quick_charge(rates, infrastructure, interface, **kwargs):
    """aco.py:363-371: sum_t ((T - t) / T) * sum_i r[i, t]."""
    T = rates.shape[1]
    c = np.array([(T - t) / T for t in range(T)])
    return QuadObjective(np.broadcast_to(c, rates.shape).copy())


def equal_share(rates, infrastructure, interface, **kwargs):
    """aco.py:374-375: -sum_squares(rates)."""
    return QuadObjective(np.zeros(rates.shape), sq=1.0)


def tou_energy_cost(rates, infrastructure, interface, **kwargs):
    """aco.py:378-380: -prices @ aggregate_period_energy."""
    prices = np.asarray(interface.get_prices(rates.shape[1]), float)
    v = _volt_kw(infrastructure)
    return QuadObjective(-(v[:, None] * (interface.period / 60)) * prices[None, :])


def total_energy(rates, infrastructure, interface, **kwargs):
    """aco.py:383-384: sum of per-period energy in kWh."""
    v = _volt_kw(infrastructure)
    return QuadObjective(np.repeat((v * (interface.period / 60))[:, None], rates.shape[1], axis=1))


def load_flattening(rates, infrastructure, interface, external_signal=None, **kwargs):
    """aco.py:403-408: -sum_t (v' r_t + ext_t)^2."""
    T = rates.shape[1]
    ext = np.zeros(T) if external_signal is None else np.asarray(external_signal, float)
    v = _volt_kw(infrastructure)
    return QuadObjective(-2.0 * v[:, None] * ext[None, :], flat=1.0, const=-float(ext @ ext))


def peak(rates, infrastructure, interface, baseline_peak=0, **kwargs):
    """aco.py:387-394: max(max_t aggregate_power_t, prev_peak kW[, baseline_peak]).
    Convex; only usable with a negative coefficient (as ``demand_charge`` does).
    Carried as an epigraph request for the builder."""
    prev_peak = interface.get_prev_peak() * infrastructure.voltages[0] / 1000
    floor = max(prev_peak, baseline_peak) if baseline_peak > 0 else prev_peak
    return QuadObjective(np.zeros(rates.shape), epigraph=[(1.0, {"floor": float(floor)})])


def demand_charge(rates, infrastructure, interface, baseline_peak=0, **kwargs):
    """aco.py:397-400: -demand_charge * peak."""
    p = peak(rates, infrastructure, interface, baseline_peak, **kwargs)
    dc = interface.get_demand_charge()
    return -dc * p


# ---------------------------------------------------------------------------
#  The optimiser (aco.py:18-321)
# ---------------------------------------------------------------------------
_HANDLE_CACHE = {}          # insertion-ordered: least recently used first
_HANDLE_CACHE_MAX = 64


def _site_handle(infrastructure, constraint_type, with_peak, device, with_flat=False, with_max=False, polish_long=False, polish_wide=False,
                 vjp_long=False):
    """One uploaded site per (infrastructure content, cone, peak, GPU, long-horizon and wide-site polish switches, long-horizon
    gradient switch).  The
    reference rebuilds every atom on every call (adacharge.py:152-158); here the
    site matrix is uploaded once and reused by all later MPC steps.  The switch is part of the key: it is a property
    of the handle (``acnqp_set_long_polish``, ``acnqp_set_wide_polish``, ``acnqp_set_long_vjp``), and two optimizers must never flip each other's."""
    from . import backend
    from .builder import make_site

    cm = infrastructure.constraint_matrix
    key = (
        None if cm is None else (cm.shape, cm.tobytes()),
        None if infrastructure.constraint_limits is None else np.asarray(infrastructure.constraint_limits).tobytes(),
        None if infrastructure.phases is None else np.asarray(infrastructure.phases).tobytes(),
        np.asarray(infrastructure.voltages).tobytes(),
        constraint_type, bool(with_peak), int(device), bool(with_flat), bool(with_max), bool(polish_long), bool(polish_wide),
        bool(vjp_long),
    )
    ent = _HANDLE_CACHE.pop(key, None)
    if ent is None:
        site = make_site(infrastructure, constraint_type, with_peak=with_peak, with_flat=with_flat, with_max=with_max)
        ent = (site, backend.SiteHandle(site, device, polish_long=bool(polish_long), polish_wide=bool(polish_wide), vjp_long=bool(vjp_long)))
        while len(_HANDLE_CACHE) >= _HANDLE_CACHE_MAX:   # least recently used out; a caller that still holds the pair
            _HANDLE_CACHE.pop(next(iter(_HANDLE_CACHE)))  # keeps its handle alive (SiteHandle frees the device side in __del__)
    _HANDLE_CACHE[key] = ent                             # (re-)inserted last = most recently used
    return ent


def warn_inaccurate(status, pri_res, dua_res):
    """A schedule accepted as OPTIMAL_INACCURATE (aco.py:319 accepts it, and so does this path) is announced the way the
    reference's solver layer announces it -- cvxpy's ``Problem.solve`` emits a UserWarning "Solution may be inaccurate"
    for that status -- with the residuals the device reached, so the caller can judge the distance to the tolerances
    asked for (``last_result`` keeps them per problem).  Returns the number of such problems."""
    import warnings

    from . import backend

    status = np.asarray(status)
    bad = np.flatnonzero(status == backend.STATUS_SOLVED_INACCURATE)
    if bad.size:
        warnings.warn(
            f"Solution may be inaccurate: {bad.size} of {status.size} problems ended OPTIMAL_INACCURATE "
            f"(worst primal residual {float(np.max(np.asarray(pri_res)[bad])):.2e}, dual {float(np.max(np.asarray(dua_res)[bad])):.2e}); "
            "raise max_iter / retry_passes or inspect last_result", UserWarning, stacklevel=3)
    return int(bad.size)


class AdaptiveChargingOptimization:
    """Base class for all MPC based charging algorithms (aco.py:18-43).

    Args:
        objective (List[ObjectiveComponent]): components of the objective.
        interface: object providing ``period`` (and prices / demand charge /
            previous peak when the objective needs them).
        constraint_type (str): 'SOC' or 'LINEAR' (aco.py:35).
        enforce_energy_equality (bool): energy rows are equalities (aco.py:36).
        solver (str): accepted for source compatibility with the reference
            ("ECOS", "OSQP", None, cvxpy constants ...); every value runs the
            HIP ADMM backend.  Backend options go in ``solver_options``.
        solver_options (dict): overrides of ``acnqp_options`` fields
            (eps_abs, eps_rel, max_iter, rho, reg_rel, precision, ...), plus
            ``retry_stalled`` (default True; False = ``retry_passes=0``):
            problems the adaptive first pass leaves on a residual plateau
            are solved again from a cold start with a fixed penalty, inside
            the library (``acnqp_options.retry_passes``, include/acn_qp.h);
            and ``polish_long`` (default False): the Newton polish also takes
            over at horizons 33 ... 288 on sites of up to 64 EVSEs
            (``acnqp_set_long_polish``; a switch of the site handle, not an
            ``acnqp_options`` field); and ``polish_wide`` (default False):
            on sites of 65 ... 1,024 EVSEs the Newton polish runs behind
            the solve on what it left MAX_ITER or SOLVED_INACCURATE
            (``acnqp_set_wide_polish``; a switch of the site handle too);
            and ``vjp_long`` (default False): ``schedule_gradients`` also
            serves horizons 33 ... 288 on sites of up to 64 EVSEs
            (``acnqp_set_long_vjp``; a switch of the site handle too).
        device (int): HIP device ordinal.
    """

    def __init__(
        self,
        objective: List[ObjectiveComponent],
        interface,
        constraint_type="SOC",
        enforce_energy_equality=False,
        solver="ECOS",
        solver_options: Optional[dict] = None,
        device: int = 0,
    ):
        self.interface = interface
        self.constraint_type = constraint_type
        self.enforce_energy_equality = enforce_energy_equality
        self.solver = solver
        self.objective_configuration = objective
        self.solver_options = dict(solver_options or {})
        self.device = device
        self.last_result = None
        self._last_plan = None
        self._last_batch = None
        self._last_handle = None
        self._last_options = None
        self._last_duals = None

    # the single-problem API asks for tighter residuals than the batch default so that the
    # reference's own test tolerances (1e-7 on the peak row, t_aco.py:257) hold
    _SINGLE_DEFAULTS = dict(eps_abs=1e-9, eps_rel=1e-9, max_iter=100000)

    # -- the reference's constraint builders (aco.py:45-198) -----------------------------------
    # They return cvxpy constraints there; here they return the numeric description of the same
    # constraint blocks (the arrays the C-ABI consumes), keyed exactly like the reference's dicts.
    @staticmethod
    def charging_rate_bounds(rates, active_sessions, evse_index):
        """aco.py:45-79: ``lb <= rates <= ub``; later sessions overwrite their own window and
        ``ub < lb`` is replaced by ``lb``."""
        lb, ub = np.zeros(rates.shape), np.zeros(rates.shape)
        for session in active_sessions:
            i = evse_index.index(session.station_id)
            w = slice(session.arrival_offset, session.arrival_offset + session.remaining_time)
            lb[i, w] = session.min_rates
            ub[i, w] = session.max_rates
        ub[ub < lb] = lb[ub < lb]
        return {"charging_rate_bounds.lb": lb, "charging_rate_bounds.ub": ub}

    @staticmethod
    def energy_constraints(rates, active_sessions, infrastructure, period, enforce_energy_equality=False):
        """aco.py:81-124: one row per session, ``coef * sum(rates[i, off:off+len]) <= (==) rhs``."""
        out = {}
        for session in active_sessions:
            i = infrastructure.get_station_index(session.station_id)
            out[f"energy_constraints.{session.session_id}"] = dict(
                evse=i, offset=session.arrival_offset, length=session.remaining_time,
                coefficient=infrastructure.voltages[i] * period / 1e3 / 60,
                rhs=session.remaining_demand, equality=bool(enforce_energy_equality),
            )
        return out

    @staticmethod
    def infrastructure_constraints(rates, infrastructure, constraint_type="SOC"):
        """aco.py:126-179: per constraint id, the row(s) applied to every period and the limit."""
        from .builder import _bad_constraint_type

        cm = infrastructure.constraint_matrix
        if cm is None or cm.shape == (0, 0):
            return {}
        out = {}
        if constraint_type == "SOC":
            if infrastructure.phases is None:
                raise ValueError("phases is required when using SOC infrastructure constraints.")
            ph = np.deg2rad(infrastructure.phases)
            for j, v in enumerate(cm):
                out[f"infrastructure_constraints.{infrastructure.constraint_ids[j]}"] = dict(
                    rows=np.stack([v * np.cos(ph), v * np.sin(ph)]), norm="l2", limit=infrastructure.constraint_limits[j])
        elif constraint_type == "LINEAR":
            for j, v in enumerate(cm):
                out[f"infrastructure_constraints.{infrastructure.constraint_ids[j]}"] = dict(
                    rows=np.abs(v)[None, :], norm="linear", limit=infrastructure.constraint_limits[j])
        else:
            _bad_constraint_type(constraint_type)
        return out

    @staticmethod
    def peak_constraint(rates, peak_limit):
        """aco.py:181-198: ``sum(rates, axis=0) <= peak_limit`` if a limit is given."""
        if peak_limit is not None:
            return {"peak_constraint": np.broadcast_to(np.asarray(peak_limit, float), (rates.shape[1],)).copy()}
        return {}

    def build_objective(self, rates, infrastructure, **kwargs):
        """aco.py:200-218: weighted sum of the objective components (a ``QuadObjective``)."""
        obj = QuadObjective.zero(rates.shape)
        for component in self.objective_configuration:
            merged = dict(kwargs)
            merged.update(component.kwargs)
            obj = obj + component.coefficient * component.function(rates, infrastructure, self.interface, **merged)
        return obj

    def build_problem(
        self,
        active_sessions,
        infrastructure,
        peak_limit: Optional[Union[float, List[float], np.ndarray]] = None,
        prev_peak: float = 0,
    ):
        """aco.py:220-284.  Returns the structured one-problem ``ProblemBatch``
        (the reference returns cvxpy objects; see module docstring)."""
        from .builder import build_batch

        return build_batch(
            [active_sessions], infrastructure, self.interface, self.objective_configuration,
            self.constraint_type, self.enforce_energy_equality,
            peak_limits=[peak_limit], prev_peak=prev_peak,
        )

    def solve(
        self,
        active_sessions,
        infrastructure,
        peak_limit: Union[float, List[float], np.ndarray] = None,
        prev_peak=0,
        verbose: bool = False,
        warm_start=None,
    ):
        """aco.py:286-321: (N, T) array of charging rates; raises
        ``InfeasibilityException`` unless the solve ends optimal.

        ``warm_start`` (extension; the reference starts every solve from nothing, adacharge.py:152-158):
        ``(x0, y0)`` -- a schedule (N, >= T) and the site-row multipliers ``last_multipliers`` (Mg, >= T) of an
        earlier, similar solve, already shifted to this problem's first period (the site must carry the same rows:
        same constraint type, peak / load-flattening / demand-charge rows).  Changes the iteration count, not the optimum."""
        if len(active_sessions) == 0:  # aco.py:310-311
            return np.zeros((infrastructure.num_stations, 1))
        rates, status = self.solve_batch(
            [active_sessions], infrastructure, peak_limits=[peak_limit], prev_peak=prev_peak,
            verbose=verbose, _defaults=self._SINGLE_DEFAULTS, warm_start=[warm_start],
        )
        from . import backend

        if status[0] not in backend.ACCEPTED_STATUSES:  # aco.py:319-320 (OPTIMAL or OPTIMAL_INACCURATE)
            raise InfeasibilityException(
                f"Solve failed with status {backend.STATUS_NAMES.get(int(status[0]), status[0])}"
            )
        return rates[0]

    def solve_table(self, table, infrastructure, peak_limits=None, prev_peak=0, _defaults: Optional[dict] = None,
                    warm_start=None, keep_on_device: bool = False):
        """Batched solve of a ``session_table.SessionTable`` (every snapshot non-empty): the array-native entry --
        no Python loop over sessions anywhere on the path, and (round 4) no dense (B, N, T) problem array on the host
        either: the sessions go to the library as they are (``acnqp_solve_table``) and ``charging_rate_bounds`` /
        ``energy_constraints`` / the linear cost (aco.py:45-124, 200-218) take their array form on the device.
        Returns ``(backend.BatchResult, builder.TablePlan)``; a warm start takes the dense entry (``plan.expand()``).
        ``keep_on_device``: the schedules also stay in HBM (``BatchResult.x_dev``, a float64 tensor on the handle's GPU;
        ``BatchResult.handle`` is the handle that owns it) for ``postprocessing.postprocess_batch_device``."""
        from . import backend
        from .builder import _bad_constraint_type, _objective_needs_flat, _objective_needs_max, plan_from_table

        if self.constraint_type not in ("SOC", "LINEAR"):
            _bad_constraint_type(self.constraint_type)
        pl = [None] * table.B if peak_limits is None else list(peak_limits)
        site, handle = _site_handle(
            infrastructure, self.constraint_type, any(p is not None for p in pl), self.device,
            with_flat=_objective_needs_flat(self.objective_configuration),
            with_max=_objective_needs_max(self.objective_configuration),
            polish_long=bool(self.solver_options.get("polish_long", False)),
            polish_wide=bool(self.solver_options.get("polish_wide", False)),
            vjp_long=bool(self.solver_options.get("vjp_long", False)),
        )
        plan = plan_from_table(
            table, infrastructure, self.interface, self.objective_configuration, self.constraint_type,
            self.enforce_energy_equality, peak_limits=pl, prev_peak=prev_peak, site=site,
        )
        opts = dict(_defaults or {})
        opts.update(self.solver_options)
        opts.pop("polish_long", None)   # (consumed above: the handle's switches)
        opts.pop("polish_wide", None)
        opts.pop("vjp_long", None)
        if not bool(opts.pop("retry_stalled", True)):   # shorthand kept from round 2: the passes live in the library now
            opts["retry_passes"] = 0
        self._last_plan, self._last_batch = plan, None
        self._last_table, self._last_infrastructure = table, infrastructure
        self._last_handle, self._last_options, self._last_duals = handle, backend.default_options(**opts), None
        if warm_start is not None and any(w is not None for w in warm_start):
            # per problem (x0, y0) or None; a problem without one starts from its own cold start's point only if all
            # are None -- mixed batches give the cold problems x0 = y0 = 0 (a valid, if plain, starting point)
            batch = self.last_batch
            wx = np.zeros((batch.B, batch.N, batch.Tm))
            wy = np.zeros((batch.B, site.Mg, batch.Tm))
            for b, w in enumerate(warm_start):
                if w is not None:
                    x0, y0 = np.asarray(w[0], float), np.asarray(w[1], float)
                    T = min(batch.Tm, x0.shape[1], y0.shape[1])
                    wx[b, :, :T], wy[b, :, :T] = x0[:, :T], y0[:, :T]
            res = handle.solve(batch, backend.default_options(**opts), warm=(wx, wy), want_y=True)
        else:
            x_dev = None
            if keep_on_device:
                import torch

                x_dev = torch.empty((plan.B, plan.N, plan.Tm), dtype=torch.float64, device=torch.device("cuda", handle.device))
            res = handle.solve_table(plan, backend.default_options(**opts), want_y=True, x_dev=x_dev)
        if keep_on_device and res.x_dev is None:   # (the warm-started dense entry: upload its answer)
            import torch

            res.x_dev = torch.from_numpy(np.ascontiguousarray(res.x)).to(torch.device("cuda", handle.device))
        res.handle = handle
        self.last_result = res
        return res, plan

    @property
    def last_batch(self):
        """The structured problems behind ``last_result`` as dense arrays (diagnostics, tests): expanded on demand."""
        if getattr(self, "_last_batch", None) is None and getattr(self, "_last_plan", None) is not None:
            self._last_batch = self._last_plan.expand()
        return getattr(self, "_last_batch", None)

    @property
    def last_duals(self):
        """``backend.DualResult`` of the last solve: the multipliers of the energy rows (``mu``) and of the rate bounds
        (``z``) and the KKT residuals of every problem of ``last_result``, computed on the GPU from ``last_result`` and
        ``last_batch`` on first access (no solve pays for it), then cached.  Units of the C ABI (include/acn_qp.h); they
        are the duals of the problem the kernels solve, the Tikhonov floor ``reg_rel`` of LP-like problems included."""
        if getattr(self, "_last_duals", None) is None and self.last_result is not None and getattr(self, "_last_handle", None) is not None:
            self._last_duals = self._last_handle.duals(self.last_batch, self.last_result, self._last_options)
        return getattr(self, "_last_duals", None)

    def dual_values(self, active_sessions, infrastructure, b: int = 0):
        """Dual values of problem ``b`` of the last solve, keyed exactly like the constraints dict the reference's
        ``build_problem`` returns (aco.py:245-276), in the reference's units (rates in A, energy in kWh):

          * ``charging_rate_bounds.lb`` / ``.ub``: (N, T) arrays ``max(-z, 0)`` / ``max(z, 0)``;
          * ``energy_constraints.<session_id>``: ``mu / k_i`` with ``k_i = voltage_i * period / 1e3 / 60`` (per kWh,
            aco.py:114);
          * ``infrastructure_constraints.<id>``: (T,) array, ``y_j`` (LINEAR) or ``|(y_j, y_{j+M})|`` (SOC);
          * ``peak_constraint``: (T,) array, the peak row of ``y`` (only when the solve had a peak limit).

        Sign convention: with ``f`` the MINIMISED objective (the negative of the reference's maximised one), rates ``r``
        and ``nu`` the value reported for a session, the Lagrangian is ``L = f + nu (k sum r - demand) + ...``.  Every
        value is non-negative except an equality energy row's, whose sign follows that Lagrangian.  cvxpy is not a
        dependency of this package, so the sign and scaling conventions of its ``constraint.dual_value`` have not been
        compared with these; the Lagrangian above is what is guaranteed.  The values are the duals of the problem the
        kernels solve (for LP-like objectives that includes the Tikhonov floor ``reg_rel``)."""
        d, res, batch = self.last_duals, self.last_result, self.last_batch
        if d is None:
            raise RuntimeError("dual_values: no solve yet")
        from . import backend

        if int(res.status[b]) not in backend.ACCEPTED_STATUSES:
            raise InfeasibilityException(f"problem {b} ended with status {backend.STATUS_NAMES.get(int(res.status[b]), res.status[b])}: no dual values")
        site = batch.site
        T, M = int(batch.T[b]), site.M
        z, y = d.z[b][:, :T], res.y[b][:, :T]
        out = {"charging_rate_bounds.lb": np.maximum(-z, 0.0), "charging_rate_bounds.ub": np.maximum(z, 0.0)}
        for session in active_sessions:
            i = infrastructure.get_station_index(session.station_id)
            slot = np.flatnonzero((batch.s_len[b, :, i] > 0) & (batch.s_off[b, :, i] == session.arrival_offset))
            if session.remaining_time <= 0 or slot.size == 0:
                out[f"energy_constraints.{session.session_id}"] = 0.0
                continue
            k_i = infrastructure.voltages[i] * self.interface.period / 1e3 / 60
            out[f"energy_constraints.{session.session_id}"] = float(d.mu[b, slot[0], i]) / k_i
        for j in range(M):
            val = np.hypot(y[j], y[j + M]) if site.cone == 1 else y[j].copy()
            out[f"infrastructure_constraints.{infrastructure.constraint_ids[j]}"] = val
        if site.has_peak and np.isfinite(batch.peak[b][:T]).any():
            out["peak_constraint"] = y[site.Mg - 1].copy()
        return out

    def schedule_gradients(self, grad_rates, b: int = 0):
        """How a scalar ``L`` of the optimal schedule of problem ``b`` of the last solve moves with the problem's data:
        ``grad_rates`` (N, T) is ``dL/d(rates)``; one adjoint solve on the GPU (``SiteHandle.vjp``, include/acn_qp.h) gives, in
        the reference's units (rates in A, energy in kWh) and with ``f`` the MINIMISED objective as in ``dual_values``:

          * ``"q"``: (N, T) ``dL/dq``, q the linear cost of ``f`` per ampere (objective weights and tariffs enter through it);
          * ``"energy_demands"``: {session_id: ``dL/d(remaining demand)`` per kWh} (0 for a session whose row is slack);
          * ``"infrastructure_limits"``: {constraint id: ``dL/d(limit)``, summed over the periods the limit binds in};
          * ``"peak_limit"``: (T,) ``dL/d(peak limit of period t)`` (only when the solve had a peak limit);
          * ``"rate_bounds"``: {"lb": (N, T), "ub": (N, T)}, non-zero where the rate sits on that bound;
          * ``"info"``: dict(verdict, rows, weak, free, solve_residual, stationarity) of ``backend.VjpResult``.  ``weak``
            counts constraints that are active with a zero multiplier: there the schedule has a kink and the gradient is
            that of the active set as found.  A verdict other than 0 comes with zero gradients.

        Raises ``ValueError`` with the reason for a problem the adjoint kernels do not serve (more than 64 EVSEs, horizons
        beyond 32 -- beyond 288 with ``solver_options={"vjp_long": True}``, which also asks for a site with at least one
        constraint --, more than four sessions per EVSE, load-flattening or demand-charge terms)."""
        res, batch = self.last_result, self.last_batch
        if res is None or getattr(self, "_last_handle", None) is None:
            raise RuntimeError("schedule_gradients: no solve yet")
        from . import backend

        if int(res.status[b]) not in backend.ACCEPTED_STATUSES:
            raise InfeasibilityException(f"problem {b} ended with status {backend.STATUS_NAMES.get(int(res.status[b]), res.status[b])}: no gradients")
        table, infrastructure, site = self._last_table, self._last_infrastructure, batch.site
        T, M = int(batch.T[b]), site.M
        g = np.asarray(grad_rates, float)
        if g.ndim != 2 or g.shape[0] != batch.N or g.shape[1] < T:
            raise ValueError(f"grad_rates must have shape ({batch.N}, {T})")
        gx = np.zeros((1, batch.N, batch.Tm))
        gx[0, :, :T] = g[:, :T]
        one = slice(b, b + 1)
        point = backend.BatchResult(res.x[one], res.status[one], res.iters[one], res.pri_res[one], res.dua_res[one], res.obj[one], y=res.y[one])
        v = self._last_handle.vjp(batch.subset(one), point, gx, options=self._last_options)
        out = {"q": v.q[0][:, :T].copy(), "energy_demands": {}, "infrastructure_limits": {},
               "rate_bounds": {"lb": v.lb[0][:, :T].copy(), "ub": v.ub[0][:, :T].copy()}}
        for k in np.flatnonzero(table.prob == b):
            i, sid = int(table.evse[k]), table.session_ids[k] if table.session_ids is not None else int(k)
            slot = np.flatnonzero((batch.s_len[b, :, i] > 0) & (batch.s_off[b, :, i] == table.off[k]))
            k_i = infrastructure.voltages[i] * self.interface.period / 1e3 / 60
            out["energy_demands"][sid] = float(v.cap[0, slot[0], i]) / k_i if table.rem[k] > 0 and slot.size else 0.0
        for j in range(M):
            out["infrastructure_limits"][infrastructure.constraint_ids[j]] = float(v.rows[0, j].sum())
        if site.has_peak and np.isfinite(batch.peak[b][:T]).any():
            out["peak_limit"] = v.rows[0, M][:T].copy()
        out["info"] = dict(verdict=int(v.info[0, 0]), rows=int(v.info[0, 1]), weak=int(v.info[0, 2]), free=int(v.info[0, 3]),
                           solve_residual=float(v.res[0, 0]), stationarity=float(v.res[0, 1]))
        return out

    @property
    def last_multipliers(self):
        """(B, Mg, Tm) site-row multipliers of the last solve: the ``y0`` of a later warm start."""
        return None if self.last_result is None else self.last_result.y

    def solve_batch(
        self,
        session_lists: Sequence[Sequence],
        infrastructure,
        peak_limits: Optional[Sequence] = None,
        prev_peak=0,
        verbose: bool = False,
        _defaults: Optional[dict] = None,
        warm_start: Optional[Sequence] = None,
    ):
        """Batched extension (not in the reference): one independent MPC
        problem per entry of ``session_lists`` (state snapshots, sites' days,
        demand scenarios), all solved in one kernel launch.  Returns
        ``(list of (N, T_b) arrays, status (B,) int32)``; never raises for
        solver outcomes -- inspect ``status``."""
        from . import backend
        from .builder import build_batch

        if self.constraint_type not in ("SOC", "LINEAR"):
            from .builder import _bad_constraint_type

            _bad_constraint_type(self.constraint_type)
        B = len(session_lists)
        nonempty = [k for k, sl in enumerate(session_lists) if len(sl) > 0]
        rates = [np.zeros((infrastructure.num_stations, 1)) for _ in range(B)]
        status = np.full(B, backend.STATUS_SOLVED, dtype=np.int32)
        if not nonempty:
            return rates, status
        pl = [None] * B if peak_limits is None else list(peak_limits)
        from .session_table import SessionTable

        table = SessionTable.from_sessions([session_lists[k] for k in nonempty], infrastructure)
        ws = None if warm_start is None else [warm_start[k] for k in nonempty]
        res, batch = self.solve_table(table, infrastructure, [pl[k] for k in nonempty], prev_peak, _defaults, ws)
        if verbose:
            for j, k in enumerate(nonempty):
                print(
                    f"[acnqp] problem {k}: status={backend.STATUS_NAMES.get(int(res.status[j]))} "
                    f"iters={int(res.iters[j])} pri_res={res.pri_res[j]:.3e} dua_res={res.dua_res[j]:.3e} "
                    f"obj={-(res.obj[j] + batch.const[j]):.9g} (maximised) kernel_ms={res.kernel_ms:.3f}"
                )
        for j, k in enumerate(nonempty):
            rates[k] = res.x[j, :, : int(batch.T[j])].copy()
            status[k] = res.status[j]
        warn_inaccurate(res.status, res.pri_res, res.dua_res)
        return rates, status
