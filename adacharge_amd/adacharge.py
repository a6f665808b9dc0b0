"""Algorithm adapters -- mirror of /root/reference/adacharge/adacharge.py.

``AdaptiveSchedulingAlgorithm`` keeps the acnportal ``BaseAlgorithm`` plugin
contract (constructor kwargs ada.py:43-58, ``register_interface`` ada.py:116-133,
``schedule(active_sessions) -> {station_id: ndarray}`` ada.py:135-193); the body
is re-pointed at the HIP backend through ``AdaptiveChargingOptimization``.
"""
from __future__ import annotations

import warnings
from copy import deepcopy

import numpy as np

from .acn import (
    BaseAlgorithm,
    SessionInfo,
    apply_minimum_charging_rate,
    apply_upper_bound_estimate,
    enforce_pilot_limit,
)
from .adaptive_charging_optimization import *  # noqa: F401,F403  (ada.py:5 star-import)
from .adaptive_charging_optimization import AdaptiveChargingOptimization
from .postprocessing import (
    diff_based_reallocation,
    index_based_reallocation,
    project_into_continuous_feasible_pilots,
    project_into_discrete_feasible_pilots,
)


def get_active_sessions(active_evs, current_time):
    """ada.py:18-39: SessionInfo list for acnsim EV objects."""
    return [
        SessionInfo(
            ev.station_id, ev.session_id, ev.requested_energy, ev.energy_delivered,
            ev.arrival, ev.departure, current_time=current_time,
        )
        for ev in active_evs
    ]


class AdaptiveSchedulingAlgorithm(BaseAlgorithm):
    """Model Predictive Control based scheduling algorithm (ada.py:42-193)."""

    def __init__(
        self,
        objective,
        constraint_type="SOC",
        enforce_energy_equality=False,
        solver=None,
        peak_limit=None,
        estimate_max_rate=False,
        max_rate_estimator=None,
        uninterrupted_charging=False,
        quantize=False,
        reallocate=False,
        max_recompute=None,
        allow_overcharging=False,
        verbose=False,
        solver_options=None,
        device=0,
        warm_start=False,
    ):
        super().__init__()
        self.objective = objective
        self.constraint_type = constraint_type
        self.enforce_energy_equality = enforce_energy_equality
        self.solver = solver
        self.peak_limit = peak_limit
        # extension (off by default: the reference rebuilds everything each step and keeps no state, ada.py:152-158):
        # start each solve from the previous step's schedule and multipliers, shifted by the periods elapsed
        self.warm_start = warm_start
        self._warm = None   # (current_time, x (N, T), y (N, T)) of the previous solve
        self.estimate_max_rate = estimate_max_rate
        self.max_rate_estimator = max_rate_estimator
        self.uninterrupted_charging = uninterrupted_charging
        self.quantize = quantize
        self.reallocate = reallocate
        self.verbose = verbose
        self.solver_options = solver_options
        self.device = device
        if not self.quantize and self.reallocate:
            raise ValueError(
                "reallocate cannot be true without quantize. "
                "Otherwise there is nothing to reallocate :)."
            )
        if self.quantize:
            # ada.py:106-111 reads the BaseAlgorithm default before assigning (Appendix D.1)
            if self.max_recompute is not None:
                warnings.warn("Overriding max_recompute to 1 since quantization is on.")
            self.max_recompute = 1
        else:
            self.max_recompute = max_recompute
        self.allow_overcharging = allow_overcharging

    def register_interface(self, interface):
        """ada.py:116-133."""
        self._interface = interface
        if self.max_rate_estimator is not None:
            self.max_rate_estimator.register_interface(interface)

    def _preprocess(self, active_sessions, infrastructure):
        """ada.py:141-150."""
        active_sessions = enforce_pilot_limit(active_sessions, infrastructure)
        if self.estimate_max_rate:
            active_sessions = apply_upper_bound_estimate(self.max_rate_estimator, active_sessions)
        if self.uninterrupted_charging:
            active_sessions = apply_minimum_charging_rate(
                active_sessions, infrastructure, self.interface.period
            )
        return active_sessions

    def _trimmed_peak(self, active_sessions):
        """ada.py:160-167: scalar passes through, vector is sliced from the
        current simulation time."""
        if self.peak_limit is None or np.isscalar(self.peak_limit):
            return self.peak_limit
        t = self.interface.current_time
        horizon = max(s.arrival_offset + s.remaining_time for s in active_sessions)
        return self.peak_limit[t : t + horizon]

    def _postprocess(self, rates_matrix, active_sessions, infrastructure):
        """ada.py:176-189."""
        if self.quantize:
            if self.reallocate:
                rates_matrix = diff_based_reallocation(
                    rates_matrix, active_sessions, infrastructure, self.interface
                )
            else:
                rates_matrix = project_into_discrete_feasible_pilots(rates_matrix, infrastructure)
        else:
            rates_matrix = project_into_continuous_feasible_pilots(rates_matrix, infrastructure)
        return np.maximum(rates_matrix, 0)

    def _optimizer(self):
        return AdaptiveChargingOptimization(
            self.objective, self.interface, self.constraint_type, self.enforce_energy_equality,
            solver=self.solver, solver_options=self.solver_options, device=self.device,
        )

    def schedule(self, active_sessions):
        """See BaseAlgorithm (ada.py:135-193)."""
        if len(active_sessions) == 0:
            return {}
        infrastructure = self.interface.infrastructure_info()
        active_sessions = self._preprocess(active_sessions, infrastructure)
        optimizer = self._optimizer()
        warm = None
        if self.warm_start and self._warm is not None:
            t_prev, x_prev, y_prev = self._warm
            dt = self.interface.current_time - t_prev
            if 0 <= dt < x_prev.shape[1]:
                warm = (x_prev[:, dt:], y_prev[:, dt:])
        rates_matrix = optimizer.solve(
            active_sessions, infrastructure,
            peak_limit=self._trimmed_peak(active_sessions),
            prev_peak=self.interface.get_prev_peak(),
            verbose=self.verbose,
            warm_start=warm,
        )
        if self.warm_start:
            T = rates_matrix.shape[1]
            self._warm = (self.interface.current_time, rates_matrix.copy(), optimizer.last_multipliers[0][:, :T].copy())
        self.last_iterations = int(optimizer.last_result.iters[0])
        rates_matrix = self._postprocess(rates_matrix, active_sessions, infrastructure)
        return {
            station_id: rates_matrix[i, :] for i, station_id in enumerate(infrastructure.station_ids)
        }

    def schedule_batch(self, session_lists, peak_limits=None, as_arrays=False, postprocess="host", first_period_only=False):
        """Batched extension: one schedule per state snapshot, every optimisation problem solved by one pipelined
        pass of the HIP library, and the steps either side of the solve -- the pre-processing of ada.py:141-150 and
        the post-processing of ada.py:176-189 -- done as array operations over the whole batch
        (session_table.py, postprocessing.*_batch).  ``session_lists``: a list of SessionInfo lists, or a
        ``SessionTable`` (no Python objects at all).  Returns one ``{station_id: ndarray}`` dict per snapshot
        (``{}`` for an empty one, ``None`` where the solve did not end optimal), or, with ``as_arrays=True``,
        ``(rates (B, N, Tmax), status (B,))``.
        ``postprocess="device"``: the three branches of ada.py:176-189 run on the GPU (``acnqp_pilots_device``) on the
        copy of the schedules the solve also leaves in HBM (``acnqp_results.x_dev``; the solve still returns ``x`` to the
        host as before), and the post-processing copies back only the pilots -- the bits of tests/pilots_spec.py, which
        are the host path's wherever no decision of the reallocation sits within a rounding of its threshold.  A snapshot
        whose round robin would never end (the reference's does not return on it) raises ``ValueError``.
        ``first_period_only``: return -- and, on the device path, copy -- the first control period only: ``(B, N)``
        arrays, or dicts of one-element arrays."""
        from . import session_table as st
        from .postprocessing import (
            diff_based_reallocation_batch,
            project_into_continuous_feasible_pilots_batch,
            project_into_discrete_feasible_pilots_batch,
        )

        infrastructure = self.interface.infrastructure_info()
        if isinstance(session_lists, st.SessionTable):
            table, B, nonempty, lists = session_lists, session_lists.B, np.arange(session_lists.B), None
        else:
            B = len(session_lists)
            nonempty = np.array([k for k, sl in enumerate(session_lists) if len(sl) > 0], dtype=np.int64)
            lists = [session_lists[k] for k in nonempty]
            table = st.SessionTable.from_sessions(lists, infrastructure) if len(nonempty) else None
        status = np.full(B, 1, dtype=np.int32)
        if table is None:
            return (np.zeros((B, infrastructure.num_stations, 1)), status) if as_arrays else [{} for _ in range(B)]
        table = st.enforce_pilot_limit(table, infrastructure)                       # ada.py:141
        if self.estimate_max_rate:                                                  # ada.py:143-146
            if lists is None:
                raise ValueError("estimate_max_rate needs SessionInfo lists (the estimator API takes sessions)")
            table = st.apply_upper_bound_estimate(table, [self.max_rate_estimator.get_maximum_rates(sl) for sl in lists])
        if self.uninterrupted_charging:                                             # ada.py:147-150
            table = st.apply_minimum_charging_rate(table, infrastructure, self.interface.period)
        if peak_limits is None:                                                     # ada.py:160-167
            if self.peak_limit is None or np.isscalar(self.peak_limit):
                pl = [self.peak_limit] * table.B
            else:
                end = np.zeros(table.B, dtype=np.int64)
                np.maximum.at(end, table.prob, table.off + table.rem)
                t = self.interface.current_time
                pl = [self.peak_limit[t : t + int(e)] for e in end]
        else:
            pl = [peak_limits[k] for k in nonempty]
        if postprocess not in ("host", "device"):
            raise ValueError('postprocess must be "host" or "device"')
        on_device = postprocess == "device"
        res, batch = self._optimizer().solve_table(table, infrastructure, pl, self.interface.get_prev_peak(), keep_on_device=on_device)
        from .adaptive_charging_optimization import warn_inaccurate

        warn_inaccurate(res.status, res.pri_res, res.dua_res)   # cvxpy's "Solution may be inaccurate" (aco.py:315-321)
        if on_device:
            from .postprocessing import postprocess_batch_device, raise_if_endless

            mode = ("reallocate" if self.reallocate else "discrete") if self.quantize else "continuous"
            r, visits = postprocess_batch_device(res.x_dev, table, infrastructure, self.interface, mode, res.handle,
                                                 first_period_only=first_period_only)
            raise_if_endless(visits, table, infrastructure, self.interface, names=nonempty)
            res.x_dev = None
            if first_period_only:
                r = r[:, :, None]
        elif self.quantize:                                                         # ada.py:176-184
            if self.reallocate:
                r = diff_based_reallocation_batch(res.x, table, infrastructure, self.interface)
            else:
                r = project_into_discrete_feasible_pilots_batch(res.x, infrastructure)
        else:                                                                       # ada.py:185-188
            r = project_into_continuous_feasible_pilots_batch(res.x, infrastructure)
        r = np.maximum(r, 0)                                                        # ada.py:189
        if first_period_only:
            r = r[:, :, :1]
        if as_arrays:
            rates = np.zeros((B,) + r.shape[1:])
            rates[nonempty] = r
            status[nonempty] = res.status
            return (rates[:, :, 0] if first_period_only else rates), status
        out = [{} for _ in range(B)]
        ids = infrastructure.station_ids
        for j, k in enumerate(nonempty):
            if res.status[j] not in (1, 5):   # OPTIMAL / OPTIMAL_INACCURATE, as aco.py:319
                out[k] = None
            else:
                rj = r[j, :, : 1 if first_period_only else int(batch.T[j])]
                out[k] = {sid: rj[i] for i, sid in enumerate(ids)}
        return out

    def simulate_batch(self, fleets, steps, start_time=0, warm_start=False, return_schedules=False, observer=None, session_order=None,
                       prices=None, resolve="every_step", keep_tape=False):
        """Closed-loop extension: ``steps`` control periods of B scenarios of this site (``fleets``: one list of EV records
        per scenario, or a ``rollout.FleetTable``) with the whole state resident in HBM.  On one stream, per period:
        ``solve_device -> pilots_device (first period) -> advance_device``, with no host synchronisation inside the loop; an
        EV becomes visible at its arrival step (online MPC, one session per EVSE).  Returns a ``rollout.RolloutResult``:
        ``pilots (steps, B, N)``, ``status``, ``iters`` and ``flags (steps, B)`` and the energy delivered to every EV, copied
        back once at the end.  Serves continuous pilots and ``quantize=True``; ``reallocate`` and
        ``uninterrupted_charging`` raise ``ValueError`` -- unless the caller states the order of the session lists a plant
        would hand to ``schedule``, which those steps of the reference read and the device state does not carry:
        ``session_order="fleet"`` (a session stands where its record stands in its fleet) or ``"arrival"`` (plug-in order).
        Then ``uninterrupted_charging`` and ``reallocate`` are served (``acnqp_prepare_device`` between the advance and the
        solve; the result carries ``visits`` and ``prepare_flags``).
        ``estimate_max_rate=True`` is served when ``max_rate_estimator`` is a ``SimpleRampdown`` (``adacharge_amd.SimpleRampdown``:
        its rules run on the device, ``acnqp_estimate_device`` between the advance and the prepare step; it is per session and
        needs no ``session_order``): each solve sees every session's bounds capped with the estimate of what its EV accepts,
        moved on by what the EV drew of its last pilot, while the state keeps the session's own bounds.  The result carries
        ``estimates (steps, B, N)`` -- the bound each solve saw, +inf where no session -- and ``estimate_flags (steps, B)``;
        ``observer`` then receives a view of the state whose ``ub`` is the capped copy and whose ``own_ub`` is the state's.
        With any other estimator, or none, ``estimate_max_rate`` raises ``ValueError``.
        One objective that reads the clock is served: ``tou_energy_cost`` (at most one component; keep it LAST in the list and
        every problem of the loop is the builder's bit for bit, ``rollout.FleetTable``).  The advance prices each new problem
        from ``interface.get_prices(steps + t_max, start_time)``, or from ``prices`` -- ``(P,)`` or ``(B, P)``, entry 0 the price
        of period ``start_time``, one tariff per scenario (with a ``FleetTable`` the table's own ``prices`` hold) -- and the result
        carries ``energy_cost (B,)``.  Every other objective that reads the clock raises ``ValueError``.
        A record may carry ``battery``: ``dict(capacity=kWh, init_charge=kWh, max_power=kW, transition_soc=None or a fraction
        inside (0, 1))`` -- the battery decides what the EV DRAWS of its pilot (``acnqp_plant_device`` between the pilots and
        the advance: a current limit, the room left to full and, past ``transition_soc``, a rate that falls with that room).
        The advance, the demand-charge floor, ``delivered`` and ``energy_cost`` then follow what was drawn, and the result
        carries ``actual (steps, B, N)`` and ``plant_flags (steps, B)``.  A rollout whose fleets carry no battery launches
        and returns exactly what it did without the feature; so does one without the estimator.
        ``warm_start``: every solve but the first starts from the previous
        period's schedule and multipliers, shifted on the device.  ``observer(step, state, pilots)``: diagnostic hook called
        after each period's solve has been enqueued (it may synchronise and read the ``DeviceBatch``).
        ``resolve``: ``"every_step"`` (the default) solves every scenario at every period and ignores ``max_recompute``.
        ``"events"`` is the loop around the reference's ``schedule()`` and honours ``max_recompute``: a
        scenario is solved afresh at step 0, at the steps an EV of its fleet plugs in or unplugs, and once ``max_recompute``
        periods have passed since its last solve (``rollout.FleetTable.resolve_rows``); in between it plays the rest of the
        schedule it holds -- the last solve's, shifted by the advance and clipped into the current bounds, NOT the schedule a
        fresh solve would give once a battery has drawn less than it was offered or the tariff has moved.  Only the scenarios
        with an event are solved (``acnqp_select_device -> solve -> acnqp_hold_device`` in place of the step's solve); the mask
        is known before the run, so the loop still never synchronises.  The result carries ``solved (steps, B)`` bool (None
        under ``"every_step"``) and ``resolve_flags``; ``status`` of a held step is the status of the solve its pilots came
        from -- a scenario whose last solve was not accepted is delivered nothing until its next scheduled solve -- and
        ``iters`` of a held step is 0.  ``quantize`` sets ``max_recompute = 1``: then, as with ``max_recompute=1`` itself, every
        step is solved and the run is the ``"every_step"`` run.  Whenever some step is not solved, ``estimate_max_rate`` and
        ``uninterrupted_charging`` raise ``ValueError``: both are per solve in the reference and have no rule under a held
        schedule here.
        ``keep_tape=True`` keeps every step's state on the device in ``RolloutResult.tape`` so that
        ``rollout.rollout_gradients(result, grad_pilots)`` can run the backward sweep through the whole loop -- gradients of a
        scalar of the applied pilots with respect to the tariff, the requested energies and the site limits
        (``rollout.simulate`` says what it holds and what it serves: continuous pilots, every step solved, no battery,
        estimator or ``session_order``, a site the vjp kernels serve; anything else raises ``ValueError``).  Off, nothing
        changes."""
        from .rollout import simulate

        return simulate(self, fleets, steps, start_time, warm_start, return_schedules, observer, session_order, prices, resolve, keep_tape)


class AdaptiveChargingAlgorithmOffline(BaseAlgorithm):
    """Offline optimisation with perfect future information (ada.py:196-294)."""

    def __init__(
        self,
        objective,
        constraint_type="SOC",
        enforce_energy_equality=False,
        solver=None,
        peak_limit=None,
        verbose=False,
        solver_options=None,
        device=0,
    ):
        super().__init__()
        self.max_recompute = 1
        self.objective = objective
        self.constraint_type = constraint_type
        self.enforce_energy_equality = enforce_energy_equality
        self.solver = solver
        self.peak_limit = peak_limit
        self.verbose = verbose
        self.solver_options = solver_options
        self.device = device
        self.sessions = None
        self.session_ids = None
        self.internal_schedule = None

    def register_events(self, events):
        """ada.py:234-247: only Plugin events are considered."""
        active_evs = [deepcopy(event[1].ev) for event in events.queue if event[1].event_type == "Plugin"]
        self.sessions = get_active_sessions(active_evs, 0)
        self.session_ids = set(s.session_id for s in self.sessions)

    def solve(self):
        """ada.py:249-276."""
        if self._interface is None:
            raise ValueError(
                "Error: self.interface is None. Please register interface before calling solve."
            )
        if self.sessions is None:
            raise ValueError(
                "No events registered. Please register an event queue before calling solve."
            )
        infrastructure = self.interface.infrastructure_info()
        self.sessions = enforce_pilot_limit(self.sessions, infrastructure)
        optimizer = AdaptiveChargingOptimization(
            self.objective, self.interface, self.constraint_type, self.enforce_energy_equality,
            solver=self.solver, solver_options=self.solver_options, device=self.device,
        )
        rates_matrix = optimizer.solve(self.sessions, infrastructure, self.peak_limit, verbose=self.verbose)
        rates_matrix = project_into_continuous_feasible_pilots(rates_matrix, infrastructure)
        self.internal_schedule = {
            station_id: rates_matrix[i, :] for i, station_id in enumerate(infrastructure.station_ids)
        }

    def schedule(self, active_evs):
        """ada.py:278-294."""
        if self.internal_schedule is None:
            raise ValueError(
                "No internal schedule found. Make sure to call solve before calling schedule or "
                "running a simulation."
            )
        for ev in active_evs:
            if ev.session_id not in self.session_ids:
                raise ValueError(f"Error: Session {ev.session_id} not included in offline solve.")
        current_time = self.interface.current_time
        return {ev.station_id: [self.internal_schedule[ev.station_id][current_time]] for ev in active_evs}
