"""Closed-loop rollout of a batch of MPC scenarios with the state resident in HBM.

Every user of the reference runs it in a closed loop: each period the loop solves, sends the first-period pilots to the
chargers, integrates the delivered energy and builds the next problem.  ``simulate`` runs that loop for B scenarios of one
site on one stream -- ``acnqp_solve_batch_device -> acnqp_pilots_device -> acnqp_advance_device`` per period, no host
synchronisation in between -- and copies pilots, statuses and flags back once at the end.
With a stated ``session_order`` the loop also serves the two settings of the reference that read the session list,
``uninterrupted_charging`` and ``reallocate``: ``acnqp_prepare_device`` runs between the advance and the solve.
With ``resolve="events"`` the loop is the one around the reference's ``schedule()``: a scenario is solved afresh only where
``FleetTable.resolve_rows(max_recompute)`` says so -- step 0, plug-in and unplug events, every ``max_recompute`` periods --
and keeps the schedule it holds in between: ``acnqp_select_device -> solve -> acnqp_hold_device`` in place of the solve.

``simulate(..., keep_tape=True)`` keeps every step's state on the device and ``rollout_gradients`` runs the backward sweep
through the whole loop: per step ``acnqp_advance_vjp_device`` (the adjoint of "time passes") and ``acnqp_vjp_device`` (the
adjoint of the solve), for the gradients of a scalar of the applied pilots with respect to the tariff, the requested
energies and the site rows' limits.

``FleetTable`` is everything the loop needs that does not depend on what the solver answers, computed once for the whole
run: the arrival records of every step (the layout of ``acnqp_advance_plan``), the linear cost and the scalars of every
horizon 1 .. Tm (``builder.objective_terms``), and the peak-limit series.  This is online MPC as in the reference's closed
loop: an EV becomes visible at its arrival step, so every EVSE carries one session at a time (K = 1).
"""
from __future__ import annotations

import copy
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence

import numpy as np

from . import backend
from .builder import _objective_needs_flat, _objective_needs_max, objective_terms


START_GAIN = 1e5   # where a cold solve starts a session: Proj(-1e5 q) (kStartGain of the solver kernels, acn_qp_common.hpp)
RESOLVE_MODES = ("every_step", "events")


@dataclass
class RolloutResult:
    pilots: np.ndarray      # (steps, B, N) what went to the chargers
    status: np.ndarray      # (steps, B) int32
    iters: np.ndarray       # (steps, B) int32
    flags: np.ndarray       # (steps, B) int32: flags of the advance that built the step's problems (0 = nothing refused)
    delivered: List[np.ndarray]   # per scenario: kWh delivered to each EV of the fleet, in the fleet's order
    x: Optional[np.ndarray] = None   # (steps, B, N, Tm) the solved schedules, when asked for
    visits: Optional[np.ndarray] = None          # (steps, B) int32 visits of the reallocation's round robin (reallocate=True)
    prepare_flags: Optional[np.ndarray] = None   # (steps, B) int32 flags of acnqp_prepare_device (a session_order was stated)
    energy_cost: Optional[np.ndarray] = None     # (B,) sum over s, i of pilots[s, b, i] * weight[i] * series[b][s]; None without a clock cost
    actual: Optional[np.ndarray] = None          # (steps, B, N) what the EVs drew of the pilots (a fleet carries batteries); then
                                                 # ``delivered`` and ``energy_cost`` are computed from it, not from ``pilots``
    plant_flags: Optional[np.ndarray] = None     # (steps, B) int32 flags of acnqp_plant_device (a fleet carries batteries)
    estimates: Optional[np.ndarray] = None       # (steps, B, N) the bound each solve saw (estimate_max_rate), +inf where no session
    estimate_flags: Optional[np.ndarray] = None  # (steps, B) int32 flags of acnqp_estimate_device (estimate_max_rate)
    solved: Optional[np.ndarray] = None          # (steps, B) bool: the scenario was solved afresh at the step (resolve="events"); where
                                                 # False, ``status`` is that of the solve the step's pilots came from and ``iters`` is 0
    resolve_flags: Optional[np.ndarray] = None   # (steps, B) int32: per scenario, the flags of acnqp_hold_device OR-ed with those of
                                                 # acnqp_select_device for its row of the step's dense batch (resolve="events")
    tape: Optional["RolloutTape"] = None         # what ``rollout_gradients`` reads (keep_tape=True)


@dataclass
class RolloutTape:
    """What the backward sweep of a rollout reads, all of it on the device and none of it copied: the forward loop wrote
    these tensors and the tape only keeps them alive."""
    handle: Any
    table: "FleetTable"
    plan: Any            # the AdvancePlan on the device, as the forward advances took it
    max_pilot: Any       # (N,) of the continuous pilot rule
    options: Any
    states: list         # steps DeviceBatches: problem, x, y and status of every step
    start: Any           # the empty DeviceBatch the run started from (step -1)
    pilots: Any          # (steps, B, N) as the pilot kernel wrote them
    flags: Any           # (steps, B) int32 of the advance that built each step's problems


@dataclass
class RolloutGradients:
    """``rollout_gradients``: float64 tensors on the rollout's device unless stated."""
    prices: Any          # (B, P) dL/d(price series) through the problems' linear cost; None without a clock cost
    limits: Any          # (B, M) dL/d(limit of a site row), summed over steps and periods
    info: Any            # (steps, B, 4) int32 of every step's acnqp_vjp_device (verdict 0: done)
    res: Any             # (steps, B, 2)
    garr: Any            # (A,) dL/d(a_cap) of the plan's arrival records, in A-periods
    table: Any = None

    @property
    def requested(self) -> List[np.ndarray]:
        """per scenario, dL/d(requested kWh) of every record of its fleet in the fleet's order; 0 for a record the table
        never admitted.  Reads ``garr``, so it waits for the device."""
        t = self.table
        g = self.garr.cpu().numpy()
        out = [np.zeros(len(f)) for f in t.fleets]
        order = sorted(range(len(t._stays)), key=lambda j: (t._stays[j][2], t._stays[j][0]))   # the plan's record order (stable)
        for r, j in enumerate(order):
            b, i, _, _, n, _ = t._stays[j]
            out[b][n] = g[r] / t.kwh_per_amp_period[i]
        return out


class FleetTable:
    """The EV records of B scenarios of one site, and what a rollout of ``steps`` periods from ``start_time`` precomputes
    from them.  ``fleets[b]`` is a sequence of records (dicts) with ``station``, ``arrival``, ``departure`` (periods),
    ``requested`` (kWh) and optionally ``min_rate`` / ``max_rate``: a scalar, or one value per period of the stay.
    ``enforce_pilot_limit`` (time-invariant) is applied to the records here.  The objective must not depend on the clock
    (one linear cost per horizon serves the whole run).  That is checked by evaluating the cost one period later on an
    interface that keeps its clock in ``interface.data["current_time"]`` (this package's ``Interface``; the entry is put
    back); behind any other interface only this package's clock-free components (quick_charge, equal_share, total_energy,
    load_flattening, peak, demand_charge) are accepted.  Either way any other cost that reads the clock is refused.
    The one clock-dependent cost the loop carries is ``tou_energy_cost``: the components whose function ``is
    tou_energy_cost`` are taken out of the list before the table is built and become the plan's CLOCK COST (rule 6b of
    include/acn_qp.h) -- ``coef`` the component's coefficient, ``weight[i] = voltages[i] / 1e3 * (period / 60)`` as
    ``tou_energy_cost`` computes it, ``series = interface.get_prices(steps + Tm, start_time)`` for every scenario, or the
    caller's ``prices``: a ``(P,)`` or ``(B, P)`` array whose entry 0 is the price of period ``start_time``, so that one batch
    sweeps tariffs over its scenarios.  At most one such component with a non-zero coefficient is accepted.  The advance
    then builds ``q' = q_table[row] + coef * (weight * price)``, three roundings.  The builder folds ``coefficient *
    term.lin`` in list order and negates the sum, and negation is exact, so with ``tou_energy_cost`` as the LAST component
    of the list the device's q' is the builder's q bit for bit; anywhere else in the list the builder's sum is folded in
    another order and the two may differ in the last places.  The caller's list is never reordered.
    An ``external_signal`` of ``load_flattening`` is the caller's fixed array: it is read from its first entry
    at every step, as ``schedule`` reads it.
    ``session_order`` states the order of the session lists a plant would hand to ``schedule`` -- what the reference's
    minimum-rate walk and reallocation read, and the slot state does not carry: ``"fleet"`` (a session stands where its record
    stands in its fleet), ``"arrival"`` (plug-in order: the rank of (arrival, fleet index), with the EV's true arrival also
    when it lies before ``start_time``) or None.  ``order_keys`` (steps, B, N) int32 then holds, for every step and EVSE, the
    position of the record whose stay covers that step (the ``key`` of ``acnqp_prepare_plan``); None without an order.
    A record may carry ``battery``: a dict with ``capacity`` and ``init_charge`` (kWh), ``max_power`` (kW) and optionally
    ``transition_soc`` (absent or None: an ideal battery; a fraction strictly inside (0, 1): the two-stage battery, whose
    accepted rate falls in proportion to the room left once the state of charge has passed it).  ``has_plant`` says whether
    any record does; ``plant_plan`` is then the battery table and the plug-in rows of ``acnqp_plant_device`` (include/acn_qp.h,
    "the plant"): one table row per admitted record -- a record without ``battery`` gets the "no battery model" row -- and
    ``plug`` (steps, B, N) int32, the record's row at the step it becomes visible, -1 elsewhere.  None without a battery.
    ``fresh_rows()`` marks the same steps for ``acnqp_estimate_device`` ("the ramp-down estimator"), battery or not."""

    ORDERS = ("fleet", "arrival")

    def __init__(self, fleets: Sequence[Sequence[dict]], infrastructure, interface, objective, steps: int, start_time: int = 0,
                 peak_limit=None, done_kwh: float = 1e-9, t_max: Optional[int] = None, session_order: Optional[str] = None,
                 prices=None):
        if session_order is not None and session_order not in self.ORDERS:
            raise ValueError(f'session_order must be "fleet", "arrival" or None, not {session_order!r}')
        self.session_order = session_order
        self.min_pilot = np.ascontiguousarray(infrastructure.min_pilot, float)[: infrastructure.num_stations].copy()
        self.fleets = [list(f) for f in fleets]
        self.objective, self.peak_limit = objective, peak_limit   # (simulate checks them against the algorithm's)
        self.B, self.N = len(self.fleets), infrastructure.num_stations
        self.steps, self.start = int(steps), int(start_time)
        if self.B < 1 or self.steps < 1:
            raise ValueError("a rollout needs at least one scenario and one step")
        volt = np.asarray(infrastructure.voltages, float)
        self.kwh_per_amp_period = volt * interface.period / 1e3 / 60          # aco.py:114
        if np.any(volt != volt[0]):
            raise ValueError("the rollout's demand-charge floor and done tolerance assume one voltage for the whole site")
        self.kw_per_amp = float(volt[0] / 1000.0)
        self.done_tol = float(done_kwh / self.kwh_per_amp_period[0])
        max_pilot = np.asarray(infrastructure.max_pilot, float)
        index = {s: i for i, s in enumerate(infrastructure.station_ids)}
        recs = []   # (visible step, scenario, evse, len, cap, min rates, max rates)
        rows = []   # the battery table: (t_room, t_amps, t_knee, t_slope) of every record admitted, in the order of _stays
        self.has_plant = any(ev.get("battery") is not None for fleet in self.fleets for ev in fleet)
        self._stays = []   # (scenario, evse, first step, end step, fleet index, arrival) of every record admitted
        self.windows = []   # per scenario: (evse, first step, end step) of every EV, relative to start (clipped to the run)
        longest = 1
        for b, fleet in enumerate(self.fleets):
            wins, busy = [], {}
            for n, ev in enumerate(fleet):
                i = index[ev["station"]]
                arr, dep = int(ev["arrival"]), int(ev["departure"])
                tv = max(arr, self.start)
                ln = dep - tv
                wins.append((i, tv - self.start, dep - self.start))
                row = self._battery_row(ev.get("battery"), b, n, ev, volt[i], self.kwh_per_amp_period[i])
                cap = float(ev["requested"]) / self.kwh_per_amp_period[i]
                if ln <= 0 or tv >= self.start + self.steps or cap <= self.done_tol:
                    continue
                for lo, hi in busy.get(i, ()):
                    if tv < hi and lo < dep:
                        raise ValueError(f"scenario {b}: two stays on EVSE {ev['station']} overlap; online MPC carries one session per EVSE")
                busy.setdefault(i, []).append((tv, dep))
                rates = []
                for key, default in (("min_rate", 0.0), ("max_rate", np.inf)):
                    r = ev.get(key, default)
                    r = np.full(ln, float(r)) if np.isscalar(r) else np.asarray(r, float)[tv - arr: dep - arr]
                    if len(r) != ln:
                        raise ValueError(f"{key} of an EV needs one value per period of its stay")
                    rates.append(r)
                rates[1] = np.minimum(rates[1], max_pilot[i])                 # enforce_pilot_limit (ada.py:141)
                if not np.all(np.isfinite(rates[1])):
                    raise ValueError("max_rate must be finite (the site gives no max_pilot for this EVSE)")
                recs.append((tv - self.start, b, i, ln, cap, rates[0], rates[1]))
                self._stays.append((b, i, tv - self.start, dep - self.start, n, arr))
                rows.append(row)
                longest = max(longest, ln)
            self.windows.append(wins)
        self.order_keys = None if session_order is None else self.keys_for(session_order)
        self.plant_plan = None
        if self.has_plant:
            plug = np.full((self.steps, self.B, self.N), -1, np.int32)
            for r, (b, i, lo, _, _, _) in enumerate(self._stays):
                plug[lo, b, i] = r
            t = np.array(rows, np.float64).reshape(len(rows), 4)
            self.plant_plan = backend.PlantPlan(*(np.ascontiguousarray(t[:, k]) for k in range(4)), plug)
        self.Tm = int(t_max) if t_max is not None else longest
        if self.Tm < longest:
            raise ValueError(f"t_max = {self.Tm} is shorter than the longest stay ({longest} periods)")
        self.K = 1
        recs.sort(key=lambda r: (r[0], r[1]))                                 # stable: record order inside (step, scenario)
        A = len(recs)
        key = np.array([r[0] * self.B + r[1] for r in recs], dtype=np.int64)
        seg = np.searchsorted(key, np.arange(self.steps * self.B + 1)).astype(np.int32)
        a_seg = np.empty((self.steps, self.B + 1), np.int32)                  # row s: the arrivals visible at step s, absolute
        for s in range(self.steps):
            a_seg[s] = seg[s * self.B: (s + 1) * self.B + 1]
        lens = np.array([r[3] for r in recs], dtype=np.int32)
        rate_seg = np.zeros(A + 1, np.int32)
        np.cumsum(lens, out=rate_seg[1:])
        cat = lambda k: np.concatenate([r[k] for r in recs]) if recs else np.zeros(0)
        # ---- the objective, once per horizon (aco.py:200-218 depends on a problem only through T, aco.py:243-245) ----------
        self.prev_peak = interface.get_prev_peak()
        Tm, N = self.Tm, self.N
        rest, clock = self._split_clock_cost(objective)
        q_table, h_scal = np.zeros((Tm, N, Tm)), np.zeros((Tm, 3))
        dfloor = 0.0
        for T in range(1, Tm + 1):
            q, pd, lf, _, dc, dfl = objective_terms(rest, infrastructure, interface, N, T, self.prev_peak)
            q_table[T - 1, :, :T] = q
            h_scal[T - 1] = pd, lf, dc
            dfloor = dfl
        self._refuse_clock_dependence(rest, infrastructure, interface, q_table[Tm - 1])
        # ---- the clock cost (rule 6b): the tariff over the run, one row per scenario ---------------------------------------
        self.c_coef = self.c_weight = self.c_series = None
        if clock is None and prices is not None:
            raise ValueError("prices= is given but the objective has no tou_energy_cost component with a non-zero coefficient")
        if clock is not None:
            need = self.steps + Tm
            one = np.asarray(interface.get_prices(need, self.start) if prices is None else prices, float)
            if one.ndim not in (1, 2) or (one.ndim == 2 and one.shape[0] != self.B):
                raise ValueError(f"prices must have shape (P,) or ({self.B}, P)")
            if one.shape[-1] < need:
                raise ValueError(f"the price series holds {one.shape[-1]} periods from start_time; the rollout needs steps + t_max = {need}")
            if not np.all(np.isfinite(one[..., :need])):
                raise ValueError("the price series must be finite")
            self.c_coef = float(clock.coefficient)
            self.c_weight = np.asarray(infrastructure.voltages, float) / 1e3 * (interface.period / 60)   # as tou_energy_cost computes it
            self.c_series = np.array(np.broadcast_to(one[..., :need], (self.B, need)), dtype=np.float64, order="C")   # (a copy: writable)
        self.dfloor0 = float(dfloor)
        self.need_flat, self.need_max = _objective_needs_flat(objective), _objective_needs_max(objective)
        h_row = np.r_[-1, np.arange(Tm)].astype(np.int32)
        # ---- the peak limit as a series over the run (ada.py:160-167: a scalar passes through, a vector is read from the clock)
        self.has_peak = peak_limit is not None
        series = None
        if self.has_peak:
            P = self.steps + Tm
            if np.isscalar(peak_limit):
                one = np.full(P, float(peak_limit))
            else:
                pl = np.asarray(peak_limit, float)[self.start: self.start + P]
                one = np.full(P, np.inf)
                one[: len(pl)] = pl
            series = np.ascontiguousarray(np.broadcast_to(one, (self.B, P)))
        self.plan = backend.AdvancePlan(
            q_table=q_table, h_scal=h_scal, h_row=h_row, done_tol=self.done_tol, kw_per_amp=self.kw_per_amp, peak_series=series,
            a_seg=a_seg, a_evse=np.array([r[2] for r in recs], np.int32), a_slot=np.zeros(A, np.int32), a_len=lens,
            a_cap=np.array([r[4] for r in recs], np.float64), a_rate_seg=rate_seg, a_min=cat(5), a_max=cat(6),
            c_coef=self.c_coef, c_weight=self.c_weight, c_series=self.c_series)

    NO_BATTERY = (np.inf, np.inf, 0.0, 0.0)   # the table row "no battery model": the EV draws what it is offered

    @classmethod
    def _battery_row(cls, bat, b, n, ev, voltage, kwh_per_amp_period):
        """(t_room, t_amps, t_knee, t_slope) of a record's ``battery`` in the units of the slot state (A, A-periods): the
        division of the tail's slope is done here, once; the device multiplies.  Every battery is validated, admitted or not."""
        if bat is None:
            return cls.NO_BATTERY
        who = f"scenario {b}, EV {n} ({ev.get('sid', ev['station'])}): battery"
        try:
            cap, init, power = (float(bat[k]) for k in ("capacity", "init_charge", "max_power"))
        except (KeyError, TypeError, ValueError) as exc:
            raise ValueError(f"{who} needs numbers capacity, init_charge (kWh) and max_power (kW)") from exc
        soc = bat.get("transition_soc")
        if not (np.isfinite(cap) and cap > 0):
            raise ValueError(f"{who}: capacity must be finite and > 0, not {cap!r}")
        if not 0 <= init <= cap:
            raise ValueError(f"{who}: init_charge must lie in [0, capacity], not {init!r}")
        if not (np.isfinite(power) and power > 0):
            raise ValueError(f"{who}: max_power must be finite and > 0, not {power!r}")
        if soc is not None and not 0 < float(soc) < 1:
            raise ValueError(f"{who}: transition_soc must lie strictly inside (0, 1) or be None, not {soc!r}")
        t_room = max(cap - init, 0.0) / kwh_per_amp_period
        t_amps = power * 1000 / voltage
        t_knee = (1 - float(soc)) * cap / kwh_per_amp_period if soc is not None else 0.0
        return (t_room, t_amps, t_knee, t_amps / t_knee if t_knee > 0 else 0.0)

    @staticmethod
    def _split_clock_cost(objective):
        """(the components that build q_table / h_scal, the one tou_energy_cost component or None)"""
        from .adaptive_charging_optimization import tou_energy_cost

        rest = [c for c in objective if c.function is not tou_energy_cost]
        clock = [c for c in objective if c.function is tou_energy_cost and c.coefficient != 0]
        if len(clock) > 1:
            raise ValueError(f"the objective holds {len(clock)} tou_energy_cost components with a non-zero coefficient: the rollout "
                             "carries one clock cost (one coefficient, one price series); add their coefficients up")
        if clock and not np.isfinite(clock[0].coefficient):
            raise ValueError("the coefficient of tou_energy_cost must be finite")
        return rest, (clock[0] if clock else None)

    def energy_cost(self, pilots: np.ndarray) -> Optional[np.ndarray]:
        """(B,) what the applied ``pilots`` (steps, B, N) cost under the clock cost's series: sum over s, i of
        pilots[s, b, i] * weight[i] * series[b][s] (kWh times price); None without a clock cost."""
        if self.c_series is None:
            return None
        return np.einsum("sbi,i,bs->b", pilots, self.c_weight, self.c_series[:, : pilots.shape[0]])

    def keys_for(self, session_order: str) -> np.ndarray:
        """(steps, B, N) int32: at step s, the list position under ``session_order`` of the record staying on EVSE i of
        scenario b (stays on one EVSE never overlap); 0 where no record stays."""
        if session_order not in self.ORDERS:
            raise ValueError(f'session_order must be "fleet" or "arrival", not {session_order!r}')
        keys = np.zeros((self.steps, self.B, self.N), np.int32)
        pos = {}
        if session_order == "arrival":
            for b in range(self.B):
                mine = sorted((arr, n) for bb, _, _, _, n, arr in self._stays if bb == b)
                pos.update({(b, n): r for r, (_, n) in enumerate(mine)})
        for b, i, lo, hi, n, _ in self._stays:
            keys[max(lo, 0): min(hi, self.steps), b, i] = n if session_order == "fleet" else pos[b, n]
        return keys

    def fresh_rows(self) -> np.ndarray:
        """(steps, B, N) int32: 1 at the step an admitted record becomes visible on its EVSE -- a session the estimator of
        ``estimate_max_rate`` sees for the first time -- 0 elsewhere.  Built on demand: only such a rollout reads it."""
        fresh = np.zeros((self.steps, self.B, self.N), np.int32)
        for b, i, lo, _, _, _ in self._stays:
            fresh[lo, b, i] = 1
        return fresh

    def resolve_rows(self, max_recompute=None) -> np.ndarray:
        """(steps, B) bool: the steps at which scenario b is solved afresh under ``resolve="events"`` -- the loop around the
        reference's ``schedule()`` as SURVEY.md section 3.1 records it: the plant calls the algorithm when an EV plugs in, when
        one unplugs, or when ``max_recompute`` periods have passed since the last solve, and plays the schedule it holds in
        between.  Scenario b resolves at step s when
          E0     s == 0
          E1/E2  s is the first step or the end step of any record of fleet b (``windows``, inside the run), admitted or not:
                 the plant raises plug-in and unplug events for every EV
          E3     ``max_recompute`` is not None and s - (the last step b resolved) >= max_recompute
        Everything here is known before the run: the mask never depends on what the solver answers."""
        if max_recompute is not None:
            if isinstance(max_recompute, (bool, np.bool_)) or not isinstance(max_recompute, (int, np.integer)) or max_recompute < 1:
                raise ValueError(f"max_recompute must be None or an integer >= 1, not {max_recompute!r}")
        mask = np.zeros((self.steps, self.B), dtype=bool)
        mask[0] = True
        for b, wins in enumerate(self.windows):
            for _, lo, hi in wins:
                for s in (lo, hi):
                    if 0 <= s < self.steps:
                        mask[s, b] = True
        if max_recompute is not None:
            last = np.zeros(self.B, dtype=np.int64)
            for s in range(1, self.steps):
                mask[s] |= s - last >= int(max_recompute)
                last[mask[s]] = s
        return mask

    def resolve_plan(self, max_recompute=None) -> "backend.ResolvePlan":
        """the ``backend.ResolvePlan`` of ``resolve_rows(max_recompute)``: per step the scenarios that resolve, ascending,
        and for every scenario its row in that step's dense batch, or -1"""
        mask = self.resolve_rows(max_recompute)
        steps, b = np.nonzero(mask)   # (row-major: ascending b inside a step)
        sel_seg = np.zeros(self.steps + 1, np.int32)
        np.cumsum(mask.sum(axis=1), out=sel_seg[1:])
        pos = np.full((self.steps, self.B), -1, np.int32)
        pos[steps, b] = np.arange(len(b)) - sel_seg[steps]
        return backend.ResolvePlan(sel_seg=sel_seg, sel_idx=b.astype(np.int32), pos=pos)

    def _refuse_clock_dependence(self, objective, infrastructure, interface, q_now):
        data = getattr(interface, "data", None)
        if not isinstance(data, dict):   # no clock to move: only components known not to read one
            from . import adaptive_charging_optimization as aco

            safe = (aco.quick_charge, aco.equal_share, aco.total_energy, aco.load_flattening, aco.peak, aco.demand_charge)
            unknown = [getattr(c.function, "__name__", repr(c.function)) for c in objective if c.function not in safe]
            if unknown:
                raise ValueError(f"cannot tell whether the objective components {unknown} read the clock (the interface keeps no "
                                 "data['current_time'] to move): the rollout keeps one linear cost per horizon")
            return
        had, old = "current_time" in data, data.get("current_time")
        try:
            data["current_time"] = (old or 0) + 1
            q_later = objective_terms(objective, infrastructure, interface, self.N, self.Tm, self.prev_peak)[0]
        finally:
            if had:
                data["current_time"] = old
            else:
                del data["current_time"]
        if not np.array_equal(q_later, q_now[:, : self.Tm]):
            raise ValueError("the objective depends on the clock (e.g. tou_energy_cost): the rollout keeps one linear cost per horizon")

    def delivered(self, pilots: np.ndarray) -> List[np.ndarray]:
        """kWh delivered to every EV by the applied ``pilots`` (steps, B, N): what the plant integrates, capped at the request."""
        out = []
        for b, fleet in enumerate(self.fleets):
            d = np.zeros(len(fleet))
            for n, (ev, (i, lo, hi)) in enumerate(zip(fleet, self.windows[b])):
                lo, hi = max(lo, 0), min(hi, self.steps)
                if hi > lo:
                    d[n] = min(float(ev["requested"]), float(pilots[lo:hi, b, i].sum()) * self.kwh_per_amp_period[i])
            out.append(d)
        return out


def simulate(alg, fleets, steps: int, start_time: int = 0, warm_start: bool = False, return_schedules: bool = False,
             observer=None, session_order: Optional[str] = None, prices=None, resolve: str = "every_step",
             keep_tape: bool = False) -> RolloutResult:
    """``AdaptiveSchedulingAlgorithm.simulate_batch``: see there.
    ``keep_tape=True`` keeps what ``rollout_gradients`` needs in ``RolloutResult.tape``: instead of ping-ponging two
    ``DeviceBatch``es the loop writes every step's problems into a batch of their own (with the site-row multipliers y),
    and the tape holds these ``steps`` batches and the empty one the run starts from, the handle, the plan, the options and
    ``flags``.  Nothing is copied and nothing is launched beyond what the forward launches.  The tape holds
    ``(steps + 1) * B * (32 N Tm + 8 Mg Tm + 16 K N + 8 Tm [peak row] + 69)`` bytes of states (lb, ub, q, x; y; the slot
    tables; peak; the scalars and result fields) beside the ``steps * B * (8 N + 12)`` of pilots, status and flags every
    rollout holds.  Served with a tape: ``resolve="every_step"`` (or an events run that solves every step), continuous
    pilots, no battery, no estimator, no ``session_order`` step, and a site the vjp kernels serve (N <= 64, no
    load-flattening or demand-charge row, t_max <= 32, or <= 288 with ``solver_options={"vjp_long": True}``); anything else
    raises ``ValueError`` before anything is launched."""
    if resolve not in RESOLVE_MODES:
        raise ValueError(f'resolve must be "every_step" or "events", not {resolve!r}')
    import torch

    from .adaptive_charging_optimization import _site_handle
    from .postprocessing import pilot_plan_arrays

    from .acn import SimpleRampdown

    for on, why in ((alg.reallocate, "reallocate=True: the round robin breaks ties by session-list order, which the slot state does not carry"),
                    (alg.uninterrupted_charging, "uninterrupted_charging: per-step pre-processing that reads the evolving state")):
        if on and session_order is None:
            raise ValueError(f"simulate_batch does not serve {why}")
    # the estimator of what each battery accepts: the one whose arithmetic the device does (acnqp_estimate_device)
    ramp = alg.max_rate_estimator if alg.estimate_max_rate else None
    if alg.estimate_max_rate and not isinstance(ramp, SimpleRampdown):
        raise ValueError("simulate_batch serves estimate_max_rate with max_rate_estimator=SimpleRampdown(...) only (its rules run on the "
                         f"device; any other estimator is Python code per step), not {type(ramp).__name__}")
    if session_order is not None and session_order not in FleetTable.ORDERS:
        raise ValueError(f'session_order must be "fleet", "arrival" or None, not {session_order!r}')
    if alg.constraint_type not in ("SOC", "LINEAR"):
        from .builder import _bad_constraint_type

        _bad_constraint_type(alg.constraint_type)
    interface = alg.interface
    infra = interface.infrastructure_info()
    if isinstance(fleets, FleetTable) and prices is not None:
        raise ValueError("prices= goes to the FleetTable: the table given was built with its own")
    table = fleets if isinstance(fleets, FleetTable) else FleetTable(fleets, infra, interface, alg.objective, steps, start_time, alg.peak_limit,
                                                                            session_order=session_order, prices=prices)
    if (table.steps, table.start) != (int(steps), int(start_time)):
        raise ValueError("the FleetTable was built for another run (steps, start_time)")
    if table.session_order != session_order:
        raise ValueError(f"the FleetTable was built with session_order={table.session_order!r}, the call states {session_order!r}")
    same_objective = len(table.objective) == len(alg.objective) and all(a is b or a == b for a, b in zip(table.objective, alg.objective))
    same_peak = (table.peak_limit is None) == (alg.peak_limit is None) and (
        table.peak_limit is None or np.array_equal(np.asarray(table.peak_limit, float), np.asarray(alg.peak_limit, float)))
    if not same_objective or not same_peak:
        raise ValueError("the FleetTable was built with another objective or peak_limit than the algorithm's")
    # who is solved afresh at which step: known before the run (arrivals, departures, max_recompute), never read off an answer
    rplan = counts = None
    if resolve == "events":
        mask = table.resolve_rows(alg.max_recompute)
        if not mask.all():
            for on, why in ((alg.estimate_max_rate, "estimate_max_rate: the reference's estimator runs inside schedule(), so only at solves, while "
                                                    "the device rule moves every step; under a held schedule it needs a rule of its own"),
                            (alg.uninterrupted_charging, "uninterrupted_charging: its minimum-rate step is per solve, a held schedule has none")):
                if on:
                    raise ValueError(f'simulate_batch(resolve="events") does not serve {why} (max_recompute=1 solves every step)')
            rplan = table.resolve_plan(alg.max_recompute)
            counts = rplan.counts()
            table_seg = np.asarray(rplan.sel_seg)
            host_idx = np.asarray(rplan.sel_idx)
    if keep_tape:
        _refuse_tape(alg, table, session_order, rplan)
    opts = dict(alg.solver_options or {})
    site, handle = _site_handle(infra, alg.constraint_type, table.has_peak, alg.device, with_flat=table.need_flat, with_max=table.need_max,
                                polish_long=bool(opts.pop("polish_long", False)), polish_wide=bool(opts.pop("polish_wide", False)),
                                vjp_long=bool(opts.pop("vjp_long", False)))
    if not bool(opts.pop("retry_stalled", True)):
        opts["retry_passes"] = 0
    options = backend.default_options(**opts)
    dev = torch.device("cuda", handle.device)
    B, N, Tm, K = table.B, table.N, table.Tm, table.K
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        plan = table.plan.to_device(dev)
        plan.warm_arrival_gain = START_GAIN if warm_start else 0.0
        mode = "discrete" if alg.quantize else "continuous"
        pplan = pilot_plan_arrays(None, infra, interface, mode, batch=B, t_max=Tm).to_device(dev)
        # the two settings that read the session list: its order comes from the caller, as one key per (step, scenario, EVSE)
        min_rates, realloc = bool(alg.uninterrupted_charging), bool(alg.reallocate)
        prep = min_rates or realloc
        view = [None, None, None]
        visits = pflags = None
        if session_order is not None:
            pflags = torch.zeros((steps, B), dtype=torch.int32, device=dev)
        if prep:
            cm = infra.constraint_matrix
            has_rows = cm is not None and np.size(cm) > 0
            ph = np.deg2rad(infra.phases)
            # (the reference's minimum-rate step returns the list sorted by arrival, stable: plug-in order whichever was stated)
            keys = table.keys_for("arrival") if min_rates else table.order_keys
            prplan = backend.PreparePlan(key=keys, cre=np.ascontiguousarray(cm * np.cos(ph)) if has_rows else None,
                                         cim=np.ascontiguousarray(cm * np.sin(ph)) if has_rows else None,
                                         limits=np.ascontiguousarray(infra.constraint_limits, float) if has_rows else None,
                                         min_pilot=table.min_pilot if min_rates else None).to_device(dev)
        if realloc:
            view = [torch.zeros((B, N), dtype=dt, device=dev) for dt in (torch.int32, torch.uint8, torch.float64)]
            visits = torch.zeros((steps, B), dtype=torch.int32, device=dev)
            pplan.mode = backend.PILOTS_REALLOCATE
            pplan.cre, pplan.cim, pplan.limits = prplan.cre, prplan.cim, prplan.limits
            pplan.sess_seg = (torch.arange(B + 1, dtype=torch.int32) * N).to(dev)   # every problem's view holds N entries
            pplan.s_evse, pplan.s_arrived, pplan.s_cap = (v.view(B * N) for v in view)

        def prepare(state, row):
            if prep:
                handle.prepare_device(state, prplan, pflags[row], *view, min_rates=min_rates, key_row=row, stream=stream)
        s_eq = 1 if alg.enforce_energy_equality else 0
        want_y = warm_start and site.Mg > 0
        # two states that ping-pong; with a tape, one per step and behind them the empty one the run starts from
        bufs = [backend.DeviceBatch.empty(site, B, Tm, K, dev, want_y=want_y or keep_tape, s_eq=s_eq, dfloor=table.dfloor0)
                for _ in range(steps + 1 if keep_tape else 2)]
        pilots = torch.zeros((steps, B, N), dtype=torch.float64, device=dev)
        status = torch.zeros((steps, B), dtype=torch.int32, device=dev)
        iters = torch.zeros((steps, B), dtype=torch.int32, device=dev)
        flags = torch.zeros((steps, B), dtype=torch.int32, device=dev)
        xs = torch.zeros((steps, B, N, Tm), dtype=torch.float64, device=dev) if return_schedules else None
        held = rplan is not None   # some scenario of some step keeps the schedule it holds: the advance's warm_x' is that schedule
        wx = torch.zeros((B, N, Tm), dtype=torch.float64, device=dev) if want_y or held else None
        wy = torch.zeros((B, site.Mg, Tm), dtype=torch.float64, device=dev) if want_y else None
        if held:
            rplan = rplan.to_device(dev)
            dense = backend.DeviceBatch.empty(site, B, Tm, K, dev, want_y=want_y, s_eq=s_eq, dfloor=table.dfloor0)
            heads = {m: dense.head(m) for m in set(counts)}
            dwx = torch.zeros((B, N, Tm), dtype=torch.float64, device=dev) if want_y else None
            dwy = torch.zeros((B, site.Mg, Tm), dtype=torch.float64, device=dev) if want_y else None
            solved = torch.ones((steps, B), dtype=torch.uint8, device=dev)
            sflags = torch.zeros((steps, B), dtype=torch.int32, device=dev)   # row s: entry j is the j-th scenario step s resolves
            hflags = torch.zeros((steps, B), dtype=torch.int32, device=dev)
        nothing = torch.zeros((B, N), dtype=torch.float64, device=dev)
        # a battery per EV (the plant): what is drawn of the pilots goes to the advance, not the pilots themselves
        actual = plflags = None
        if table.has_plant:
            plplan = table.plant_plan.to_device(dev)
            bat = torch.full((B, N), -1, dtype=torch.int32, device=dev)
            room = torch.zeros((B, N), dtype=torch.float64, device=dev)
            actual = torch.zeros((steps, B, N), dtype=torch.float64, device=dev)
            plflags = torch.zeros((steps, B), dtype=torch.int32, device=dev)
        # an estimate per EV of what it accepts (estimate_max_rate): the solve, the prepare entry and the plant see a VIEW of the
        # state whose ub is capped with it; the state keeps the session's own bounds, which the advance shifts
        est = eflags = ests = None
        if ramp is not None:
            fresh = torch.from_numpy(table.fresh_rows()).to(dev)
            est = torch.full((B, N), float("inf"), dtype=torch.float64, device=dev)
            ests = torch.zeros((steps, B, N), dtype=torch.float64, device=dev)
            eflags = torch.zeros((steps, B), dtype=torch.int32, device=dev)
            capped = torch.zeros((B, N, Tm), dtype=torch.float64, device=dev)   # (one: everything is on one stream)

        def estimate(state, row):
            """the state the step's solve reads: ``state`` itself, or its view under the estimate moved on by step ``row - 1``"""
            if ramp is None:
                return state
            past = row > 0
            handle.estimate_device(state, fresh, est, capped, eflags[row], pilots=pilots[row - 1] if past else None,
                                   actual=actual[row - 1] if past and actual is not None else None, status=status[row - 1] if past else None,
                                   up_threshold=ramp.up_threshold, down_threshold=ramp.down_threshold, up_increment=ramp.up_increment,
                                   fresh_row=row, stream=stream)
            ests[row].copy_(est)
            view = copy.copy(state)
            view.own_ub, view.ub = state.ub, capped
            return view
        # the first period's problems: time "passes" on an empty state, its arrivals are admitted
        handle.advance_device(bufs[-1], bufs[0], nothing, plan, -1, flags[0], use_status=False, stream=stream, seg_row=0)
        solve_next = estimate(bufs[0], 0)
        prepare(solve_next, 0)
        for s in range(steps):
            state, nxt = bufs[s % len(bufs)], bufs[(s + 1) % len(bufs)]
            cur = solve_next
            warm = want_y and s > 0   # (a site without rows has no multipliers to carry: it starts cold)
            if held and counts[s] < B:
                # only the scenarios with an event are solved: out of the state into a dense batch, and the answers back beside
                # the held, shifted schedules of everyone else (every size is the plan's: nothing is read off the device)
                m, lo = counts[s], int(table_seg[s])
                part = heads[m]
                if m > 0:
                    handle.select_device(cur, part, rplan.sel_idx[lo: lo + m], sflags[s], m, warm_x=wx if warm else None,
                                         warm_y=wy if warm else None, out_warm_x=dwx if warm else None, out_warm_y=dwy if warm else None,
                                         stream=stream)
                    handle.solve_device(part, options, stream=stream, warm_x=dwx[:m] if warm else None, warm_y=dwy[:m] if warm else None)
                handle.hold_device(cur, part, rplan.pos[s], m, wx, status[s - 1], solved[s], hflags[s], held_y=wy if want_y else None,
                                   stream=stream)
            else:
                handle.solve_device(cur, options, stream=stream, warm_x=wx if warm else None, warm_y=wy if warm else None)
            handle.pilots_device(pplan, cur.x, first=pilots[s], visits=visits[s] if realloc else None, stream=stream)
            if actual is not None:
                handle.plant_device(cur, plplan, pilots[s], bat, room, actual[s], plflags[s], status=cur.status, plug_row=s, stream=stream)
            status[s].copy_(cur.status)
            iters[s].copy_(cur.iters)
            if xs is not None:
                xs[s].copy_(cur.x)
            if observer is not None:
                observer(s, cur, pilots[s])
            if s + 1 < steps:
                handle.advance_device(state, nxt, pilots[s] if actual is None else actual[s], plan, s, flags[s + 1], use_status=True, warm_x=wx,
                                      warm_y=wy, stream=stream, seg_row=s + 1)
                solve_next = estimate(nxt, s + 1)
                prepare(solve_next, s + 1)
        torch.cuda.synchronize(dev)
        p = pilots.cpu().numpy()
        st = status.cpu().numpy()
        p[~np.isin(st, backend.ACCEPTED_STATUSES)] = 0.0   # what the advance delivered for a step that did not solve: nothing
        vis = None if visits is None else visits.cpu().numpy()
        if vis is not None and (vis < 0).any():
            s_bad, b_bad = (int(v[0]) for v in np.nonzero(vis < 0))
            raise ValueError(f"step {s_bad}, scenario {b_bad}: allowable pilots end below a session's cap; the reallocation of the "
                             "rounding loss would never end")
        drawn = p if actual is None else actual.cpu().numpy()   # (the plant draws nothing in a step that did not solve)
        was_solved = rflags = None
        if resolve == "events":
            was_solved, rflags = np.ones((steps, B), dtype=bool), np.zeros((steps, B), np.int32)
        if held:
            was_solved, rflags, sf = solved.cpu().numpy().astype(bool), hflags.cpu().numpy(), sflags.cpu().numpy()
            for s in np.flatnonzero(np.asarray(counts) < B):
                rows = host_idx[table_seg[s]: table_seg[s + 1]]
                rflags[s, rows] |= sf[s, : len(rows)]
        return RolloutResult(p, st, iters.cpu().numpy(), flags.cpu().numpy(), table.delivered(drawn),
                             None if xs is None else xs.cpu().numpy(), vis, None if pflags is None else pflags.cpu().numpy(),
                             table.energy_cost(drawn), None if actual is None else drawn, None if plflags is None else plflags.cpu().numpy(),
                             None if ests is None else ests.cpu().numpy(), None if eflags is None else eflags.cpu().numpy(),
                             was_solved, rflags,
                             RolloutTape(handle, table, plan, pplan.max_pilot, options, bufs[:steps], bufs[-1], pilots, flags) if keep_tape else None)


def _refuse_tape(alg, table: FleetTable, session_order, rplan) -> None:
    """what ``keep_tape=True`` does not serve, each with its reason"""
    why = None
    if alg.quantize:
        why = "quantize: a quantised pilot is piecewise constant in the schedule, there is no gradient to carry"
    elif table.has_plant:
        why = "a battery: the plant between the pilots and the advance has no adjoint"
    elif alg.estimate_max_rate:
        why = "estimate_max_rate: the estimator's state has no adjoint"
    elif rplan is not None:
        why = 'resolve="events" with a held step: a held schedule has no adjoint (max_recompute=1 solves every step)'
    elif session_order is not None:
        why = "a stated session_order: the prepare step between the advance and the solve has no adjoint"
    elif table.need_flat or table.need_max:
        why = "load_flattening / demand_charge: the gradients through the solve serve no site with a flat or max row"
    elif table.N > 64:
        why = f"a site of {table.N} EVSEs: the gradients through the solve serve at most 64"
    else:
        long = bool((alg.solver_options or {}).get("vjp_long", False))
        if table.Tm > (288 if long else 32):
            why = (f"t_max = {table.Tm}: the gradients through the solve serve horizons up to 32, and up to 288 with "
                   'solver_options={"vjp_long": True}')
    if why:
        raise ValueError(f"simulate_batch(keep_tape=True) does not serve {why}")


def rollout_gradients(result: RolloutResult, grad_pilots) -> RolloutGradients:
    """The gradients of a scalar L of the applied pilots of a rollout run with ``keep_tape=True``: ``grad_pilots`` (steps, B, N)
    = dL/d(pilots), a numpy array or a tensor on the rollout's device.  The backward sweep visits the steps from the last
    to the first; per step ``acnqp_advance_vjp_device`` (the adjoint of the advance that followed the step, the clip of
    the pilot rule included) and ``acnqp_vjp_device`` (the adjoint of the step's solve), then one last call of the former
    for the advance that built the first problems -- ``2 steps + 1`` launches on the current stream and no host
    synchronisation.  Returns ``RolloutGradients``: ``prices`` (B, P), ``requested`` (per scenario, one value per fleet record,
    in L per kWh), ``limits`` (B, M), and every step's ``info`` and ``res``.
    These are the gradients THROUGH the loop.  A loss that reads a parameter also directly keeps that term for the caller:
    the energy cost of ``FleetTable.energy_cost`` is ``sum pilots * weight * price``, so with ``w = table.c_weight`` and
    ``p = table.c_series[:, :steps]``

        g = rollout_gradients(result, np.einsum("i,bs->sbi", w, p))          # d cost / d pilots
        dcost_dprice = g.prices.cpu().numpy(); dcost_dprice[:, :steps] += np.einsum("sbi,i->bs", result.pilots, w)

    Steps whose solve was not accepted, or whose working set is beyond the vjp kernel's tables, pass no gradient
    (``info[s, b, 0] != 0``)."""
    import torch

    tape = result.tape
    if tape is None:
        raise ValueError("rollout_gradients needs a rollout run with keep_tape=True")
    handle, table, plan = tape.handle, tape.table, tape.plan
    steps, B, N = tape.pilots.shape
    Tm, K = table.Tm, table.K
    dev = tape.pilots.device
    M = handle.site.M
    nrow = M + (1 if handle.site.has_peak else 0)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        gd = torch.as_tensor(grad_pilots, dtype=torch.float64, device=dev).contiguous()
        if tuple(gd.shape) != (steps, B, N):
            raise ValueError(f"grad_pilots must have shape {(steps, B, N)}")
        f8 = dict(dtype=torch.float64, device=dev)
        gx, gq = torch.empty((B, N, Tm), **f8), torch.empty((B, N, Tm), **f8)
        gcap, grow = torch.empty((B, K, N), **f8), torch.empty((B, nrow, Tm), **f8)
        carry = [torch.empty((B, K, N), **f8) for _ in range(2)]
        info, res = torch.zeros((steps, B, 4), dtype=torch.int32, device=dev), torch.zeros((steps, B, 2), **f8)
        garr = torch.zeros(plan._len("a_evse"), **f8)
        gprice = None if plan.c_series is None else torch.zeros(tuple(plan.c_series.shape), **f8)
        limits = torch.zeros((B, M), **f8)
        nxt = {}   # the adjoints of the state one step later: nothing behind the last step
        for s in range(steps - 1, -2, -1):
            cur = tape.states[s] if s >= 0 else tape.start
            at = s >= 0
            handle.advance_vjp_device(cur, plan, s, carry[s % 2], applied=tape.pilots[s] if at else None, max_pilot=tape.max_pilot if at else None,
                                      gdir=gd[s] if at else None, gx=gx if at else None, garr=garr, gprice=gprice, stream=stream,
                                      seg_row=s + 1 if s + 1 < steps else None, **nxt)
            if not at:
                break
            handle.vjp_device(cur, gx, gq, gcap, grow, info[s], res[s], options=tape.options, stream=stream)
            if M:
                limits.add_(grow[:, :M].sum(dim=2))
            nxt = dict(gq_next=gq, gcap_vjp_next=gcap, gcap_carry_next=carry[s % 2], horizon_next=cur.horizon, flags_next=tape.flags[s])
    return RolloutGradients(gprice, limits, info, res, garr, table)
