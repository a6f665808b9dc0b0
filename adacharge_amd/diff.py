"""The batched QP as a differentiable torch operation: ``solve_qp`` solves on the GPU (``SiteHandle.solve_device``) and its
backward is ONE adjoint launch (``SiteHandle.vjp_device``, adacharge_amd/csrc/acn_qp_vjp.hpp, acn_qp_vjp_long.hpp) -- for learning objective
weights and tariffs against an outcome of the schedule, bilevel pricing, sensitivity studies over scenario batches.

    x = solve_qp(handle, template, q, s_cap, lb, ub)      # (B, N, Tm) float64 on the handle's GPU
    (w * x).sum().backward()                               # q.grad, s_cap.grad, lb.grad, ub.grad

Everything stays on the current stream; neither direction synchronises with the host.  The gradients are those of the
active set at the solver's answer (include/acn_qp.h says how it is taken): accurate where the answer is -- solve with tight
``eps_abs`` / ``eps_rel`` -- and one-sided at a kink.  The limits of the site's rows belong to the handle, not to the
problem: their gradients come from ``SiteHandle.vjp_device`` directly.  Served shapes: N <= 64, K <= 4, no load-flattening
or demand-charge row, and horizons <= 32 on any handle; horizons 33 ... 288 on a ``SiteHandle(site, device, vjp_long=True)``
whose site has at least one row (and at most 48 rows of G).  Another shape raises ValueError in backward, with the reason.

``simulate_prices`` is the same for the CLOSED LOOP: a whole ``simulate_batch`` rollout as one differentiable operation of the
tariff, its backward the sweep of ``rollout.rollout_gradients``.

    pilots = simulate_prices(alg, table, prices)          # (steps, B, N) float64 on the GPU, what went to the chargers
    (w * pilots).sum().backward()                          # prices.grad (B, P)
"""
from __future__ import annotations

import warnings
from typing import Optional

import numpy as np
import torch

from .backend import ACCEPTED_STATUSES, _PROBLEM_ARRAYS, DeviceBatch, Options, SiteHandle, default_options

_last_info = None      # info (B, 4) int32 of the most recent backward, still on the device
_warned = False


class _SolveQP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, handle, template, options, q, s_cap, lb, ub, peak):
        dev = DeviceBatch.__new__(DeviceBatch)
        dev.B, dev.N, dev.Tm, dev.K = template.B, template.N, template.Tm, template.K
        for k in _PROBLEM_ARRAYS:
            setattr(dev, k, getattr(template, k))
        given = dict(q=q, s_cap=s_cap, lb=lb, ub=ub, peak=peak)
        for k, t in given.items():
            if t is None:
                continue
            ref = getattr(template, k)
            if ref is None or t.shape != ref.shape or t.dtype != torch.float64 or t.device != ref.device:
                raise ValueError(f"{k} must be a float64 tensor of shape {None if ref is None else tuple(ref.shape)} on the template's device")
            setattr(dev, k, t.detach().contiguous())
        dev._alloc_results(handle.site.Mg, True, template.lb.device)
        handle.solve_device(dev, options, stream=torch.cuda.current_stream(template.lb.device).cuda_stream)
        ctx.handle, ctx.dev, ctx.options, ctx.has_peak = handle, dev, options, peak is not None
        return dev.x

    @staticmethod
    def backward(ctx, grad_x):
        global _last_info
        handle, dev = ctx.handle, ctx.dev
        B, N, Tm, K = dev.B, dev.N, dev.Tm, dev.K
        M = handle.site.M
        nrow = M + (1 if handle.site.has_peak else 0)
        f8 = dict(dtype=torch.float64, device=dev.x.device)
        gq, glb, gub = (torch.empty((B, N, Tm), **f8) for _ in range(3))
        gcap, grow, res = torch.empty((B, K, N), **f8), torch.empty((B, nrow, Tm), **f8), torch.empty((B, 2), **f8)
        info = torch.empty((B, 4), dtype=torch.int32, device=dev.x.device)
        try:
            handle.vjp_device(dev, grad_x.contiguous(), gq, gcap, grow, info, res, glb=glb, gub=gub, options=ctx.options,
                              stream=torch.cuda.current_stream(dev.x.device).cuda_stream)
        except ValueError as e:
            if 32 < Tm <= 288 and not handle.vjp_long:
                raise ValueError(f"{e}; horizons 33 ... 288 are served on a SiteHandle(site, device, vjp_long=True)") from e
            raise
        _last_info = info
        gpeak = grow[:, M, :].contiguous() if ctx.has_peak and handle.site.has_peak else None
        return None, None, None, gq, gcap, glb, gub, gpeak


def solve_qp(handle: SiteHandle, template: DeviceBatch, q, s_cap, lb, ub, peak=None, options: Optional[Options] = None):
    """The optimal schedules x (B, N, Tm) of the problems of ``template`` (a ``DeviceBatch``: it gives the horizons, the
    session windows, pdiag and s_eq) with its q, s_cap, lb, ub and -- on a site with a peak row -- peak replaced by the given
    float64 device tensors of the same shapes; differentiable in all five."""
    return _SolveQP.apply(handle, template, options if options is not None else default_options(), q, s_cap, lb, ub, peak)


class _SimulatePrices(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alg, table, prices):
        from .rollout import simulate

        if table.c_series is None:
            raise ValueError("simulate_prices needs a FleetTable whose objective has a tou_energy_cost component")
        B, need = table.c_series.shape
        if prices.dim() != 2 or prices.shape[0] != B or prices.shape[1] < need or prices.dtype != torch.float64:
            raise ValueError(f"prices must be a float64 tensor of shape ({B}, P) with P >= steps + t_max = {need}")
        table.c_series[...] = prices.detach()[:, :need].cpu().numpy()   # (the plan reads this array: the table now carries these prices)
        result = simulate(alg, table, table.steps, table.start, keep_tape=True)
        ctx.result, ctx.shape, ctx.where = result, tuple(prices.shape), prices.device
        tape = result.tape
        served = torch.from_numpy(np.isin(result.status, ACCEPTED_STATUSES)).to(tape.pilots.device)[..., None]
        # what the advance saw: a step whose solve was not accepted delivered nothing (RolloutResult.pilots says the same)
        return torch.where(served, tape.pilots, torch.zeros((), dtype=torch.float64, device=tape.pilots.device))

    @staticmethod
    def backward(ctx, grad_pilots):
        global _last_info
        from .rollout import rollout_gradients

        g = rollout_gradients(ctx.result, grad_pilots.contiguous())
        _last_info = g.info.reshape(-1, 4)
        out = torch.zeros(ctx.shape, dtype=torch.float64, device=g.prices.device)
        out[:, : g.prices.shape[1]] = g.prices
        return None, None, out.to(ctx.where)


def simulate_prices(alg, table, prices):
    """The pilots (steps, B, N) of the closed-loop rollout ``alg.simulate_batch(table, table.steps, table.start,
    keep_tape=True)`` under the tariff ``prices`` -- a float64 tensor (B, P), entry 0 the price of the run's first period,
    P >= steps + t_max -- as a float64 tensor on the rollout's GPU, differentiable in ``prices``.  ``table`` is a
    ``rollout.FleetTable`` whose objective holds ``tou_energy_cost``; the prices are written into its series, so the table
    carries them afterwards.  The gradient is the one THROUGH the loop (``rollout.rollout_gradients`` says what a loss
    that also reads the prices directly adds).  What ``keep_tape=True`` does not serve raises ValueError in forward."""
    return _SimulatePrices.apply(alg, table, prices)


def check_last_backward() -> int:
    """How many problems of the most recent backward (of ``simulate_prices``: over all its steps) got no gradient (a verdict other than 0 in ``info``: not solved, or an
    active set beyond the kernel's tables -- their gradients are exact zeros).  Reads ``info``, so it waits for the device:
    call it when convenient, not in the training step's hot path.  Warns the first time the count is not zero."""
    global _warned
    if _last_info is None:
        return 0
    bad = int((_last_info[:, 0] != 0).sum().item())
    if bad and not _warned:
        _warned = True
        warnings.warn(f"solve_qp: {bad} of {_last_info.shape[0]} problems got zero gradients (verdicts {sorted(set(_last_info[:, 0].tolist()) - {0})}: "
                      "1 not solved, 2 active set beyond the kernel's tables, 3 pivot)", RuntimeWarning, stacklevel=2)
    return bad
