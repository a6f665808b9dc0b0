"""adacharge_amd: MI355X-native batched MPC solver behind adacharge's API.

Package root re-exports the same names as the reference's
``adacharge/__init__.py`` (star-imports of adacharge, postprocessing and
adaptive_charging_optimization).
"""
from .adaptive_charging_optimization import (  # noqa: F401
    AdaptiveChargingOptimization,
    InfeasibilityException,
    ObjectiveComponent,
    QuadObjective,
    Rates,
    demand_charge,
    equal_share,
    load_flattening,
    peak,
    quick_charge,
    total_energy,
    tou_energy_cost,
)
from .adacharge import (  # noqa: F401
    AdaptiveChargingAlgorithmOffline,
    AdaptiveSchedulingAlgorithm,
    get_active_sessions,
)
from .postprocessing import (  # noqa: F401
    ceil_to_set,
    diff_based_reallocation,
    floor_to_set,
    increment_in_set,
    index_based_reallocation,
    project_into_continuous_feasible_pilots,
    project_into_discrete_feasible_pilots,
)
from .utils import infrastructure_constraints_feasible  # noqa: F401
from .acn import SimpleRampdown  # noqa: F401  (the estimator estimate_max_rate=True reads; acnportal is not a dependency)

__version__ = "0.1.0"


def __getattr__(name):
    """``solve_qp`` (adacharge_amd/diff.py: the batched QP as a differentiable torch operation) on first use: torch is
    plumbing here and is not imported with the package."""
    if name == "solve_qp":
        from .diff import solve_qp

        return solve_qp
    if name == "simulate_prices":   # the closed-loop rollout as a differentiable operation of the tariff, likewise
        from .diff import simulate_prices

        return simulate_prices
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
