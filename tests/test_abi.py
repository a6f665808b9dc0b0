"""The C-ABI library loads, exports every symbol include/acn_qp.h declares and
rejects misuse with return codes -- no compute calls (no GPU here)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from adacharge_amd import backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "acn_qp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(acnqp_[a-z_]+)\s*\(", text)))


def test_header_symbols_all_exported(hip_library):
    syms = declared_symbols()
    assert set(syms) == set(backend.EXPORTED_SYMBOLS)
    for s in syms:
        assert hasattr(hip_library, s), s


def test_abi_v10_version_and_defaults(hip_library):
    assert hip_library.acnqp_abi_version() == 10   # ABI v10: acnqp_route
    o = backend.default_options()
    assert o.precision == 64 and 0 < o.alpha < 2 and o.max_iter > 0 and o.eps_abs > 0
    # ABI v7: stall rule and retry passes are options of the library (every entry point), not of the binding
    assert o.stall_iters == 3000 and o.retry_passes == 2 and o.retry_max_iter == 8000 and o.retry_rho == 0.5
    assert o.inaccurate_floor == 1e-5 and o.polish_iters == 800 and o.polish_stall == 0
    assert C.sizeof(backend.Options) == 120   # sizeof(acnqp_options) as gcc lays the header out
    o2 = backend.default_options(eps_abs=1e-9, max_iter=5)
    assert o2.eps_abs == 1e-9 and o2.max_iter == 5
    assert backend.default_options(polish_stall=100).polish_stall == 100      # ABI v9: the last field of the structure
    # (the header's own layout, polish_stall behind inaccurate_floor included: test_every_struct_and_constant_matches_the_header)
    with pytest.raises(TypeError):
        backend.default_options(nonsense=1)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "acn_qp.h")).read(), flags=re.S)


STRUCTS = {
    "acnqp_site": backend._Site, "acnqp_problems": backend._Problems, "acnqp_results": backend._Results, "acnqp_options": backend.Options,
    "acnqp_table": backend._Table, "acnqp_duals": backend._Duals, "acnqp_pilot_plan": backend._PilotPlan, "acnqp_pilots": backend._Pilots,
    "acnqp_advance_plan": backend._AdvancePlan, "acnqp_next": backend._Next, "acnqp_clock_cost": backend.ClockCost,
    "acnqp_prepare_plan": backend._PreparePlan, "acnqp_prepare_view": backend._PrepareView,
}


def test_every_struct_and_constant_matches_the_header(tmp_path):
    """The header, laid out by gcc, against the binding: size of every struct, offset and size of every field, the value of
    every constant.  The program is generated from the binding's own ``_fields_``, so a field the header does not have
    fails the compile; a struct the header has and ``STRUCTS`` lacks fails the count."""
    text = _header()
    assert sorted(re.findall(r"typedef\s+struct\s*\{[^}]*\}\s*(acnqp_\w+)\s*;", text)) == sorted(STRUCTS)
    consts = re.findall(r"#define\s+(ACNQP_(?:(?:STATUS|ROUTE|PILOTS|ADVANCE)_\w+|PREPARE_FUTURE|ABI_VERSION))\b", text)
    lines = []
    for name, cls in STRUCTS.items():
        lines.append(f'printf("%zu\\n", sizeof({name}));')
        lines += [f'printf("%zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f, _ in cls._fields_]
    lines += [f'printf("%d\\n", {c});' for c in consts]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "acn_qp.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n")
    cc = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    got = iter(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n"))
    checked = 0
    for name, cls in STRUCTS.items():
        assert int(next(got)) == C.sizeof(cls), name
        for f, ctype in cls._fields_:
            assert next(got).split() == [str(getattr(cls, f).offset), str(C.sizeof(ctype))], (name, f)
            checked += 1
    assert checked == sum(len(cls._fields_) for cls in STRUCTS.values()) >= 150
    assert C.sizeof(backend.Options) == 120 and backend.Options.polish_stall.offset == backend.Options.inaccurate_floor.offset + 8 == 112
    value ={c: int(next(got)) for c in consts}
    assert value.pop("ACNQP_ABI_VERSION") == 10
    assert {v: c[len("ACNQP_ROUTE_"):].lower() for c, v in value.items() if c.startswith("ACNQP_ROUTE_")} == backend.ROUTE_NAMES
    rest = {c[len("ACNQP_"):]: v for c, v in value.items() if not c.startswith("ACNQP_ROUTE_")}
    assert len(rest) == 6 + 3 + 3 + 1   # statuses, pilot modes, advance flags, the prepare flag
    assert rest == {k: getattr(backend, k) for k in rest}


def test_every_entry_has_its_prototype(hip_library):
    """After ``load_library`` every declared entry has the header's parameter count in ``argtypes``, and the introspection
    entries have theirs without any method having set it."""
    decl = dict(re.findall(r"\b(acnqp_[a-z_]+)\s*\(([^()]*)\)\s*;", _header()))
    assert set(decl) == set(backend.EXPORTED_SYMBOLS) == set(declared_symbols())
    for name, params in decl.items():
        n = 0 if params.strip() in ("", "void") else len(params.split(","))
        assert getattr(hip_library, name).argtypes is not None and len(getattr(hip_library, name).argtypes) == n, name
    for name, n in (("acnqp_debug_polish_alongside", 1), ("acnqp_debug_wave_rank", 2), ("acnqp_debug_wave_evse_extent", 2)):
        assert name not in backend.EXPORTED_SYMBOLS and len(getattr(hip_library, name).argtypes) == n, name
    assert hip_library.acnqp_debug_polish_alongside.restype is C.c_int64 and hip_library.acnqp_launch_count.restype is C.c_int64
    assert hip_library.acnqp_host_alloc.restype is C.c_void_p and hip_library.acnqp_last_error.restype is C.c_char_p


def test_create_rejects_bad_arguments(hip_library):
    h = C.c_void_p()
    assert hip_library.acnqp_create(None, 0, C.byref(h)) == -1
    assert b"null" in hip_library.acnqp_last_error()
    G = np.ones((1, 2000))
    lim = np.ones(1)
    desc = backend._Site(2000, 1, 1, 0, 0, 0, 0, G.ctypes.data_as(C.c_void_p), lim.ctypes.data_as(C.c_void_p))
    assert hip_library.acnqp_create(C.byref(desc), 0, C.byref(h)) == -1   # N > 1024
    desc = backend._Site(4, 1, 3, 0, 0, 0, 0, G.ctypes.data_as(C.c_void_p), lim.ctypes.data_as(C.c_void_p))
    assert hip_library.acnqp_create(C.byref(desc), 0, C.byref(h)) == -1   # n_rows inconsistent
    desc = backend._Site(4, 1, 1, 7, 0, 0, 0, G.ctypes.data_as(C.c_void_p), lim.ctypes.data_as(C.c_void_p))
    assert hip_library.acnqp_create(C.byref(desc), 0, C.byref(h)) == -1   # bad cone
    # SOC, 21 infrastructure rows + a peak row: n_rows = 43 <= 48, but the SOC rows pad to 8 * ceil(21 / 4) = 48, + 1
    G = np.ones((43, 4))
    lim = np.ones(21)
    desc = backend._Site(4, 21, 43, 1, 1, 0, 0, G.ctypes.data_as(C.c_void_p), lim.ctypes.data_as(C.c_void_p))
    assert hip_library.acnqp_create(C.byref(desc), 0, C.byref(h)) == -1
    assert b"49 site rows after padding" in hip_library.acnqp_last_error() and b"padded limit" in hip_library.acnqp_last_error()
    assert hip_library.acnqp_solve_batch(None, None, None, None) == -1
    assert hip_library.acnqp_last_kernel_ms(None) < 0
    assert hip_library.acnqp_accel_columns(None, 12, 1, 64, 10) == 0
    pol = C.c_int32(7)
    assert hip_library.acnqp_route(None, 12, 1, 1, C.byref(pol)) == 0 and pol.value == 0   # ABI v10: no handle, no route
    assert hip_library.acnqp_route(None, 12, 1, 1, None) == 0
    assert hip_library.acnqp_kernel_times(None, None, 0) == 0
    assert hip_library.acnqp_launch_count(None) == 0
    hip_library.acnqp_destroy(None)   # no-op


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setenv("ACNQP_LIBRARY", str(tmp_path / "nope.so"))
    monkeypatch.setattr(backend, "_lib", None)
    with pytest.raises(backend.BackendUnavailable, match="no CPU fallback"):
        backend.load_library()


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under adacharge_amd/ (nor
    bench.py's measured path) may import it."""
    pkg = os.path.join(ROOT, "adacharge_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f
                assert "oracle/" not in src or f.endswith((".hpp", ".py")) and "import" not in src.split("oracle/")[0][-20:]


@pytest.mark.gpu
def test_soc_row_limit_is_the_padded_one():
    """acnqp_create counts SOC rows as the kernels pad them (8 ceil(M / 4)): 21 rows + a peak (n_rows 43, 49 padded) is
    refused with a message naming the padded limit; 20 rows + a peak (n_rows 41, 41 padded, MR 48) is the largest such
    site, and it solves a small batch within the site rows."""
    from adacharge_amd import ObjectiveComponent, equal_share, quick_charge, sites
    from adacharge_amd.acn import Interface
    from adacharge_amd.backend import SiteHandle, default_options
    from adacharge_amd.builder import build_batch, make_site

    for pods, ok in ((15, False), (14, True)):   # M = pods + 6
        infra = sites.balanced_three_phase(60, pods=pods, load_fraction=0.35)
        assert infra.constraint_matrix.shape[0] == pods + 6
        site = make_site(infra, "SOC", with_peak=True)
        assert site.Mg == 2 * (pods + 6) + 1
        if not ok:
            with pytest.raises(ValueError, match="49 site rows after padding.*padded limit"):
                SiteHandle(site, 0)
            continue
        iface = Interface({"infrastructure_info": infra, "period": 5})
        snaps = sites.snapshot_batch(infra, 12, 8, seed=41)
        batch = build_batch(snaps, infra, iface, [ObjectiveComponent(quick_charge), ObjectiveComponent(equal_share, 1e-3)],
                            "SOC", peak_limits=[300.0] * 8, site=site)
        h = SiteHandle(site, 0)
        res = h.solve(batch, default_options())
        h.close()
        assert (res.status == 1).all(), res.status
        ph = np.deg2rad(infra.phases)
        cm = infra.constraint_matrix
        mag = np.hypot(np.einsum("mn,bnt->bmt", cm * np.cos(ph), res.x), np.einsum("mn,bnt->bmt", cm * np.sin(ph), res.x))
        assert (mag <= infra.constraint_limits[None, :, None] + 1e-3).all()
        assert (res.x.sum(axis=1) <= 300.0 + 1e-3).all()
