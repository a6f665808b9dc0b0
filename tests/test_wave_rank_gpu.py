"""The wave kernel's eigen extent (acn_qp_rank.hpp): the site's live eigenpairs compacted to the
front and the null k-steps not computed, against the full extent on the shared eigenbasis (ACNQP_WAVE_FULL_RANK=1, the
kernel as it was).  The switch is read once per process, so the cases of tests/wave_rank_cases.py are solved in two
child processes -- all of them in each -- and compared here: the same bits (a skipped term was finite x 0 and the live
terms of every sum keep their order).  What acnqp_debug_wave_rank reports is asserted for every case, so that no case
can pass by running the full extent twice."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import wave_rank_cases as WC

FAMILY = {"soc_h12": "wave1", "linear_h12": "wave1", "soc_h24": "wave2", "soc_h40": "wave5", "mt2_h12": "wave3", "mt2_h24": "wave4",
          "infeasible": "wave1", "warm": "wave1"}


@functools.lru_cache(maxsize=None)
def _runs():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for tag, env in (("site", {}), ("full", {"ACNQP_WAVE_FULL_RANK": "1"})):
            f = os.path.join(tmp, tag + ".npz")
            e = {k: v for k, v in os.environ.items() if k not in ("ACNQP_WAVE_FULL_RANK", "ACNQP_NO_WAVE", "ACNQP_NO_WAVE2", "ACNQP_WAVE_MIN_BATCH")}
            subprocess.run([sys.executable, WC.__file__, f], check=True, env=dict(e, **env), timeout=600)
            with np.load(f) as z:
                out[tag] = {k: z[k] for k in z.files}
    return out


def _expected(name):
    """(rank, live k-steps once compacted, extent of the instantiation, padded rows / 4) from the site's rows alone"""
    site = WC.build(name)[0].site
    rank = int(np.linalg.matrix_rank(site.G))
    padded = 8 * ((site.M + 3) // 4) if site.cone == 1 else site.M
    full = 4 * max(1, -(-padded // 16))
    ks = -(-rank // 4)
    return rank, ks, (2 if ks <= 2 else 3 if ks == 3 else full), full


@pytest.mark.gpu
@pytest.mark.parametrize("name", WC.CASES)
def test_site_extent_gives_the_bits_of_the_full_extent(name):
    r = _runs()
    site, full = ({k.split(":", 1)[1]: v for k, v in r[tag].items() if k.startswith(name + ":")} for tag in ("site", "full"))
    rank, ks, ext, all_ks = _expected(name)
    fam = FAMILY.get(name, "wave1")
    assert str(site["family"]) == fam and str(full["family"]) == fam
    assert (int(site["rank"]), int(site["eig_ksteps"]), int(site["extent"])) == (rank, ks, ext), name
    assert (int(full["rank"]), int(full["eig_ksteps"]), int(full["extent"])) == (rank, ks, all_ks), name
    if name.startswith("syn"):
        rows = int(name[3:])
        assert rank == rows and ext == {8: 2, 9: 3, 12: 3, 13: 4, 16: 4}[rows]
    else:
        assert ext < all_ks, (name, ext, all_ks)   # the sites of BASELINE.json all take a specialised extent
    for key in WC.KEYS + (("y",) if "y" in site else ()):
        assert np.array_equal(site[key], full[key]), (name, key, np.abs(site[key].astype(float) - full[key].astype(float)).max())
    if name == "infeasible":
        assert site["status"][0] == 3 and np.isin(site["status"], (1, 3)).all() and (site["status"] == 1).sum() >= 8, site["status"]
    else:
        assert (site["status"] == 1).all(), (name, site["status"])
    if name == "warm":
        assert "y" in site


@pytest.mark.gpu
@pytest.mark.parametrize("rows", WC.SYNTHETIC_ROWS)
def test_full_rank_sites_pass_the_host_kkt_check(rows):
    """A wrong permutation of fragQ would hit both runs alike where it does nothing (a site whose eigenpairs are compact
    already) -- and anywhere else the answer would be wrong: the host certificate (oracle/kkt.py) on the synthetic sites."""
    from oracle import kkt

    name = f"syn{rows}"
    batch = WC.build(name)[0]
    got = {k.split(":", 1)[1]: v for k, v in _runs()["site"].items() if k.startswith(name + ":")}
    for b in range(batch.B):
        bad = kkt.failures(kkt.certify(batch, b, got["x"][b], got["y"][b], got["obj"][b]), int(got["status"][b]))
        assert not bad, (name, b, bad)
