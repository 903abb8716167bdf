"""The semi-Lagrangian fall of WSM3 / WSM6 (icar_amd/csrc/wsm_fall.h) on its own, through tests/support/wsm_fall_probe.hip: the wave
form (one wave per column, 3 .. 63 levels) and the serial form (one thread per column, 3 .. 64 levels) against the oracle's fall
(oracle/wsm6_oracle.c: orc_wsm_fall_column, the functions its WSM6 runs, pinned to the compiled reference at every height in
tests/test_oracle_wsm_columns.py), bit for bit, for one and two fields with and without the refinement of the speed -- and with
that the two forms against each other on the same columns.  The columns: 24 of the sweep's scheme states per height and a synthetic
set for the edges (tests/wsm_columns_case.py: synthetic_columns); tests/test_wsm_columns_inputs.py shows with the oracle's branch
counters that they reach every branch of the fall at every height.  The refinement uses a probe speed of IEEE operations only."""
import ctypes
import numpy as np
import pytest
import wsm_columns_case as W
from util import COUNTS

pytestmark = pytest.mark.gpu
SERIAL, WAVE = 0, 1


def device_fall(probe, form, cols, nf, iter):
    km = cols[0]["dz"].size
    n = len(cols)
    a = {k: np.ascontiguousarray(np.stack([c[k] for c in cols]), np.float32) for k in ("den", "denfac", "tk", "dz", "ww")}
    rql = np.ascontiguousarray(np.stack([np.stack([c["rql"][f] for c in cols]) for f in range(nf)]), np.float32)      # (nf, n, km)
    dt = np.array([c["dt"] for c in cols], np.float32)
    out = np.full_like(rql, np.nan); precip = np.full((nf, n), np.nan, np.float32)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    rc = probe.icar_probe_wsm_fall(form, n, km, nf, iter, p(a["den"]), p(a["denfac"]), p(a["tk"]), p(a["dz"]), p(a["ww"]), p(rql), p(dt), p(out), p(precip))
    return rc, out, precip


def columns_of(km):
    cols = W.synthetic_columns(km) + W.scheme_columns(km)
    for c in cols:
        assert (c["rql"] >= 0).all(), c["name"]                 # the wave form's precondition for its empty-column test
    return cols


def height(oracle, probe, km):
    cols = columns_of(km)
    bad = []
    for nf in (1, 2):
        for it in (0, 1):
            want = [W.oracle_fall(oracle, c, nf, it) for c in cols]
            wq = np.stack([w[0] for w in want], axis=1); wp = np.stack([w[1] for w in want], axis=1)       # (nf, n, km), (nf, n)
            for form, name in ((WAVE, "wave"), (SERIAL, "serial")):
                if form == WAVE and km > 63:
                    continue
                rc, q, p = device_fall(probe, form, cols, nf, it)
                assert rc == 0, f"probe returned {rc}"
                COUNTS["bit_exact_fields"] += 2
                dq = q.view(np.int32) != wq.view(np.int32); dp = p.view(np.int32) != wp.view(np.int32)
                if dq.any() or dp.any():
                    who = sorted({cols[i]["name"] for i in np.nonzero(dq.any(axis=(0, 2)) | dp.any(axis=0))[0]})
                    lev = sorted({int(k) for k in np.nonzero(dq)[2]})
                    bad.append(f"{name} NF={nf} iter={it}: {int(dq.sum())} cells, {int(dp.sum())} surface sums differ; columns {who[:6]}; levels {lev[:8]}")
    assert not bad, "; ".join(bad)


def test_fall_both_forms_equal_the_oracle_at_every_height(oracle, probe):
    bad = {}
    for km in range(3, 65):
        try:
            height(oracle, probe, km)
        except AssertionError as e:
            bad[km] = str(e).splitlines()[0][:400]
    assert not bad, f"{len(bad)} of 62 column heights fail: " + " | ".join(f"km={k}: {v}" for k, v in bad.items())


@pytest.mark.parametrize("form,km", [(WAVE, 2), (WAVE, 64), (WAVE, 65), (SERIAL, 2), (SERIAL, 65)])
def test_probe_refuses_heights_outside_a_form(probe, form, km):
    """the entry checks km itself and launches nothing: the outputs keep what they held"""
    cols = W.synthetic_columns(max(km, 3))[:3]
    for c in cols:
        for k in ("den", "denfac", "tk", "dz", "ww"):
            c[k] = np.resize(c[k], km).astype(np.float32)
        c["rql"] = np.resize(c["rql"], (2, km)).astype(np.float32)
    rc, q, p = device_fall(probe, form, cols, 2, 1)
    assert rc == 3 and np.isnan(q).all() and np.isnan(p).all()
