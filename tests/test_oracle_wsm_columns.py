"""The CPU restatements of WSM3 / WSM6 (oracle/wsm3_oracle.c, oracle/wsm6_oracle.c) at every column height the device accepts, on
the inputs of the device's own sweep (tests/wsm_columns_case.py: both states of a height, its time step, three calls with cooling):
  * against the UNMODIFIED reference modules compiled into oracle/_ref, bit for bit on every field and surface sum, at every
    height (skipped where oracle/_ref is absent);
  * against golden vectors that those modules wrote (tests/golden/make_golden_wsm.py: COLUMN_CASES) at 3 / 4, 41, 62, 63 and 64
    levels, everywhere -- tests/golden_pin.py runs this part on the GPU machine's own build of the oracle."""
import json
import os
import sys

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLD)
from util import bits_equal  # noqa: E402
import make_golden_wsm as G  # noqa: E402
import wsm_columns_case as W  # noqa: E402
from oracle import ref  # noqa: E402      (a module of this repository: if it does not import, that is an error, not a skip)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32),
                          np.ascontiguousarray(b).view(np.int64 if b.dtype == np.float64 else np.int32))


@pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("scheme", [3, 6])
def test_oracle_equals_reference_at_every_height(oracle, scheme):
    ref.wsm3_init(); ref.wsm6_init()
    bad = {}
    for nk in W.HEIGHTS[scheme]:
        for state in W.STATES:
            c = W.make_case(scheme, nk, state, nx=G.COLUMNS_NX)
            want = W.oracle_run(None, scheme, c, W.wsm_dt(nk), state=state, ref=ref)
            got = W.oracle_run(oracle, scheme, c, W.wsm_dt(nk), state=state)
            diff = {k: int((got[k] != want[k]).sum()) for k in want if not same(got[k], want[k])}
            if diff:
                bad[(nk, state)] = diff
            assert want["acc_rain"].max() > 0
    assert not bad, f"{len(bad)} of {2 * len(W.HEIGHTS[scheme])} runs differ from the compiled reference: {bad}"


@pytest.mark.parametrize("name", list(G.COLUMN_CASES))
def test_wsm_columns_golden(oracle, name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    p = json.loads(str(g["params"]))
    assert p == G.COLUMN_CASES[name], "fixture made with other parameters: rerun tests/golden/make_golden_wsm.py"
    c = W.make_case(p["scheme"], p["nz"], p["state"], nx=G.COLUMNS_NX)
    assert G.columns_fingerprint(c, p["scheme"]) == float(g["input_fingerprint"]), "the inputs drifted: the stored outputs belong to other inputs"
    got = W.oracle_run(oracle, p["scheme"], c, W.wsm_dt(p["nz"]), state=p["state"])
    for k in got:
        assert got[k].dtype == g[k].dtype and bits_equal(got[k].astype(np.float32), g[k].astype(np.float32)) and same(got[k], g[k]), \
            f"{k}: {int((got[k] != g[k]).sum())} cells differ"
    assert g["acc_rain"].max() > 0
