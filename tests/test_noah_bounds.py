"""tests/support/noah_bounds_main.c -- the restatement of lsm_noah and LSM_NOAH_INIT under the address and undefined-behaviour sanitizers,
as a stand-alone program (nothing is loaded into python, nothing runs on a GPU): it runs lsm_init and every carried call on a fixture's
inputs with every table an allocation of exactly the reference's extent, then single cells whose categories sit at both ends of every
table.  Its checksum over the outputs is the restatement's run through python: the program ran what the fixtures pin."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import noah_oracle as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "support", "noah_bounds_main.c")
SAN = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

pytestmark = pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc is not present on this host")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("noah_bounds") / "noah_bounds")
    r = subprocess.run(["gcc"] + SAN + [SRC, "-o", exe, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def write_case(path, tab, c):
    A = N.state0(c)
    names = N.fields()
    force = [k for k in names if k in c["forcing"][0]]
    with open(path, "wb") as f:
        np.array([c["nx"], c["ny"], len(c["forcing"]), N.ISURBAN, N.ISICE, int(c["fndsnowh"]), len(force)], np.int32).tofile(f)
        np.array([c["dt"]], np.float32).tofile(f)
        np.ascontiguousarray(tab["nrotbl"], np.int32).tofile(f)
        for k in N.T_VEG + N.T_SOIL + ["slope_data"]:
            np.ascontiguousarray(tab[k], np.float32).tofile(f)
        np.array([tab[k] for k in N.T_GEN], np.float32).tofile(f)
        np.array([tab[k] for k in N.T_INT], np.int32).tofile(f)
        for k in names:
            a = c["forcing"][0][k] if k in force else c[k] if k in c else A[k]
            np.ascontiguousarray(a, np.int32 if k in ("ivgtyp", "isltyp") else np.float32).tofile(f)
        np.array([names.index(k) for k in force], np.int32).tofile(f)
        for F in c["forcing"]:
            for k in force:
                F[k].tofile(f)


@pytest.mark.parametrize("name", ["noah_a_snowfall_melt_24x12", "noah_d_deep_pack_23x13", "noah_f_urban_bare_24x12"])
def test_no_finding_on_a_fixture_s_inputs_and_at_the_tables_ends(program, tmp_path, name):
    tab = N.load_tables()
    c = N.make_case(tab, **N.CASES[name])
    path = str(tmp_path / "case.bin")
    write_case(path, tab, c)
    r = subprocess.run([program, path], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-3000:])
    assert "table ends: 4 cells, no finding" in r.stdout
    A = N.state0(c)
    N.lsm_init(tab, c, A)
    for n in range(len(c["forcing"])):
        N.lsm_noah(tab, c, A, n)
    want = sum(int(A[k].view(np.uint32).astype(np.uint64).sum()) for k in N.OUT) % 2 ** 64
    assert int(r.stdout.split("checksum")[1].split()[0]) == want
