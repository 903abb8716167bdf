"""The block of INTEGRATION.md for the 2-D forced variables (section 2, fenced as f95), type-checked against the REFERENCE's own domain_t /
variable_t / time_delta_t, in the way tests/test_forcing_integration_compiles.py checks the f90 block:
tests/support/integration_glue_forcing2d.f90 holds its statements, flang -fsyntax-only must accept it, every statement of the block must
be in it, and a glue with a member the reference does not have must be rejected.  Build container only (skips where the reference
sources are absent)."""
import os
import re

import pytest

import test_integration_compiles as T

GLUE = os.path.join(T.ROOT, "tests", "support", "integration_glue_forcing2d.f90")
pytestmark = T.pytestmark
modules = T.modules


def blocks():
    return re.findall(r"```f95\n(.*?)```", open(os.path.join(T.ROOT, "INTEGRATION.md")).read(), flags=re.S)


def test_forcing2d_glue_compiles_against_the_reference_modules(modules):
    rc, err = T.syntax_check(GLUE)
    assert rc == 0, err


def test_every_statement_of_the_forcing2d_block_is_in_the_glue(modules):
    b = blocks()
    assert len(b) == 1
    for name in ("hip_forcing2d_upload", "hip_forcing2d_interpolate", "hip_forcing2d_update_delta", "hip_forcing2d_apply", "hip_forcing2d_enable",
                 "hip_forcing2d_get", "hip_forcing2d_set"):
        assert name in b[0], name
    have = set(T.statements(open(GLUE).read()))
    want = T.statements(b[0])
    assert len(want) >= 10
    missing = [st for st in want if st not in have]
    assert not missing, "INTEGRATION.md statements that the compile-checked glue does not contain:\n  " + "\n  ".join(missing)


@pytest.mark.parametrize("old,new", [("domain%sst%dqdt_2d)", "domain%sst%dqdt_2dd)"),                             # no such member of variable_t
                                     ("ICAR_FORCED2D_SST, input_data%data_2d)", "ICAR_FORCED2D_SST, input_data%data_3d)"),   # rank 3 for a rank-2 dummy
                                     ("hip_forcing2d_apply(hip, dt%seconds())", "hip_forcing2d_apply(hip, dt)")])   # time_delta_t is not REAL(8)
def test_a_wrong_forcing2d_binding_is_rejected(modules, tmp_path, old, new):
    src = open(GLUE).read()
    assert old in src
    p = tmp_path / "bad_glue.f90"
    p.write_text(src.replace(old, new, 1))
    rc, err = T.syntax_check(str(p))
    assert rc != 0 and "error" in err.lower()
