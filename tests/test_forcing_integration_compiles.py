"""The forcing block of INTEGRATION.md (section 2, fenced as f90), type-checked against the REFERENCE's own domain_t / boundary_t /
options_t, in the way tests/test_integration_compiles.py checks the `fortran` blocks: tests/support/integration_glue_forcing.f90 holds its
statements, flang -fsyntax-only must accept it, every statement of the block must be in it, and a glue with a member the reference does
not have must be rejected.  Build container only (skips where the reference sources are absent)."""
import os
import re

import pytest

import test_integration_compiles as T

GLUE = os.path.join(T.ROOT, "tests", "support", "integration_glue_forcing.f90")
pytestmark = T.pytestmark
modules = T.modules


def blocks():
    return re.findall(r"```f90\n(.*?)```", open(os.path.join(T.ROOT, "INTEGRATION.md")).read(), flags=re.S)


def test_forcing_glue_compiles_against_the_reference_modules(modules):
    rc, err = T.syntax_check(GLUE)
    assert rc == 0, err


def test_every_statement_of_the_forcing_block_is_in_the_glue(modules):
    b = blocks()
    assert len(b) == 1 and "hip_forcing_configure" in b[0] and "hip_forcing_step" in b[0] and "hip_update_delta_fields" in b[0]
    have = set(T.statements(open(GLUE).read()))
    want = T.statements(b[0])
    assert len(want) >= 30
    missing = [st for st in want if st not in have]
    assert not missing, "INTEGRATION.md statements that the compile-checked glue does not contain:\n  " + "\n  ".join(missing)


@pytest.mark.parametrize("old,new", [("this%nsmooth,", "this%nsmoothing,"),                               # no such member of domain_t
                                     ("forcing%geo_u%vert_lut%w", "forcing%geo_u%vert_lut%weights"),      # nor of vert_look_up_table
                                     ("domain%grid%halo_size, dt%seconds())", "domain%grid%halo_size, dt)")])   # time_delta_t is not REAL(8)
def test_a_wrong_forcing_binding_is_rejected(modules, tmp_path, old, new):
    src = open(GLUE).read()
    assert old in src
    p = tmp_path / "bad_glue.f90"
    p.write_text(src.replace(old, new, 1))
    rc, err = T.syntax_check(str(p))
    assert rc != 0 and "error" in err.lower()
