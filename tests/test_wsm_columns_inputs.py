"""What the column-height sweeps of WSM3 / WSM6 (tests/test_gpu_wsm_columns.py) and of their fall (tests/test_gpu_wsm_fall.py) rest
on, checked with the oracle alone: at every height the inputs reach every branch of the semi-Lagrangian fall that the oracle counts
(oracle/wsm_fall_count.h), rain -- and in the cold state snow, for WSM6 graupel too -- reaches the ground, and columns without any
hydrometeor share a 16-column tile of the fall kernels with columns that fall.  `pytest -s` prints the counter tables."""
import numpy as np
import wsm_columns_case as W

# (scheme or "probe", height, counter): reason.  Nothing for 8 levels and more.
EXEMPT = {
    (3, 3, "kt_gt_mid"): "kt is found among the interfaces below the top one, so kt <= km - 1 = 2 and kb >= 1: no whole arrival cell between them",
    (3, 3, "max_mid"): "as kt_gt_mid at 3 levels",
    ("probe", 3, "kt_gt_mid"): "as for the scheme at 3 levels: kt - kb - 1 <= km - 3 = 0",
    ("probe", 3, "max_mid"): "as kt_gt_mid at 3 levels",
    # a whole arrival cell below the ground needs interface 1 to fall further than the lowest level is thick in one minor step of at
    # most 180 s; the lowest level of these heights is 1.5 .. 2.6 km thick, rain near the ground falls at most 10 m/s (the probe's
    # synthetic columns reach the branch at these heights)
    (3, 3, "out_whole"): "lowest level 2.6 km thick: no hydrometeor falls that far in 180 s",
    (3, 4, "out_whole"): "lowest level 2.0 km thick: no hydrometeor falls that far in 180 s",
    (3, 5, "out_whole"): "lowest level 1.6 km thick: rain falls 10 m/s x 175 s = 1.75 km at most, and the limiter keeps interface 1 slower than the cell above",
    (6, 4, "out_whole"): "lowest level 2.0 km thick: no hydrometeor falls that far in 180 s",
    (6, 5, "out_whole"): "lowest level 1.6 km thick: as for WSM3 at 5 levels",
    # the 24 state columns that the fall probe takes beside its synthetic set (of them only columns, lim_trip and kt_eq_kb are asked)
    ("state columns", 3, "kt_eq_kb"): "levels of 3.6 km, 7.3 km and 100 m: no output level of these 24 columns lies inside one arrival cell; the synthetic set has kt == kb at 3 levels",
}


def table(title, rows, names):
    print("\n" + title)
    print(" nk " + " ".join(n[:8].rjust(8) for n in names))
    for nk, cnt in rows:
        print(f"{nk:3d} " + " ".join(f"{cnt[n]:8d}" for n in names))


def merge(a, b):
    return {n: (max(a[n], b[n]) if n == "max_mid" else a[n] + b[n]) for n in a} if a else dict(b)


def scheme_height(orc, scheme, nk):
    """both states of a height through the oracle: (counters, {state: result}, {state: case})"""
    cnt, outs, cases = {}, {}, {}
    for state in W.STATES:
        c = W.make_case(scheme, nk, state)
        out, n = W.counted(orc, lambda: W.oracle_run(orc, scheme, c, W.wsm_dt(nk), state=state))
        cnt = merge(cnt, n); outs[state] = out; cases[state] = c
    return cnt, outs, cases


def check_scheme(oracle, scheme):
    rows, bad = [], {}
    for nk in W.HEIGHTS[scheme]:
        cnt, outs, cases = scheme_height(oracle, scheme, nk)
        rows.append((nk, cnt))
        try:
            for n, v in cnt.items():
                assert v > 0 or (scheme, nk, n) in EXEMPT, f"counter {n} is 0"
                assert not (v > 0 and (scheme, nk, n) in EXEMPT), f"counter {n} is exempt but reached"
            for state, out in outs.items():
                c = cases[state]
                assert all(np.isfinite(a).all() for a in out.values()), "not finite"
                assert out["acc_rain"].max() > 0, f"{state}: no rain at the surface"
                assert W.untouched(c, out, scheme, cool=W.STATES[state]["cool"]), f"{state}: the oracle changed the ring"
                for k in W.KEYS[scheme][2:]:
                    assert c[k].max() > 0 and not np.array_equal(out[k], c[k]), f"{state}: {k} not seeded or unchanged"
                    assert state == "warm" or out[k][1:-1, :, 1:-1].max() > 0, f"{state}: no {k} after the last call"      # (the warm state melts its ice)
            assert outs["cold"]["acc_snow"].max() > 0.05, "cold: no snow at the surface"
            if scheme == 6:
                assert outs["cold"]["acc_graupel"].max() > 0.05, "cold: no graupel at the surface"
            dz = cases["warm"]["dz_levels"]
            assert abs(float(dz.sum()) - float(W.level_thickness(nk).sum())) < 1.0 and float(dz[-1]) == W.TOP_LEVEL, "column depth"
        except AssertionError as e:
            bad[nk] = str(e)
    table(f"WSM{scheme}: branches of the fall over both states, {W.CALLS} calls, {W.NX - 2} x {W.NY - 2} columns", rows, oracle.WSM_FALL_COUNTERS)
    assert not bad, bad


def test_wsm3_inputs_reach_every_branch_at_every_height(oracle):
    check_scheme(oracle, 3)


def test_wsm6_inputs_reach_every_branch_at_every_height(oracle):
    check_scheme(oracle, 6)


def test_exemptions_are_below_8_levels():
    assert all(nk < 8 for (_, nk, _) in EXEMPT)


def test_heights_time_steps_and_tile():
    assert W.WSM3_HEIGHTS == list(range(3, 65)) and W.WSM6_HEIGHTS == list(range(4, 65))
    for scheme in (3, 6):
        two = [nk for nk in W.HEIGHTS[scheme] if W.wsm_dt(nk) > 180.0]
        assert two and 64 in two and all(int(np.rint(W.wsm_dt(nk) / 120.0)) == 2 for nk in two), two
        assert all(60.0 <= W.wsm_dt(nk) <= 180.0 for nk in W.HEIGHTS[scheme] if nk not in two)
    n = W.NX - 2
    assert n >= 81 and n % W.TILE and 0 < n % W.TILE < 4 and n // W.TILE >= 4 and 64 < n < 128 and W.NY - 2 >= 3
    # every 16-column tile of a row (counted from its = 2, as the fall kernels do) holds a column that starts empty and one that does not
    empty = set(int(i) for i in W.empty_columns())
    for t in range((n + W.TILE - 1) // W.TILE):
        cols = [1 + t * W.TILE + o for o in range(W.TILE) if 1 + t * W.TILE + o <= W.NX - 2]
        assert any(i in empty for i in cols), (t, cols)         # (the last tile of three columns too)
        assert any(i not in empty for i in cols), (t, cols)
    # ... and the cases are built so: the shortest column, a middle one and both sides of the wave / serial switch, both states
    for scheme in (3, 6):
        for nk in (W.HEIGHTS[scheme][0], 40, 63, 64):
            for state in W.STATES:
                c = W.make_case(scheme, nk, state)
                for i in range(1, W.NX - 1):
                    none = not any(c[k][:, :, i].any() for k in W.KEYS[scheme][2:])
                    assert none == (i in empty), (scheme, nk, state, i)


def test_probe_columns_reach_every_branch_at_every_height(oracle):
    """the columns of tests/test_gpu_wsm_fall.py (24 of the scheme states and the synthetic set, one and two fields, with and without
    the refinement of the speed): every counter at every height, both outcomes of a re-evaluated level included; the synthetic set
    alone reaches every one too, and km - 3 whole cells between kb and kt -- the most there can be"""
    rows, bad = [], {}
    for km in range(3, 65):
        def run(cols):
            for c in cols:
                assert (c["rql"] >= 0).all(), c["name"]
                for nf in (1, 2):
                    for it in (0, 1):
                        q, p = W.oracle_fall(oracle, c, nf, it)
                        assert np.isfinite(q).all() and np.isfinite(p).all() and (q >= 0).all(), (km, c["name"])
        syn = W.synthetic_columns(km)
        _, cnt = W.counted(oracle, lambda: run(syn))
        rows.append((km, cnt))
        for n, v in cnt.items():
            if not (v > 0 or ("probe", km, n) in EXEMPT):
                bad[(km, n)] = v
        if cnt["max_mid"] != km - 3:
            bad[(km, "max_mid")] = cnt["max_mid"]
        _, cnt2 = W.counted(oracle, lambda: run(W.scheme_columns(km)))
        for n in ("columns", "lim_trip", "kt_eq_kb"):
            if (cnt2[n] > 0) == (("state columns", km, n) in EXEMPT):
                bad[(km, "state columns", n)] = cnt2[n]
    table("the synthetic columns of the fall probe: branches over NF = 1, 2 and iter = 0, 1", rows, oracle.WSM_FALL_COUNTERS)
    assert not bad, bad
