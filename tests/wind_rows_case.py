"""Inputs, shape lists and a numpy restatement for the geometry sweep of the linear-wind rows W2 / W3
(tests/test_gpu_wind_rows_geometry.py on the device, tests/test_wind_rows_inputs.py for what the inputs, the restatement and the
oracle alone must meet).  Needs no GPU.

spatial_winds() below is written from the reference's Fortran statements -- src/physics/linear_winds.f90:906-1126,
src/utilities/array_utilities.f90:263-288 (calc_weight) and :355-411 (smooth_array_3d, ydim = 3), src/utilities/atm_utilities.f90:
334-367 and :401-467 -- one float32 numpy expression per statement, NOT from oracle/wind_oracle.c: a second, independent statement of
what the W2 kernels of icar_amd/csrc/linear_winds.hip have to compute.  What is sequential in the reference stays sequential here:
the in-place bottom-up vertical smoothing, the DOUBLE PRECISION running row and column sums of smooth_array, and the row loop
(rows 1 .. ny see winds that their own row has not changed yet; row ny + 1 sees u(:, :, ny) after its update).  log, exp and atan
are the host C library's logf / expf / atanf through ctypes: numpy's own float32 log / exp are not bit-identical to them.

Arrays are C-order (ny, nz, nx) == Fortran (i, k, j); u is (ny, nz, nx + 1), v is (ny + 1, nz, nx); the look-up tables are in the
reference's order, C-order (ny[+1], nz, nx[+1], n_nsq, n_dir, n_spd)."""
import ctypes
import numpy as np
from icar_amd.options import lt_options_type
from oracle import wind_oracle as W
from wind_case import atmosphere

f32 = np.float32
_libm = ctypes.CDLL("libm.so.6")
for _n in ("logf", "expf", "atanf"):
    getattr(_libm, _n).restype = ctypes.c_float
    getattr(_libm, _n).argtypes = [ctypes.c_float]

PI = f32(3.1415927)                      # src/constants/icar_constants.f90:389-395
LH_VAPORIZATION = f32(2260000.0)
RD = f32(287.058)
RW = f32(461.5)
CP = f32(1012.0)
GRAVITY = f32(9.81)
ONE = f32(1)

ARMS = ("v<0", "v==0,u>0", "v==0,u<=0", "v>0,u>=0", "v>0,u<0")       # the five ways through calc_direction


def _libm_f(name, a):
    a = np.asarray(a, f32)
    fn = getattr(_libm, name)
    return np.fromiter((fn(x) for x in a.ravel().tolist()), f32, a.size).reshape(a.shape)


def logf(a): return _libm_f("logf", a)
def expf(a): return _libm_f("expf", a)
def atanf(a): return _libm_f("atanf", a)


# ---- restatement ------------------------------------------------------------------------------------------------------------
def calc_sat_lapse_rate(T, mr):
    """atm_utilities.f90:401-410"""
    L = LH_VAPORIZATION                                                                         # :407
    return GRAVITY * ((ONE + (L * mr) / (RD * T)) / (CP + (L * L * mr * (RD / RW)) / (RD * T * T)))   # :408-409


def calc_moist_stability(t_top, t_bot, z_top, z_bot, qv_top, qv_bot, qc):
    """atm_utilities.f90:417-430"""
    t = (t_top + t_bot) / f32(2)                                                                # :423
    qv = (qv_top + qv_bot) / f32(2)                                                             # :424
    dz = z_top - z_bot                                                                          # :425
    sat_lapse = calc_sat_lapse_rate(t, qv)                                                      # :426
    return ((GRAVITY / t) * ((t_top - t_bot) / dz + sat_lapse) * (ONE + (LH_VAPORIZATION * qv) / (RD * t))
            - (GRAVITY / (ONE + qv + qc) * (qv_top - qv_bot) / dz))                             # :428-429


def calc_dry_stability(th_top, th_bot, z_top, z_bot):
    """atm_utilities.f90:436-442"""
    return GRAVITY * (logf(th_top) - logf(th_bot)) / (z_top - z_bot)                            # :441


def calc_stability(th_top, th_bot, pii_top, pii_bot, z_top, z_bot, qv_top, qv_bot, qc, variable_N, N_squared):
    """atm_utilities.f90:448-467 on arrays"""
    if variable_N:
        with np.errstate(all="ignore"):
            dry = calc_dry_stability(th_top, th_bot, z_top, z_bot)                              # :455
            moist = calc_moist_stability(th_top * pii_top, th_bot * pii_bot, z_top, z_bot, qv_top, qv_bot, qc)   # :461
    else:
        dry = np.full(qc.shape, f32(N_squared), f32)                                            # :457
        moist = dry / f32(10.0)                                                                 # :463
    return np.where(qc < f32(1e-7), dry, moist).astype(f32)                                     # :453


def calc_direction(u, v):
    """atm_utilities.f90:334-355 on arrays: (direction, the index into ARMS of the arm each element took)"""
    with np.errstate(all="ignore"):
        a = atanf(u / v)
    arm = np.where(v < 0, 0, np.where(v == 0, np.where(u > 0, 1, 2), np.where(u >= 0, 3, 4)))
    direction = np.choose(arm, [a + PI,                                                         # :340
                                np.full(a.shape, PI / f32(2.0), f32),                           # :343
                                np.full(a.shape, PI * f32(1.5), f32),                           # :345
                                a,                                                              # :349
                                a + (f32(2) * PI)])                                             # :351
    assert direction.dtype == np.float32
    return direction, arm.astype(np.int32)


def calc_speed(u, v):
    return np.sqrt(u * u + v * v)                                                               # atm_utilities.f90:366


def bracket(axis, match):
    """the search loops of linear_winds.f90:1045-1074: pos = 1; do step = 1, n; if (match > axis(step)) pos = step"""
    pos = np.ones(match.shape, np.int32)
    for step in range(1, len(axis) + 1):
        pos = np.where(match > axis[step - 1], np.int32(step), pos)
    return pos


def calc_weight(axis, bestpos, match):
    """array_utilities.f90:263-288 on arrays: (weight, nextpos), 1-based positions"""
    n = len(axis)
    low = match < axis[0]                                                                       # :275
    top = bestpos == n                                                                          # :279
    nextpos = np.where(low, 1, np.where(top, n, bestpos + 1)).astype(np.int32)                  # :276, :280, :283
    inner = np.minimum(bestpos + 1, n)
    with np.errstate(all="ignore"):
        w = (axis[inner - 1] - match) / (axis[inner - 1] - axis[bestpos - 1])                   # :284
    weight = np.where(low | top, ONE, w).astype(f32)                                            # :277, :281
    return weight, nextpos


def smooth_array_ydim3(wind, windowsize):
    """array_utilities.f90:308-417 with ydim = 3 on wind (nrow, nlev, nx) == Fortran (nx, ny = levels, nz = rows); returns the
    smoothed copy.  rowsums, rowmeans and cursum are DOUBLE PRECISION (:321-322)."""
    nrow, nlev, nx = wind.shape
    w = int(windowsize)
    assert nx > w, "rowmeans(2:windowsize) needs nx > windowsize"
    inputwind = wind.copy()                                                                     # :332
    out = np.empty_like(wind)
    nrows = ncols = w * 2 + 1                                                                   # :325, :351-352
    for j in range(nlev):                                                                       # :355
        rowsums = (inputwind[0, j, :] * f32(w + 2)).astype(np.float64)                          # :362
        for i in range(2, min(w, nrow) + 1):                                                    # :363
            rowsums = rowsums + inputwind[i - 1, j, :]                                          # :364
        if w > nrow:                                                                            # :366
            rowsums = rowsums + (inputwind[nrow - 1, j, :] * f32(w - nrow)).astype(np.float64)  # :367
        for k in range(1, nrow + 1):                                                            # :373
            starty = max(2, k - w)                                                              # :376
            endy = min(nrow, k + w)                                                             # :377
            rowsums = rowsums - inputwind[starty - 2, j, :] + inputwind[endy - 1, j, :]         # :378
            assert rowsums.dtype == np.float64
            rowmeans = rowsums / nrows                                                          # :383
            cursum = np.float64(0)
            for i in range(2, w + 1):                                                           # sum(rowmeans(2:windowsize))
                cursum = cursum + rowmeans[i - 1]
            cursum = cursum + rowmeans[0] * (w + 2)                                             # :384
            for i in range(1, nx + 1):                                                          # :387
                startx = max(2, i - w)                                                          # :389
                endx = min(nx, i + w)                                                           # :390
                cursum = cursum - rowmeans[startx - 2] + rowmeans[endx - 1]                     # :391
                out[k - 1, j, i - 1] = f32(cursum / ncols)                                      # :393
    return out


def vsmooth_window(j, nz, vsmooth):
    """(bottom, top), 1-based, of linear_winds.f90:920-922 and :962-963"""
    top = min(j + vsmooth, nz)
    bottom = max(1, j - (vsmooth - (top - j)))
    return bottom, top


def _interpolate(L, b):
    """linear_winds.f90:1084-1091 / :1100-1107 without the relaxation: L is one (row, level) line of a table, (n, n_nsq, n_dir,
    n_spd); b holds the brackets and weights of the same n faces"""
    ii = np.arange(L.shape[0])

    def lut(s, d, n):
        return L[ii, n - 1, d - 1, s - 1]
    dw, sw, nw = b["dweight"], b["sweight"], b["nweight"]
    first = (nw * (dw * lut(b["spos"], b["dpos"], b["npos"]) + (ONE - dw) * lut(b["spos"], b["nextd"], b["npos"]))
             + (ONE - nw) * (dw * lut(b["spos"], b["dpos"], b["nextn"]) + (ONE - dw) * lut(b["spos"], b["nextd"], b["nextn"])))
    second = (nw * (dw * lut(b["nexts"], b["dpos"], b["npos"]) + (ONE - dw) * lut(b["nexts"], b["nextd"], b["npos"]))
              + (ONE - nw) * (dw * lut(b["nexts"], b["dpos"], b["nextn"]) + (ONE - dw) * lut(b["nexts"], b["nextd"], b["nextn"])))
    out = sw * first + (ONE - sw) * second
    assert out.dtype == np.float32
    return out


def spatial_winds(u3d, v3d, th, exner, z, qv, hydrometeors, u_lut, v_lut, u_pert, v_pert, opt, dirv, spdv, nsqv, vsmooth, winsz,
                  state=None):
    """linear_winds.f90:840-1127 with reverse = .false.; the arguments of oracle.orc.spatial_winds: u3d, v3d, u_pert and v_pert
    are updated in place, nsquared is returned.  With a dict as `state` it is filled with the bracket state: per face (ny + 1,
    nx + 1) dpos, nextd, spos, nexts, dweight, sweight, arm (index into ARMS), curdir, curspd; per face and level (ny + 1, nz,
    nx + 1) npos, nextn, nweight, curnsq; per cell (ny, nz, nx) at_min / at_max (N^2 sits on min_stability / max_stability)."""
    ny, nz, nx = th.shape
    nxu, nyv = nx + 1, ny + 1
    variable_N, smooth_nsq = bool(opt["variable_N"]), bool(opt["smooth_nsq"])
    N_squared, max_stability, min_stability = f32(opt["N_squared"]), f32(opt["max_stability"]), f32(opt["min_stability"])
    linear_contribution, linear_update_fraction = f32(opt["linear_contribution"]), f32(opt["linear_update_fraction"])
    nsquared = np.zeros((ny, nz, nx), f32)
    at_min = np.zeros((ny, nz, nx), bool); at_max = np.zeros((ny, nz, nx), bool)
    for k in range(ny):                                                                         # :913
        for j in range(1, nz + 1):                                                              # :915
            if variable_N:                                                                      # :918
                bottom, top = vsmooth_window(j, nz, vsmooth)                                    # :920-922
                hyd = np.zeros(nx, f32)                                                         # :924
                for q in hydrometeors:                                                          # :925-932
                    if q is not None:
                        hyd = hyd + q[k, j - 1, :]
                b, t = bottom - 1, top - 1
                val = calc_stability(th[k, b], th[k, t], exner[k, b], exner[k, t], z[k, b], z[k, t], qv[k, b], qv[k, t], hyd,
                                     variable_N, N_squared)                                     # :936-941 (bottom in the *_top slots)
                val = np.maximum(min_stability, np.minimum(max_stability, val))                 # :943
                at_min[k, j - 1] = val == min_stability; at_max[k, j - 1] = val == max_stability
            else:
                val = np.full(nx, N_squared, f32)                                               # :952
            nsquared[k, j - 1, :] = logf(val)                                                   # :956
        if smooth_nsq:                                                                          # :959
            for j in range(1, nz + 1):
                bottom, top = vsmooth_window(j, nz, vsmooth)                                    # :962-963
                for smoothz in range(bottom, j):                                                # :965
                    nsquared[k, j - 1, :] = nsquared[k, j - 1, :] + nsquared[k, smoothz - 1, :]
                for smoothz in range(j + 1, top + 1):                                           # :968
                    nsquared[k, j - 1, :] = nsquared[k, j - 1, :] + nsquared[k, smoothz - 1, :]
                nsquared[k, j - 1, :] = nsquared[k, j - 1, :] / f32(top - bottom + 1)           # :971
    if smooth_nsq:
        nsquared = smooth_array_ydim3(nsquared, winsz)                                          # :981

    st = {n: np.zeros((nyv, nxu), np.int32) for n in ("dpos", "nextd", "spos", "nexts", "arm")}
    st.update({n: np.zeros((nyv, nxu), f32) for n in ("dweight", "sweight", "curdir", "curspd")})
    st.update({n: np.zeros((nyv, nz, nxu), np.int32) for n in ("npos", "nextn")})
    st.update({n: np.zeros((nyv, nz, nxu), f32) for n in ("nweight", "curnsq")})
    vi = np.minimum(np.arange(nxu), nx - 1)                                                     # :998, 0-based
    for k in range(1, nyv + 1):                                                                 # :994
        uk = min(k, ny)                                                                         # :996
        su = np.zeros(nxu, f32); sv = np.zeros(nxu, f32)
        for j in range(nz):                                                                     # sum(u3d(i, :, uk)), sum(v3d(vi, :, k))
            su = su + u3d[uk - 1, j, :]
            sv = sv + v3d[k - 1, j, vi]
        u1d = su / f32(nz)                                                                      # :999
        v1d = sv / f32(nz)                                                                      # :1000
        b = {}
        curdir, arm = calc_direction(u1d, v1d)                                                  # :1046
        b["dpos"] = bracket(dirv, curdir)                                                       # :1045-1052
        curspd = calc_speed(u1d, v1d)                                                           # :1056
        b["spos"] = bracket(spdv, curspd)                                                       # :1055-1062
        b["dweight"], b["nextd"] = calc_weight(dirv, b["dpos"], curdir)                         # :1078
        b["sweight"], b["nexts"] = calc_weight(spdv, b["spos"], curspd)                         # :1079
        for n in ("dpos", "nextd", "spos", "nexts", "dweight", "sweight"):
            st[n][k - 1] = b[n]
        st["arm"][k - 1] = arm; st["curdir"][k - 1] = curdir; st["curspd"][k - 1] = curspd
        for j in range(1, nz + 1):                                                              # :1003
            bottom = max(j - winsz, 1)                                                          # :1019
            top = min(j + winsz, nz)                                                            # :1020
            sn = np.zeros(nxu, f32)
            for s in range(bottom, top + 1):                                                    # sum(nsquared(vi, bottom:top, uk))
                sn = sn + nsquared[uk - 1, s - 1, vi]
            curnsq = sn / f32(top - bottom + 1)                                                 # :1067
            b["npos"] = bracket(nsqv, curnsq)                                                   # :1069-1074
            b["nweight"], b["nextn"] = calc_weight(nsqv, b["npos"], curnsq)                     # :1080
            for n in ("npos", "nextn", "nweight"):
                st[n][k - 1, j - 1] = b[n]
            st["curnsq"][k - 1, j - 1] = curnsq
            if k <= ny:                                                                         # :1083
                wind = _interpolate(u_lut[k - 1, j - 1], b)
                u_pert[k - 1, j - 1, :] = (u_pert[k - 1, j - 1, :] * (ONE - linear_update_fraction)
                                           + linear_update_fraction * wind)                     # :1090-1091
                u3d[k - 1, j - 1, :] = u3d[k - 1, j - 1, :] + u_pert[k - 1, j - 1, :] * linear_contribution   # :1096
            bv = {n: a[:nx] for n, a in b.items()}                                              # :1099 (i <= nx)
            wind = _interpolate(v_lut[k - 1, j - 1], bv)
            v_pert[k - 1, j - 1, :] = (v_pert[k - 1, j - 1, :] * (ONE - linear_update_fraction)
                                       + linear_update_fraction * wind)                         # :1106-1107
            v3d[k - 1, j - 1, :] = v3d[k - 1, j - 1, :] + v_pert[k - 1, j - 1, :] * linear_contribution       # :1113
    nsquared = expf(nsquared)                                                                   # :1125
    if state is not None:
        state.update(st); state["at_min"] = at_min; state["at_max"] = at_max
    return nsquared


# ---- the W2 sweep -----------------------------------------------------------------------------------------------------------
WIDTH_WINSZ = 2
# nx and nx + 1 on both sides of 64 and of 128 (blocks of 64 over nx and over nx + 1); WIDTH_WINSZ + 1 is the smallest width the
# device accepts with smooth_nsq on
WIDTHS = [WIDTH_WINSZ + 1, 62, 63, 64, 65, 127, 128, 129]
LEVELS = [2, 3, 4, 5, 8, 9, 63, 64, 65]      # at 6 x 3: every nz % 4 (tiles of 4 levels), the thinnest column, the second block of k_lw_colsmooth
ROW_WINSZ = 4
ROWS = [3, 4, 5, 9, 10]                      # at winsz 4, nx 9, nz 3: ny < w, ny == w, ny == w + 1, 2w + 1, 2w + 2 (the arms of the running row sums)
WINDOWS = [(1, 1), (2, 1), (3, 4), (4, 2), (7, 8)]   # (vsmooth, winsz) at 9 x 5 x 4: vsmooth = nz - 1, nz and beyond; winsz >= nz; always nx > winsz
HYDROMETEORS = ("all", "none", "rain")       # the four fields associated, none of them, only rain_mass
AXES = [(5, 3, 2), (2, 2, 2)]                # (n_dir, n_spd, n_nsq); the setup refuses fewer than two values on an axis
PLANT_SHAPE = (66, 4, 5)
PLANT_FACES = [0, 1, 2, 3, 4, 5, 63, 64, 66]  # the first faces, both sides of the wave edge, the last face (it reads v cell nx - 1)
PLANT_ROWS = (0, 2)
# (u, v) of a whole column, so that the column mean is exact, and the edge it reaches
PLANTS = [(0.0, 0.0),        # calm: v == 0, u <= 0 arm, speed 0
          (5.0, 0.0),        # v == 0, u > 0
          (-5.0, 0.0),       # v == 0, u <= 0
          (0.0, 4.0),        # curdir == 0 == dirv[0]
          (0.0, -4.0),       # curdir == pi
          (-1e-6, 6.0),      # curdir rounds to dirmax: the top of the direction axis, dweight == 0
          (6.0, 8.0),        # speed exactly 10 == spdv[1] with 4 speeds on 0 .. 30: sweight == 0
          (40.0, 20.0)]      # faster than spdmax: bestpos == n, nexts == n
UNSTABLE_COLUMNS = [0, 1, 5, 63, 64, 65]     # theta falls 2 K per level: N^2 < 0 -> min_stability
INVERSION_COLUMNS = [2, 3, 62]               # theta rises 30 K per level: N^2 ~ 1e-2 -> max_stability
# the second option set of the planted case: the low ends of the axes lie inside the data, so that match < d(1) (weight 1, next = 1)
# is reachable on all three, and -- beyond what the first set can reach, see planted_case -- so do the high ends of the direction
# and N^2 axes, so that bestpos == n is reachable on them too
PLANT_SECOND = dict(spdmin=4.0, dirmin=0.5, dirmax=6.0, nsqmin=-14.0, nsqmax=-8.0)


def case(label, nx, ny, nz, winsz, vsmooth, n, variable_N=None, smooth_nsq=True):
    """one case of the sweep; n rotates the option sets through the shapes: variable_N alternates unless given, the hydrometeor
    sets have period 3, update is on in two of five, the small axes in three of seven"""
    return dict(label=label, nx=nx, ny=ny, nz=nz, winsz=winsz, vsmooth=vsmooth, smooth_nsq=smooth_nsq,
                variable_N=(n % 2 == 0) if variable_N is None else variable_N, hydrometeors=HYDROMETEORS[n % 3],
                update=n % 5 in (1, 3), axes=AXES[0] if n % 7 < 4 else AXES[1], seed=100 + n, options={})


def width_cases():
    """ny alternates 3, 4; nz cycles 2 .. 5"""
    return [case(f"width {nx}", nx, 3 + n % 2, 2 + n % 4, WIDTH_WINSZ, 2, n) for n, nx in enumerate(WIDTHS)]


def level_cases():
    return [case(f"levels {nz}", 6, 3, nz, 2, 3, 8 + n) for n, nz in enumerate(LEVELS)]


def row_cases():
    return [case(f"rows {ny}", 9, ny, 3, ROW_WINSZ, 1, 17 + n) for n, ny in enumerate(ROWS)]


def window_cases():
    return [case(f"windows vsmooth {vs} winsz {w}", 9, 5, 4, w, vs, 22 + n, variable_N=True) for n, (vs, w) in enumerate(WINDOWS)]


def unsmoothed_cases():
    """smooth_nsq off (every list above has it on: the smoothing kernels are what most of their edges belong to), with and without
    variable_N, at a width on the block edge, a column in the second block of 64 levels and a window wider than the column"""
    return [case("unsmoothed 64 wide", 64, 4, 5, 2, 2, 27, variable_N=True, smooth_nsq=False),
            case("unsmoothed 65 wide fixed N", 65, 3, 2, 2, 2, 28, variable_N=False, smooth_nsq=False),
            case("unsmoothed 65 levels", 6, 3, 65, 2, 3, 29, variable_N=True, smooth_nsq=False),
            case("unsmoothed winsz 8 fixed N", 9, 5, 4, 8, 7, 30, variable_N=False, smooth_nsq=False)]


def sweep_cases():
    return width_cases() + level_cases() + row_cases() + window_cases() + unsmoothed_cases()


def planted_case(second=False):
    """66 x 4 x 5, winsz 2, vsmooth 2, smooth_nsq off, 9 directions (so that pi / 2 and pi are axis values), 4 speeds, 3 N^2 values:
    atmosphere(66, 4, 5, seed=3) with the PLANTS written over whole columns of rows PLANT_ROWS at PLANT_FACES (row r turns the
    list by 3 r, so every face meets two plants), and theta over UNSTABLE_COLUMNS / INVERSION_COLUMNS of every row.

    What lt_options_type can and cannot reach: with the default axes (dirmin 0, dirmax 2 pi, spdmin 0, nsq axis on
    log(min_stability) .. log(max_stability)) a direction is never above dirmax and never below 0, a speed never below 0, and the
    window mean of log(N^2) never above log(max_stability): bestpos == n on the direction and N^2 axes and match < d(1) on the
    direction and speed axes are unreachable, whatever the winds.  They are reachable with axes that end inside the data, which
    is what the second option set (PLANT_SECOND) is: lt_options_type lets every end of every axis be set."""
    c = case("planted second set" if second else "planted", *PLANT_SHAPE, 2, 2, 0, variable_N=True, smooth_nsq=False)
    c.update(hydrometeors="all", update=False, axes=(9, 4, 3), seed=3, plant=True, options=dict(PLANT_SECOND) if second else {})
    return c


def lt_options(c):
    nd, ns, nn = c["axes"]
    return lt_options_type(buffer=3, n_dir_values=nd, n_spd_values=ns, n_nsq_values=nn, stability_window_size=c["winsz"],
                           vert_smooth=c["vsmooth"], variable_N=c["variable_N"], smooth_nsq=c["smooth_nsq"], linear_contribution=0.8,
                           linear_update_fraction=0.3, **c["options"])


def inputs(c):
    """everything a run of the case needs: the atmosphere (hydrometeor fields the case does not have are removed), random tables,
    the axes and the oracle's option dict"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    a = atmosphere(nx, ny, nz, seed=c["seed"], moist=True)
    keep = {"all": ("cloud_water_mass", "cloud_ice_mass", "rain_mass", "snow_mass"), "none": (), "rain": ("rain_mass",)}[c["hydrometeors"]]
    for k in ("cloud_water_mass", "cloud_ice_mass", "rain_mass", "snow_mass"):
        if k not in keep:
            del a[k]
    if c.get("plant"):
        for r in PLANT_ROWS:
            for n, face in enumerate(PLANT_FACES):
                pu, pv = PLANTS[(n + 3 * r) % len(PLANTS)]
                a["u"][r, :, face] = f32(pu)
                a["v"][r, :, min(face, nx - 1)] = f32(pv)
        lev = np.arange(nz, dtype=np.float32)[None, :, None]
        a["potential_temperature"][:, :, UNSTABLE_COLUMNS] = f32(300.0) - f32(2.0) * lev
        a["potential_temperature"][:, :, INVERSION_COLUMNS] = f32(285.0) + f32(30.0) * lev
    lt = lt_options(c)
    nd, ns, nn = c["axes"]
    rng = np.random.default_rng(c["seed"] + 1000)
    ulut = (2.0 * rng.standard_normal((ny, nz, nx + 1, nn, nd, ns))).astype(np.float32)
    vlut = (2.0 * rng.standard_normal((ny + 1, nz, nx, nn, nd, ns))).astype(np.float32)
    lo, hi = lt.resolved()
    o = dict(variable_N=lt.variable_N, smooth_nsq=lt.smooth_nsq, N_squared=lt.N_squared, max_stability=lt.max_stability,
             min_stability=lt.min_stability, linear_contribution=lt.linear_contribution, linear_update_fraction=lt.linear_update_fraction)
    return dict(a=a, lt=lt, ulut=ulut, vlut=vlut, o=o, dirv=W.linear_space(lt.dirmin, lt.dirmax, nd),
                spdv=W.linear_space(lt.spdmin, lt.spdmax, ns), nsqv=W.linear_space(lo, hi, nn),
                hyd=tuple(a.get(k) for k in ("cloud_water_mass", "cloud_ice_mass", "rain_mass", "snow_mass")))


FIELDS = ("u", "v", "u_perturbation", "v_perturbation", "nsquared")
PASSES = 2                                   # the perturbation state carries from the first to the second (linear_update_fraction < 1)


def run(fn, c, x, states=None):
    """PASSES calls of fn (oracle.spatial_winds or spatial_winds above) on the inputs x: the five FIELDS after the last; with a
    list as `states` (the restatement only) the bracket state of every pass is appended"""
    a, lt = x["a"], x["lt"]
    u = a["u"].copy(); v = a["v"].copy(); up = np.zeros_like(u); vp = np.zeros_like(v)
    for _ in range(PASSES):
        kw = {}
        if states is not None:
            states.append({}); kw["state"] = states[-1]
        nsq = fn(u, v, a["potential_temperature"], a["exner"], a["z"], a["water_vapor"], x["hyd"], x["ulut"], x["vlut"], up, vp,
                 x["o"], x["dirv"], x["spdv"], x["nsqv"], lt.vert_smooth, lt.stability_window_size, **kw)
    return u, v, up, vp, nsq


def window_clips(nz, half, follow):
    """which ends of the vertical windows of a column of nz levels are cut off: a set out of "none", "top", "bottom", "both".
    follow=True: the window of :920-922 (it looks further down by what the top cut off); False: the j -+ winsz window of :1019-1020"""
    out = set()
    for j in range(1, nz + 1):
        top = j + half > nz
        bottom = (j - (half - (min(j + half, nz) - j)) < 1) if follow else (j - half < 1)
        out.add("both" if top and bottom else "top" if top else "bottom" if bottom else "none")
    return out


# ---- W3 -----------------------------------------------------------------------------------------------------------------------
DZ_LEVELS = np.array([40.0, 100.0, 200.0, 330.0], np.float32)     # sub-layers per level at minimum_layer_size 100: 1, 1, 2, 4
MINIMUM_LAYER_SIZE = 100.0
W3_AXES = (3, 2, 2)
W3_DX = 1500.0
# (nxg, nyg, buffer): transforms of 43 x 38, 42 x 39, 43 x 39 (43 is prime), 73 x 31 and 74 x 30; the last two are the single
# images with nx + 1 = 64 and 65
W3_SIZES = [(31, 26, 4), (30, 27, 4), (33, 29, 3), (63, 21, 3), (64, 20, 3)]
TILED = (31, 27, 4)                          # the constant-z table on every image of 2 x 2 and 3 x 2: a 43 x 39 transform
TILINGS = (4, 6)
VARYING = (31, 26, 4)                        # the space_varying_dz table on every image of 2 x 2
# (U, V, N^2, z_bottom, z_top) of test_gpu_winds.py::test_terrain_frequency_and_perturbation_vs_oracle
PERTURBATIONS = [(10.0, 5.0, 1e-4, 200.0, 450.0), (-7.0, 0.0, 3e-5, 0.0, 60.0), (0.0, 12.0, 6e-4, 1000.0, 1900.0), (3.0, -14.0, 1e-7, 50.0, 151.0)]


def transform_size(nxg, nyg, buffer):
    """linear_winds.f90:1201-1205: the buffer of the namelist, then two more cells, on every side"""
    return nxg + 2 * (buffer + 2), nyg + 2 * (buffer + 2)


def w3_options(buffer):
    nd, ns, nn = W3_AXES
    return lt_options_type(buffer=buffer, n_dir_values=nd, n_spd_values=ns, n_nsq_values=nn, minimum_layer_size=MINIMUM_LAYER_SIZE)


def layer_bounds():
    """z_bottom, z_top of the four layers over flat ground (linear_winds.f90:751-753)"""
    zc = np.cumsum(DZ_LEVELS, dtype=np.float32) - DZ_LEVELS / f32(2)
    return (zc - DZ_LEVELS / f32(2)).astype(f32), (zc + DZ_LEVELS / f32(2)).astype(f32)


def varying_layers(t):
    """SLEVE-like layers over the terrain t (nyg, nxg), thinner over high ground: (z_bottom, z_top) as (nyg, nz, nxg)"""
    nyg, nxg = t.shape
    squeeze = (1.0 - 0.25 * t / t.max()).astype(np.float32)
    dz3 = (DZ_LEVELS[None, :, None] * squeeze[:, None, :]).astype(np.float32)
    zb3 = np.concatenate([np.zeros((nyg, 1, nxg), np.float32), np.cumsum(dz3, axis=1, dtype=np.float32)[:, :-1]], axis=1)
    return zb3, (zb3 + dz3).astype(np.float32)


def varying_sublayers(zb3, zt3):
    """the number of sub-layer solutions per level of linear_perturbation_varyingz (linear_winds.f90:297-314)"""
    out = []
    for z in range(zb3.shape[1]):
        start_z, end_z = zb3[:, z].min(), zt3[:, z].max()
        step = min(f32(MINIMUM_LAYER_SIZE), (zt3[:, z] - zb3[:, z]).min())
        current_z = start_z + step / f32(2)
        n = 0
        while current_z < end_z:
            n += 1; current_z = current_z + step
        out.append(n)
    return out
