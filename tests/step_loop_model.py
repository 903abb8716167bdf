"""TEST INFRASTRUCTURE: the sub-step loop of src/main/time_step.f90:440-551 assembled on the host from the CPU oracle's operators, with
the microphysics gate of src/physics/mp_driver.f90:692-718 written from the reference (not from icar_amd/csrc/timestep.hip), and the
cases that tests/test_gpu_step_loop_gate.py, tests/test_gpu_step_failed_state.py and tests/test_step_loop_model_inputs.py share.

run() covers update_dt (cfl_strictness 3, the 120 s cap, the reference's stop below 0.1 s), the end-time clamp, the `enforce` flag of the
last two sub-steps, diagnostic_update, the gated microphysics (Thompson or mp_simple), advect (MPDATA or upwind), apply_forcing and
enforce_limits; a run of a given number of sub-steps (what icar_hip_step_n does: no clamp, no enforce_limits) likewise.  It keeps one
record per sub-step."""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

f32 = np.float32
ADV_ORDER = ["water_vapor", "cloud_water", "rain", "snow", "potential_temperature", "cloud_ice", "graupel", "ice_number", "rain_number"]
WINDS = ["u", "v", "w", "pressure"]
ADVECTED = {"thompson": ADV_ORDER, "simple": ADV_ORDER[:5]}
DEVICE_NAME = {"water_vapor": "water_vapor", "cloud_water": "cloud_water_mass", "rain": "rain_mass", "snow": "snow_mass",
               "potential_temperature": "potential_temperature", "cloud_ice": "cloud_ice_mass", "graupel": "graupel_mass",
               "ice_number": "cloud_ice_number", "rain_number": "rain_number", "u": "u", "v": "v", "w": "w", "pressure": "pressure"}
FORCED = [("water_vapor", True), ("potential_temperature", True), ("u", False), ("v", False), ("pressure", False), ("w", False)]
MPDATA, UPWIND = 2, 1                     # options%physics%advection (kADV_MPDATA, kADV_UPWIND): the oracle's scheme numbers too

# (dt, the gate was open, the microphysics' own time step or None, enforce_limits ran, dt was shortened to the end time)
SubStep = namedtuple("SubStep", "dt gate_open mp_dt enforce clamped")


class Gate:
    """mp(domain, options, dt_in, halo, subset), mp_driver.f90:692-718: last_model_time is a SAVE variable that starts at -999"""

    def __init__(self, update_interval=0.0, top_mp_level=0):
        self.upd = float(f32(update_interval))          # options%mp_options%update_interval reaches the driver as a REAL(4)
        self.top = int(top_mp_level)
        self.last = None                                # None: -999, no call yet

    def reset(self):
        self.last = None

    def call(self, now, dt, kte, halo):
        """One call at model time `now` with time step dt.  Returns (mp_dt, kte), mp_dt None when the call does nothing.  halo: the
        call is the pass over the halo strips, which leaves last_model_time alone (:711-713)."""
        dt4 = float(f32(dt))                            # real(dt%seconds()), time_step.f90:512
        if self.last is None:
            self.last = now - max(self.upd, dt4)        # :698-702
        if (now + dt4) - self.last < self.upd:          # :705
            return None, kte
        mp_dt = float(f32(now - self.last))             # :708
        if not halo:
            self.last = now                             # :711-713
        if 0 < self.top < kte:                          # :716-718
            kte = self.top
        return mp_dt, kte


def cfl_dt(oracle, s, c, factor=0.9):
    """compute_dt with cfl_strictness 3 (time_step.f90:264-313) as a REAL(4); update_dt caps it at 120 s (:417)"""
    return f32(factor) / f32(oracle.max_courant(s["u"], s["v"], s["w"], c["dz_levels"], float(c["dx"])))


def microphysics(oracle, scheme, s, c, diag, mp_dt, kte, acc, acc_snow):
    ny, nz, nx = c["dz_mass"].shape
    if scheme == "thompson":
        z = [np.zeros((ny, nx), f32) for _ in range(5)]
        oracle.thompson(s["water_vapor"], s["cloud_water"], s["rain"], s["cloud_ice"], s["snow"], s["graupel"], s["ice_number"],
                        s["rain_number"], s["potential_temperature"], diag["exner"], s["pressure"], c["dz_mass"], mp_dt, *z,
                        1, nx, 1, ny, 1, nz, 2, nx - 1, 2, ny - 1, 1, kte)
        acc += z[0]; acc_snow += z[2]
    else:
        rain = np.zeros((ny, nx), f32); snow = rain.copy()
        assert oracle.mp_simple(s["pressure"], s["potential_temperature"], diag["exner"], diag["density"], s["water_vapor"], s["cloud_water"],
                                s["rain"], s["snow"], rain, snow, mp_dt, c["dz_mass"], 2, nx - 1, 2, ny - 1, 1, kte) == 0
        acc += rain; acc_snow += snow


def run(oracle, c, dq, forced=FORCED, scheme="thompson", advection=MPDATA, end=None, nsteps=None, update_interval=0.0, top_mp_level=0,
        t0=0.0, mp_reset_at=(), state=None, acc0=None):
    """The loop from model time t0 until `end` (icar_hip_step) or for nsteps sub-steps (icar_hip_step_n).  c: the case (its constant
    members are read), dq: the forcing tendencies, state: the prognostic fields to start from (default: the case's), acc0: the accumulated
    precipitation to start from (default: none).  mp_reset_at:
    sub-step numbers (from 0) in front of which mp_init runs again (icar_hip_mp_reset).  Stops where update_dt would
    (dt < 0.1, time_step.f90:322-328): too_small then holds that dt.
    Returns s (the fields), diag (the last diagnostic_update), acc / acc_snow, t, n, dts, records, too_small."""
    assert (end is None) != (nsteps is None)
    names = ADVECTED[scheme]
    ny, nz, nx = c["dz_mass"].shape
    src = c if state is None else state
    s = {k: np.ascontiguousarray(src[k], f32).copy() for k in names + WINDS}
    acc = np.zeros((ny, nx), np.float64) if acc0 is None else np.array(acc0, np.float64); acc_snow = np.zeros((ny, nx), np.float64)
    oracle.set_math_mode(0)
    gate = Gate(update_interval, top_mp_level)
    t, n, dts, records, diag, too_small = float(t0), 0, [], [], None, None
    while (t < end) if nsteps is None else (n < nsteps):                                                # :462
        if n in mp_reset_at:
            gate.reset()
        dt4 = cfl_dt(oracle, s, c)                                                                      # :465
        if dt4 < f32(0.1):                                                                              # :322-328 `stop`
            too_small = float(dt4)
            break
        dt = min(float(dt4), 120.0)                                                                     # :417
        clamped = False
        if end is not None and t + dt > end:                                                            # :469-471
            dt = end - t; clamped = True
        enforce = end is not None and (end - t) < dt * 2
        dt4 = float(f32(dt))
        diag = oracle.diagnostic_update(s["pressure"], s["potential_temperature"], s["u"], s["v"], s["w"], c["dzdx"], c["dzdy"], c["jacobian"])   # :474
        if not dt > 1e-3:                                                                               # :483
            records.append(SubStep(dt, False, None, False, clamped)); t += dt; n += 1; dts.append(dt)
            continue
        # :512-523: mp(halo=1) on the strips, then mp(subset=1) on the interior; the scheme is column-local, so the two passes
        # with one mp_dt and one kte are one pass over its..ite, jts..jte
        strips = gate.call(t, dt, nz, halo=True)
        mp_dt, kte = gate.call(t, dt, nz, halo=False)
        assert strips == (mp_dt, kte), "the strips and the interior of one sub-step see one gate"
        if mp_dt is not None:
            microphysics(oracle, scheme, s, c, diag, mp_dt, kte, acc, acc_snow)
        q = np.stack([s[k] for k in names]).copy()
        oracle.advect(advection, q, s["u"], s["v"], s["w"], diag["density"], c["jacobian"], c["jacobian_u"], c["jacobian_v"], c["jacobian_w"],
                      c["advection_dz"], c["dz_levels"], float(c["dx"]), dt4)                            # :529
        for m, k in enumerate(names): s[k] = q[m].copy()
        for k, fb in forced:                                                                            # :534
            oracle.apply_forcing(s[k], dq[k], dt, int(fb), 1, 1, 1, 1)
        if enforce:                                                                                     # :537-539
            for k in names: oracle.enforce_limits(s[k])
        records.append(SubStep(dt, mp_dt is not None, mp_dt, enforce, clamped))
        t += dt; n += 1; dts.append(dt)                                                                 # :547
    return SimpleNamespace(s=s, diag=diag, acc=acc, acc_snow=acc_snow, t=t, n=n, dts=dts, records=records, too_small=too_small)


# ---- the cases of the gate and failed-state tests ----------------------------------------------------------------------------------
TILES = [(24, 10, 16), (67, 7, 9)]                      # those of tests/test_gpu_lazy_diagnostics.py
CONFIGS = {"thompson_mpdata": ("thompson", MPDATA), "mp_simple_upwind": ("simple", UPWIND)}
INTERVALS = {"always_open": 0.4, "opens_and_shuts": 2.5, "first_call_only": 10.0}     # update_interval in units of dt0
END = 8.4                                               # the end time of the icar_hip_step runs in units of dt0: the last sub-step is clamped
CLOCK_OFFSET = 1.0e6 + 0.25
RESET_AT, RESET_STEPS = 3, 6                            # step_n(3), icar_hip_mp_reset, step_n(3)
TOO_LARGE = 2000.0                                      # m/s2: dqdt of u that leaves |u| ~ 1e5 m/s after one sub-step of ~60 s
_chains = {}


def case(oracle, tile):
    from test_gpu_lazy_diagnostics import case as lazy_case
    return lazy_case(oracle, *tile)


def first_dt(oracle, c):
    """dt0: the first CFL step of the case"""
    return min(float(cfl_dt(oracle, c, c)), 120.0)


def interval(oracle, c, which):
    return float(f32(INTERVALS[which] * first_dt(oracle, c)))


def top_level(c):
    return c["nz"] - 4                                  # top_mp_level: a few levels below the top


def chain(oracle, tile, config, which="opens_and_shuts", top=False, t0=0.0, mode="step", reset=False):
    """the host chain of a gate case, computed once per session (nobody changes it)"""
    key = (tuple(tile), config, which, top, t0, mode, reset)
    if key not in _chains:
        c, dq = case(oracle, tile)
        scheme, adv = CONFIGS[config]
        kw = dict(scheme=scheme, advection=adv, update_interval=interval(oracle, c, which), top_mp_level=top_level(c) if top else 0, t0=t0)
        if mode == "step":
            kw["end"] = t0 + END * first_dt(oracle, c)
        else:
            kw["nsteps"] = RESET_STEPS
            kw["mp_reset_at"] = (RESET_AT,) if reset else ()
        _chains[key] = run(oracle, c, dq, **kw)
    return _chains[key]


def too_large_tendencies(dq, with_nan=False):
    """the tendencies of a case with a dqdt of u after whose first forcing the Courant maximum asks for dt < 0.1 s"""
    bad = dict(dq)
    bad["u"] = np.full(dq["u"].shape, TOO_LARGE, f32)
    if with_nan:
        bad["u"][3, 2, 5] = np.nan
    return bad


def end_time(oracle, c, t0=0.0):
    return t0 + END * first_dt(oracle, c)


# ---- the same cases on the device --------------------------------------------------------------------------------------------------
DEVICE_CONFIGS = {"thompson_mpdata": (MPDATA, 1), "mp_simple_upwind": (UPWIND, 2), "wsm6_mpdata": (MPDATA, 4)}      # (advection, microphysics)


def device_options(c, config, update_interval=0.0, top_mp_level=0):
    from test_gpu_lazy_diagnostics import options
    opt = options(c, *DEVICE_CONFIGS[config])
    opt.mp_options.update_interval = update_interval; opt.mp_options.top_mp_level = top_mp_level
    return opt


def device_domain(c, dq, opt, halo=None):
    """a single-image domain_t holding the case and its tendencies, MPDATA in the reference's operation order (bit for bit against the
    oracle); halo: the grid's halo width (default 1)"""
    from icar_amd.advection import adv_init
    from icar_amd.capi import lib, check
    from icar_amd.domain import domain_t
    from icar_amd.grid import grid_t
    from icar_amd.microphysics import mp_init
    d = domain_t(grid_t().set_grid_dimensions(c["nx"], c["ny"], c["nz"], 1, 1, halo_width=halo), device=0, dx=float(c["dx"]))
    d.load_case(c)
    check(lib().icar_hip_mpdata_exact(d.ctx, 1), "mpdata_exact")
    mp_init(opt, d); adv_init(d, opt)
    for k, a in dq.items():
        d.set_dqdt(k, a)
    return d
