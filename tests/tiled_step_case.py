"""The sub-step loop of time_step.f90:462-539 on the host tiles of a decomposition, with a live halo exchange between them (TEST ONLY).

The CPU chains of the single-image step tests (test_gpu_cu_step.py, test_gpu_tiedtke_step.py, test_gpu_nsas_step.py, test_gpu_ysu_step.py,
test_gpu_lsm_noah_step.py) lifted into one object, TileChain, that runs on ONE image's memory (ims..ime, jms..jme, halos included) with
that image's tile bounds and boundary flags, in three phases per sub-step so that a driver can put what the images do together between
them:

    local_dt()                      the oracle's max_courant on the tile's memory        -> co_min over the images, the 120 s cap, the clamp
    open(dt, t)                     diagnostic_update, the 10 m diagnostics, [rad] [lsm] [pbl] [convect] on (its, ite, jts, jte), mp(halo=1)
                                    -> halo_send: the edge planes are packed HERE (with a halo wider than 1 the second plane has not seen
                                       the microphysics yet, as in the reference)
    interior()                      mp(subset=1)
                                    -> halo_retrieve
    close(dt, enforce)              advect, the forcing from the tile's own cut of the dq arrays, enforce_limits

run() drives a list of chains: one chain and a HaloComm over gloo in a worker of tests/test_gpu_multirank_physics.py, every chain of a
decomposition in one process with LocalExchange (the same HostTile pack / unpack, delivered by hand) in tests/test_multirank_physics_inputs.py.
dt never comes from the device.

The case (whole_case) is the one of the issue "Test every physics slot of the time step on tiled runs with live halos": 40 x 28 x 12, a hill,
noisy winds, forced u / v / w / pressure / qv / theta, a land-and-water mask, latitude and longitude, the radiation calendar anchor."""
import ctypes

import numpy as np

f32 = np.float32
NXG, NYG, NZ = 40, 28, 12
# fixed so that the restatements meet every condition of tests/test_multirank_physics_inputs.py (that file asserts them)
SEED, HILL, MOIST, DX, WATER = 61, 900.0, 1.35, 2000.0, 0.5
# What the issue's sketch of the case could not give at 40 x 28 x 12, and what was changed for it (the conditions themselves stand):
#  * with icar_amd.ideal's default layers the top of 12 levels lies at 4 km, where p > 0.7 p_sfc in every column: NSAS's kbmax, kbm and kmax
#    are then the level count everywhere and a tile row has the limits of the whole row.  LEVELS keeps the thin layers near the ground
#    (pbl_simple's sub-step counts need them) and reaches 7.5 km; the centre of level 9 lies where p = 0.7 p_sfc, so that kbm is 10 over
#    the hill and 9 beside it;
#  * icar_amd.ideal's hill is symmetric about the middle of the domain, where the 2 x 2 and 4 x 2 decompositions cut it: both halves of a
#    row then hold the row's highest column.  The hill stands at the western edge instead (HILL_AT, in fractions of nx and ny), inside the
#    westernmost tiles;
#  * kbm only bounds the search for the level of the largest moist static energy, which the case's sounding has at the ground.  ALOFT_SHARE
#    of the columns therefore carry a saturated layer from level ALOFT[0] + 1 (the level kbm = 10 lets in and kbm = 9 keeps out) up over
#    ALOFT[1] more levels, warmed by ALOFT_WARM K in its lowest ALOFT[2] levels, over air dried to ALOFT_DRY of its vapour.
LEVELS = [50, 75, 125, 200, 300, 400, 550, 700, 1200, 1100, 1300, 1500]
HILL_AT, HILL_HALF_WIDTH, SFC_LAYER = (0.03, 0.32), (0.27, 0.38), 400.0
ALOFT, ALOFT_SHARE, ALOFT_RH, ALOFT_DRY, ALOFT_WARM = (9, 3, 2), 0.4, 1.02, 0.35, 8.0
assert len(LEVELS) == NZ
GREGORIAN = 0
ANCHOR = (GREGORIAN, -(80 * 86400.0 + 30000.0), 365.0, 365.0)
SCALARS = ["water_vapor", "cloud_water", "rain", "snow", "potential_temperature", "cloud_ice", "graupel", "ice_number", "rain_number"]   # advection order
FORCED = [("water_vapor", True), ("potential_temperature", True), ("u", False), ("v", False), ("pressure", False), ("w", False)]
STEPS = (2.2, 4.4)                 # the two step() calls end at these multiples of the first CFL step
LSM_INTERVAL = 1.5                 # lsm's update interval in CFL steps: the gate opens, stays shut and opens again

# the rows of the issue's table; star: no row-coupled scheme and upwind, so the tiled run equals the one-image run in every owned cell
CONFIGS = {
    "ysu+bmj":          dict(lsm="basic", pbl="ysu", cu="bmj", mp="thompson", adv="upwind", halo=None, star=True),
    "noah+ysu":         dict(lsm="noah", pbl="ysu", cu="none", mp="mp_simple", adv="upwind", halo=None, star=True),
    "simple+tiedtke":   dict(lsm="basic", pbl="simple", cu="tiedtke", mp="thompson", adv="upwind", halo=None, star=False),
    "ysu+nsas+mpdata":  dict(lsm="basic", pbl="ysu", cu="nsas", mp="thompson", adv="mpdata-exact", halo=None, star=False),
    "ysu+nsas@h2":      dict(lsm="basic", pbl="ysu", cu="nsas", mp="thompson", adv="upwind", halo=2, star=False),
}
for _c in CONFIGS.values():
    _c["rad"] = "simple"


# ---- the case ------------------------------------------------------------------------------------------------------------------------
def whole_case(orc, cfg, tab=None):
    """(c, dq, nc): the whole domain, the rates of the forced fields, and -- lsm == "noah" -- the Noah case on the same cells (its xland is
    then the land mask).  The same arrays on every image: everything comes from SEED."""
    import pbl_oracle as P
    nx, ny = NXG, NYG
    levels = np.asarray(LEVELS, f32)
    nz = len(levels)
    lsm = cfg["lsm"]
    ALOFT_LEVEL, ALOFT_DEPTH, ALOFT_WARM_LEVELS = ALOFT
    from icar_amd import ideal
    fi = np.clip((np.arange(nx) / (nx - 1) - HILL_AT[0]) / HILL_HALF_WIDTH[0], -1.0, 1.0)
    fj = np.clip((np.arange(ny) / (ny - 1) - HILL_AT[1]) / HILL_HALF_WIDTH[1], -1.0, 1.0)
    terrain = (HILL * 0.25 * (1.0 + np.cos(np.pi * fi))[None, :] * (1.0 + np.cos(np.pi * fj))[:, None]).astype(f32)
    c = ideal.make_case(nx, ny, nz, terrain=terrain, noise=0.03, seed=SEED, n_hydro=1, uniform_dz=levels, dx=DX)      # (np.full(nz, levels): the thicknesses as given)
    rng = np.random.default_rng(SEED + 1000)
    c["z"], _ = P.mass_heights(c)
    c["land_mask"] = np.where(rng.random((ny, nx)) < WATER, 2, 1).astype(np.int32)
    c["potential_temperature"] = (c["potential_temperature"] + (0.5 * rng.standard_normal((ny, nz, nx))).astype(f32)).astype(f32)
    c["water_vapor"] = (c["water_vapor"] * f32(MOIST)).astype(f32)
    # the saturated layer aloft (ALOFT above): there the moist static energy is largest, and whether the level is inside 1..kbm is the row's matter
    aloft = (rng.random((ny, nx)) < ALOFT_SHARE)
    k = np.arange(nz)[None, :, None]
    layer = aloft[:, None, :] & (k >= ALOFT_LEVEL) & (k < ALOFT_LEVEL + ALOFT_WARM_LEVELS)
    c["potential_temperature"] = (c["potential_temperature"] + np.where(layer, f32(ALOFT_WARM), f32(0))).astype(f32)
    T = c["potential_temperature"].astype(np.float64) * c["exner"]
    qs = ideal.sat_mr(T, c["pressure"])
    c["water_vapor"] = np.where(aloft[:, None, :] & (k < ALOFT_LEVEL), ALOFT_DRY * c["water_vapor"],
                                np.where(aloft[:, None, :] & (k <= ALOFT_LEVEL + ALOFT_DEPTH), ALOFT_RH * qs, c["water_vapor"])).astype(f32)
    rng = np.random.default_rng(SEED)
    c["u"] = (c["u"] + 6.0 * rng.standard_normal((ny, nz, 1))).astype(f32)
    c["v"] = (c["v"] + 1.5 * rng.standard_normal((1, nz, nx))).astype(f32)
    c["w"] = orc.balance_uvw(c["u"], c["v"], c["jacobian_u"], c["jacobian_v"], c["jacobian_w"], c["advection_dz"], float(c["dx"]))
    c["dzdx"] = (0.05 * rng.standard_normal(c["u"].shape)).astype(f32)
    c["dzdy"] = (0.05 * rng.standard_normal(c["v"].shape)).astype(f32)
    c["latitude"] = (np.linspace(-60.0, 60.0, ny)[:, None] + np.zeros((1, nx))).astype(f32)
    c["longitude"] = (np.linspace(-180.0, 360.0, nx)[None, :] + rng.uniform(-2, 2, (ny, nx))).clip(-180, 360).astype(f32)
    T0 = (c["potential_temperature"] * c["exner"])[:, 0, :]
    c["sst"] = (T0 + rng.uniform(-5, 5, (ny, nx))).astype(f32)
    c["skin_temperature"] = (T0 + rng.uniform(-2, 2, (ny, nx))).astype(f32)
    c["sensible_heat"] = rng.uniform(-50, 300, (ny, nx)).astype(f32)
    c["latent_heat"] = rng.uniform(-20, 200, (ny, nx)).astype(f32)
    c["roughness_z0"] = (10.0 ** rng.uniform(-3, -0.5, (ny, nx))).astype(f32)
    c["dz_interface"] = c["dz_mass"].copy()
    c["ground_surf_temperature"] = (c["skin_temperature"] + rng.normal(0, 0.5, (ny, nx))).astype(f32)
    c["znu"] = ((np.arange(nz, 0, -1) - 0.5) / nz).astype(f32)
    dq = {"water_vapor": 1e-8, "potential_temperature": 1e-4, "u": 5e-4, "v": -5e-4, "pressure": 1e-3, "w": 2e-6}
    dq = {k: (sc * rng.standard_normal(c[k].shape)).astype(f32) for k, sc in dq.items()}
    dq.update(nx=nx, ny=ny)
    nc = None
    if lsm == "noah":
        import noah_oracle as N
        tm = float(T0.mean())
        nc = N.make_case(tab, nx=nx, ny=ny, seed=SEED, dt=600.0, t=[tm], sw=[300], pr=[[0.5, 2.0]], snow0=0.3, soil_t=tm - 1.0)
        c["land_mask"] = nc["xland"].astype(np.int32)
        c["roughness_z0"] = nc["z00"].copy()
    return c, dq, nc


def first_dt(orc, c):
    return min(float(f32(0.9) / f32(orc.max_courant(c["u"], c["v"], c["w"], c["dz_levels"], float(c["dx"])))), 120.0)


def schedule(orc, c):
    """(update interval of lsm in seconds, the end times of the two step() calls) from the whole domain's first CFL step"""
    dt0 = first_dt(orc, c)
    return max(int(LSM_INTERVAL * dt0), 1), tuple(m * dt0 for m in STEPS)


def grid_of(world, image, halo=None, nz=NZ):
    from icar_amd.grid import grid_t
    return grid_t().set_grid_dimensions(NXG, NYG, nz, world, image, halo_width=halo)


def cut(case, g):
    from icar_amd.ideal import cut_tile
    return cut_tile(case, g)


def advected(cfg):
    """the case keys of the advected (= exchanged) scalars, in advection order, as the var requests of the configuration's schemes make them"""
    thompson = ["water_vapor", "cloud_water", "rain", "snow", "potential_temperature", "cloud_ice", "graupel", "ice_number", "rain_number"]
    simple = ["water_vapor", "cloud_water", "rain", "snow", "potential_temperature"] + (["cloud_ice"] if cfg["pbl"] == "ysu" else [])
    return thompson if cfg["mp"] == "thompson" else simple


def local_bounds(g):
    """the tile bounds in the 1-based indices of the image's own memory"""
    return g.its - g.ims + 1, g.ite - g.ims + 1, g.jts - g.jms + 1, g.jte - g.jms + 1


def mp_regions(its, ite, jts, jte):
    """mp(halo=1): process_halo's four strips (mp_driver.f90:609-658); mp(subset=1): the rest (:728-737).  Empty regions are left out."""
    strips = [(its, its, jts, jte), (ite, ite, jts, jte), (its + 1, ite - 1, jts, jts), (its + 1, ite - 1, jte, jte)]
    inner = [(its + 1, ite - 1, jts + 1, jte - 1)]
    live = lambda r: [t for t in r if t[1] >= t[0] and t[3] >= t[2]]
    return live(strips), live(inner)


# ---- one image ------------------------------------------------------------------------------------------------------------------------
class TileChain:
    def __init__(self, orc, cfg, c, dq, g, ui, nc=None, tab=None):
        """c, dq, nc: this image's cuts (cut()); g: its grid_t; ui: lsm's update interval in seconds"""
        self.orc, self.cfg, self.c, self.dq, self.g, self.ui, self.nc, self.tab = orc, cfg, c, dq, g, ui, nc, tab
        self.ny, self.nz, self.nx = c["z"].shape
        ny, nz, nx = self.ny, self.nz, self.nx
        self.tile = local_bounds(g)
        self.adv = advected(cfg)
        self.s = {k: c[k].copy() for k in SCALARS + ["u", "v", "w", "pressure"]}
        import ra_oracle as R
        self.rad2d = {k: np.full((ny, nx), R.SENTINEL, f32) for k in R.OUTPUTS[1:]}
        self.acc = np.zeros((ny, nx), np.float64)
        self.t_mp = None
        self.nzl = None                                                          # apply_fluxes' SAVE variable nz
        self.gates, self.convecting, self.pbl_rows = [], [], []                  # per sub-step: the lsm gate, the tile's convecting columns, pbl_simple's sub-step counts
        lm = c["land_mask"]
        self.xland = np.where((lm == 0) | (lm == 2), 2.0, lm).astype(f32)
        if cfg["lsm"] == "noah":
            self._init_noah()
        else:
            self.sfc = {k: c[k].copy() for k in ("roughness_z0", "skin_temperature", "sensible_heat", "latent_heat")}
            self.sfc.update(qsfc=c["water_vapor"][:, 0, :].copy(), qfx=np.zeros((ny, nx), f32), last_model_time=-999.0)
        self.sfc.update(u_10m=np.zeros((ny, nx), f32), v_10m=np.zeros((ny, nx), f32), ustar=np.full((ny, nx), 0.1, f32))
        if cfg["pbl"] == "ysu":
            import ysu_oracle as Y
            A = Y.init_arrays(c)                                                 # pbl_init, from the roughness of the start
            for k in Y.TEND + ["exch_h"]:
                A[k] = np.zeros((ny, nz, nx), f32)
            for k in ("hpbl", "psim", "psih", "regime", "ri", "windspd"):
                A[k] = np.zeros((ny, nx), f32)
            A["kpbl"] = np.zeros((ny, nx), np.int32)
            self.ys = A
        cu = cfg["cu"]
        if cu == "bmj":
            import bmj_oracle as B
            self.cu = dict(cldefi=np.full((ny, nx), B.AVGEFI(), f32), tend_th=np.zeros((ny, nz, nx), f32), tend_qv=np.zeros((ny, nz, nx), f32))
            for k in ("raincv", "cutop", "cubot", "accumulated_convective_pcp"):
                self.cu[k] = np.zeros((ny, nx), f32)
        elif cu == "tiedtke":
            import tiedtke_oracle as T
            self.cu = {k: np.zeros((ny, nz, nx), f32) for k in T.TEND}
            self.cu.update(raincv=np.zeros((ny, nx), f32), pratec=np.zeros((ny, nx), f32), accumulated_convective_pcp=np.zeros((ny, nx), f32),
                           ktype=np.zeros((ny, nx), np.int32), diag=np.zeros((ny, nx), np.int32))
        elif cu == "nsas":
            import nsas_oracle as NS
            self.cu = {k: np.zeros((ny, nz, nx), f32) for k in NS.TEND}
            self.cu.update({k: np.zeros((ny, nx), f32) for k in NS.OUT2 + ["accumulated_convective_pcp"]})
            self.cu.update(diag=np.zeros((ny, nx), np.int32), limits=np.zeros((ny, 3), np.int32), own=np.zeros((ny, nx, 3), np.int32))

    # -- Noah: lsm_init on the image's memory and the coupling (test_gpu_lsm_noah_step.py)
    def _init_noah(self):
        import lsm_noah_driver_oracle as LN
        import noah_oracle as N
        c, nc, s, orc = self.c, self.nc, self.s, self.orc
        ny, nx = self.ny, self.nx
        A = LN.state0(nc)
        for k, m in (("tsk", "skin_temperature"), ("hfx", "sensible_heat"), ("lh", "latent_heat"), ("znt", "roughness_z0")):
            A[k] = c[m].copy()
        A["qsfc"] = c["water_vapor"][:, 0, :].copy()                             # lsm_driver.f90:568
        N.lsm_init(self.tab, nc, A)
        self.noah = A
        self.sfc = dict(roughness_z0=A["znt"], skin_temperature=A["tsk"], sensible_heat=A["hfx"], latent_heat=A["lh"], qsfc=A["qsfc"], qfx=A["qfx"])
        mask = np.ascontiguousarray(c["land_mask"], f32)
        self.drv = dict(nx=nx, ny=ny, xland=mask, terrain=c["terrain"], z1=np.ascontiguousarray(c["z"][:, 0, :]), max_swe=f32(25.0),
                        update_interval=self.ui, precip0=self.acc)
        self.noah_static = {k: nc[k] for k in ("nx", "ny", "ivgtyp", "isltyp", "vegfra", "tmn", "shdmin", "shdmax", "fndsnowh")}
        self.noah_static["xland"] = mask
        orc.set_math_mode(0)
        diag = orc.diagnostic_update(s["pressure"], s["potential_temperature"], s["u"], s["v"], s["w"], c["dzdx"], c["dzdy"], c["jacobian"])
        F0 = dict(t=np.ascontiguousarray(diag["temperature"][:, 0, :]), qv=np.ascontiguousarray(s["water_vapor"][:, 0, :]))
        ci, p_ = ctypes.c_int, lambda a: a.ctypes.data_as(ctypes.c_void_p)
        LN.lib().lnd_oracle_couple(ci(nx), ci(ny), p_(A["znt"]), p_(self.drv["z1"]), p_(self.drv["terrain"]), p_(F0["t"]), p_(F0["qv"]), p_(self.acc),
                                   p_(A["z0"]), p_(A["chs"]), p_(A["chs2"]), p_(A["rainbl_step"]), p_(A["rainbl8"]), p_(A["t2"]), p_(A["q2"]),
                                   p_(A["z_atm"]), p_(A["lnz"]), p_(A["base"]))

    def local_dt(self):
        s, c = self.s, self.c
        return float(f32(0.9) / f32(self.orc.max_courant(s["u"], s["v"], s["w"], c["dz_levels"], float(c["dx"]))))

    def _mp(self, regions):
        s, c, orc, nx, ny, nz = self.s, self.c, self.orc, self.nx, self.ny, self.nz
        g = self.g
        for its, ite, jts, jte in regions:
            if self.cfg["mp"] == "thompson":
                z = [np.zeros((ny, nx), f32) for _ in range(5)]
                orc.thompson(s["water_vapor"], s["cloud_water"], s["rain"], s["cloud_ice"], s["snow"], s["graupel"], s["ice_number"], s["rain_number"],
                             s["potential_temperature"], self.diag["exner"], s["pressure"], c["dz_mass"], self.mp_dt, *z,
                             g.ids - g.ims + 1, g.ide - g.ims + 1, g.jds - g.jms + 1, g.jde - g.jms + 1, 1, nz, its, ite, jts, jte, 1, nz)
                self.acc += z[0]
            else:
                rain, snow = np.zeros((ny, nx), f32), np.zeros((ny, nx), f32)
                err = orc.mp_simple(s["pressure"], s["potential_temperature"], self.diag["exner"], self.diag["density"], s["water_vapor"], s["cloud_water"],
                                    s["rain"], s["snow"], rain, snow, self.mp_dt, c["dz_mass"], its, ite, jts, jte, 1, nz)
                assert err == 0
                self.acc += rain

    def open(self, dt, t):
        import ra_oracle as R
        import sfc_oracle as S
        from icar_amd.constants import kWATER_SIMPLE, kLSM_BASIC
        s, c, orc, cfg, nx, ny, nz = self.s, self.c, self.orc, self.cfg, self.nx, self.ny, self.nz
        tile = self.tile
        its, ite, jts, jte = tile
        cf = lambda a: np.ascontiguousarray(a, f32)
        dt4 = float(f32(dt))
        orc.set_math_mode(0)
        diag = self.diag = orc.diagnostic_update(s["pressure"], s["potential_temperature"], s["u"], s["v"], s["w"], c["dzdx"], c["dzdy"], c["jacobian"])   # :474
        sfc = self.sfc
        cc = dict(density=diag["density"], exner=diag["exner"], temperature=diag["temperature"], u_mass=diag["u_mass"], v_mass=diag["v_mass"],
                  surface_pressure=diag["surface_pressure"], z=c["z"], terrain=c["terrain"], sst=c["sst"], land_mask=c["land_mask"],
                  dz_interface=c["dz_interface"], watersurface=kWATER_SIMPLE, landsurface=kLSM_BASIC, sfc_layer_thickness=SFC_LAYER,
                  sh_feedback_fraction=0.625, lh_feedback_fraction=1.0, update_interval=self.ui, kts=1)
        A = dict(sfc, potential_temperature=s["potential_temperature"], water_vapor=s["water_vapor"])
        S.diag_10m(cc, A)                                                                               # :143-161
        if dt > 1e-3:                                                                                   # :483
            cal, start, yd, nyd = ANCHOR                                                                # :488 rad
            D = (t - start) / 86400.0
            D, yd = (D - yd, nyd) if D >= yd else (D, yd)
            Ar = dict(self.rad2d); Ar["potential_temperature"] = s["potential_temperature"]
            inputs = dict(s); inputs.update(exner=diag["exner"], latitude=c["latitude"], longitude=c["longitude"])
            R.ra_simple(Ar, inputs, D, yd, cal, dt4, its, ite, jts, jte, 1, nz)
            if self.nzl is None:
                self.nzl = S.layers(cc)                                                                 # over this image's memory, once
            if cfg["lsm"] == "noah":                                                                    # :491 lsm, the Noah branch
                import lsm_noah_driver_oracle as LN
                import noah_oracle as N
                NA, drv = self.noah, self.drv
                is_open, lsm_dt = LN.gate(drv, NA, t)
                self.gates.append(is_open)
                if is_open:
                    lvl = lambda a, k: np.ascontiguousarray(a[:, k, :])
                    F = dict(qv=lvl(s["water_vapor"], 0), t=lvl(diag["temperature"], 0), p8w1=lvl(diag["pressure_interface"], 0),
                             p8w2=lvl(diag["pressure_interface"], 1), swdown=self.rad2d["shortwave"], glw=self.rad2d["longwave"], u10=sfc["u_10m"],
                             v10=sfc["v_10m"], psfc=diag["surface_pressure"], precip=self.acc)
                    drv["forcing"] = [F]
                    LN.pre(drv, NA, 0)
                    N.lsm_noah(self.tab, dict(self.noah_static, forcing=[F]), NA, 0, tile, lsm_dt)
                    LN.post(drv, NA, 0, tile)
            else:                                                                                       # :491 lsm basic + water_simple
                is_open = S.gate(cc, A, t)
                self.gates.append(is_open)
                if is_open: S.water_simple(cc, A)
                sfc["last_model_time"] = A["last_model_time"]
            S.apply_fluxes(cc, A, dt4, tile=tile, nzl=self.nzl)
            if cfg["pbl"] == "simple":                                                                  # :494 pbl
                import pbl_oracle as P
                nsub, _ = P.simple_pbl({k: s[k] for k in P.SCALARS}, diag["u_mass"], diag["v_mass"], diag["exner"], diag["density"], c["z"],
                                       c["dz_mass"], c["terrain"], c["land_mask"], its, ite, jts, jte, 1, nz, dt4)
                self.pbl_rows.append(nsub.copy())
            elif cfg["pbl"] == "ysu":
                import ysu_oracle as Y
                yc = dict(z=c["z"], dx=c["dx"], terrain=c["terrain"], land_mask=c["land_mask"], dz_interface=c["dz_interface"],
                          ground_surf_temperature=c["ground_surf_temperature"], pressure=s["pressure"], exner=diag["exner"],
                          pressure_interface=diag["pressure_interface"], surface_pressure=diag["surface_pressure"], u_mass=diag["u_mass"], v_mass=diag["v_mass"])
                yc.update({k: A[k] for k in ("u_10m", "v_10m", "ustar", "roughness_z0", "skin_temperature", "sensible_heat", "latent_heat")})
                yc = {k: (np.ascontiguousarray(v, np.int32 if k == "land_mask" else f32) if isinstance(v, np.ndarray) else v) for k, v in yc.items()}
                ys = self.ys
                YA = dict(ys, temperature=cf(diag["temperature"]), water_vapor=s["water_vapor"], cloud_water=s["cloud_water"],
                          cloud_ice=s["cloud_ice"], potential_temperature=s["potential_temperature"])
                Y.run_sfc(yc, YA)
                Y.run_ysu(yc, YA, dt4, tile=tile)
                Y.run_apply(yc, YA, dt4)
                ys.update({k: YA[k] for k in ys})
            cu = cfg["cu"]                                                                              # :509 convect
            Acu = None
            if cu != "none":
                Acu = dict(self.cu, temperature=cf(diag["temperature"]), water_vapor=s["water_vapor"], potential_temperature=s["potential_temperature"],
                           cloud_water=s["cloud_water"], cloud_ice=s["cloud_ice"], accumulated_precipitation=self.acc)
            if cu == "bmj":
                import bmj_oracle as B
                ccu = dict(density=diag["density"], exner=diag["exner"], pressure=s["pressure"], pressure_interface=diag["pressure_interface"],
                           dz_interface=c["dz_interface"], land_mask=c["land_mask"], tendency_fraction=1.0, fractions=[1.0] * 4)
                kind = B.convect(ccu, Acu, dt4, tile=tile)
                self.convecting.append(int((kind[jts - 1:jte, its - 1:ite] != B.NONE).sum()))
            elif cu == "tiedtke":
                import tiedtke_oracle as T
                ccu = dict(density=diag["density"], exner=diag["exner"], pressure=s["pressure"], pressure_interface=diag["pressure_interface"],
                           dz_interface=c["dz_interface"], w_real=diag["w_real"], xland=self.xland, znu=c["znu"])
                T.convect(ccu, Acu, dt4, tile)
                self.convecting.append(int((self.cu["ktype"][jts - 1:jte, its - 1:ite] != 0).sum()))
            elif cu == "nsas":
                import nsas_oracle as NS
                ccu = dict(density=cf(diag["density"]), exner=cf(diag["exner"]), pressure=cf(s["pressure"]), pressure_interface=cf(diag["pressure_interface"]),
                           dz_interface=cf(c["dz_interface"]), w_real=cf(diag["w_real"]), u_mass=cf(diag["u_mass"]), v_mass=cf(diag["v_mass"]),
                           xland=self.xland, sensible_heat=cf(A["sensible_heat"]), latent_heat=cf(A["latent_heat"]), hpbl=cf(self.ys["hpbl"]), dx=c["dx"])
                NS.convect(ccu, Acu, dt4, tile)
                self.convecting.append(int((self.cu["diag"][jts - 1:jte, its - 1:ite] & (NS.D_DEEP_RAIN | NS.D_SHALLOW) != 0).sum()))
            if Acu is not None:
                for k in ("water_vapor", "potential_temperature", "cloud_water", "cloud_ice"):
                    s[k] = Acu[k]
        self.mp_dt = dt4 if self.t_mp is None else float(f32(t - self.t_mp)); self.t_mp = t
        strips, self._inner = mp_regions(*tile)
        self._mp(strips)                                                                                # :512 mp(halo=1)

    def interior(self):
        self._mp(self._inner)                                                                           # :523 mp(subset=1)

    def close(self, dt, enforce):
        s, c, orc, g = self.s, self.c, self.orc, self.g
        dt4 = float(f32(dt))
        q = np.stack([s[n] for n in self.adv]).copy()                                                   # :529 advect
        orc.advect(1 if self.cfg["adv"] == "upwind" else 2, q, s["u"], s["v"], s["w"], self.diag["density"], c["jacobian"], c["jacobian_u"],
                   c["jacobian_v"], c["jacobian_w"], c["advection_dz"], c["dz_levels"], float(c["dx"]), dt4)
        for m, n in enumerate(self.adv): s[n] = q[m].copy()
        for n, fb in FORCED:                                                                            # :534 apply_forcing, this image's edges
            orc.apply_forcing(s[n], self.dq[n], dt, int(fb), int(g.west_boundary), int(g.east_boundary), int(g.south_boundary), int(g.north_boundary))
        if enforce:                                                                                     # :537-539
            for n in self.adv: orc.enforce_limits(s[n])


# ---- the exchange -----------------------------------------------------------------------------------------------------------------------
class LocalExchange:
    """halo_send / halo_retrieve between the chains of one process: HostTile's pack and unpack (tests/host_tile.py), each message handed
    to the neighbour's inbox, unpacked north, south, east, west as the reference retrieves (exchangeable_obj.f90:138-151)"""
    OPPOSITE = {0: 1, 1: 0, 2: 3, 3: 2}
    NAMES = {0: "north", 1: "south", 2: "east", 3: "west"}

    def __init__(self, chains):
        from host_tile import HostTile
        self.chains = chains
        self.tiles = [HostTile(ch.g, None) for ch in chains]
        self.peers = []
        for r, ch in enumerate(chains):
            nb = ch.g.neighbors(r + 1)
            self.peers.append({d: nb[n] - 1 for d, n in self.NAMES.items() if nb[n] is not None})
        self.inbox = [dict() for _ in chains]

    def co_min(self, values):
        return min(values)

    def send(self):
        for r, (ch, tile) in enumerate(zip(self.chains, self.tiles)):
            tile.f = ch.s
            h = ch.g.halo_size
            for d, peer in self.peers[r].items():
                buf = tile.new_buffer(tile.halo_count(d, h) * len(ch.adv))
                tile.halo_pack(d, h, ch.adv, buf)
                self.inbox[peer][self.OPPOSITE[d]] = buf

    def retrieve(self):
        for r, (ch, tile) in enumerate(zip(self.chains, self.tiles)):
            tile.f = ch.s
            for d in sorted(self.inbox[r]):
                tile.halo_unpack(d, ch.g.halo_size, ch.adv, self.inbox[r][d])
            self.inbox[r] = {}


class GlooExchange:
    """the same through icar_amd.halo.HaloComm over a torch.distributed (gloo) group: one chain per process"""
    def __init__(self, chain, image, group=None):
        from host_tile import HostTile
        from icar_amd.halo import HaloComm
        self.chain, self.group = chain, group
        self.tile = HostTile(chain.g, None)
        self.comm = HaloComm(chain.g, image, group=group)

    def co_min(self, values):
        from icar_amd.halo import co_min
        return co_min(values[0], group=self.group)

    def send(self):
        self.tile.f = self.chain.s
        self.comm.send(self.tile, self.chain.adv)

    def retrieve(self):
        self.tile.f = self.chain.s
        self.comm.retrieve(self.tile, self.chain.adv)


def run(chains, ends, ex, t=0.0):
    """time_step.f90:440-551 for every end time in turn.  Returns (the sub-step count of each call, the model time after each call)."""
    counts, clocks = [], []
    for end in ends:
        n = 0
        while t < end:                                                                                  # :462
            dt = min(ex.co_min([ch.local_dt() for ch in chains]), 120.0)                                # :413 co_min, :417
            if t + dt > end: dt = end - t                                                               # :469-471
            enforce = (end - t) < dt * 2
            for ch in chains: ch.open(dt, t)
            ex.send()                                                                                   # :515
            for ch in chains: ch.interior()
            ex.retrieve()                                                                               # :526
            for ch in chains: ch.close(dt, enforce)
            t += dt; n += 1                                                                             # :547
        counts.append(n); clocks.append(t)
    return counts, clocks


def chains_of(orc, cfg, world, c, dq, nc=None, tab=None, ui=None):
    """every image's chain of a decomposition (world = 1: the one-image run)"""
    import copy
    out = []
    for image in range(1, world + 1):
        g = grid_of(world, image, cfg["halo"], c["nz"])
        out.append(TileChain(orc, cfg, cut(c, g), cut(dq, g), g, ui, None if nc is None else copy.deepcopy(cut(nc, g)), tab))
    return out


def owned(g):
    """(slices of the image's memory, slices of the whole domain) of the owned cells, rows first"""
    return ((slice(g.jts - g.jms, g.jte - g.jms + 1), slice(g.its - g.ims, g.ite - g.ims + 1)), (slice(g.jts - 1, g.jte), slice(g.its - 1, g.ite)))


# ---- the device ---------------------------------------------------------------------------------------------------------------------------
def options(cfg, c, ui):
    from icar_amd import radiation, pbl, surface, convection
    from icar_amd.options import options_t
    from icar_amd.microphysics import mp_var_request
    from icar_amd import constants as K
    opt = options_t()
    opt.physics.advection = K.kADV_UPWIND if cfg["adv"] == "upwind" else K.kADV_MPDATA
    opt.physics.microphysics = K.kMP_THOMPSON if cfg["mp"] == "thompson" else K.kMP_SB04
    opt.physics.radiation = K.kRA_SIMPLE
    opt.physics.boundarylayer = {"simple": K.kPBL_SIMPLE, "ysu": K.kPBL_YSU}[cfg["pbl"]]
    if cfg["lsm"] == "noah":
        opt.physics.landsurface, opt.physics.watersurface = K.kLSM_NOAH, 0
        opt.lsm_options.max_swe = 25.0
    else:
        opt.physics.landsurface, opt.physics.watersurface = K.kLSM_BASIC, K.kWATER_SIMPLE
    opt.physics.convection = {"none": 0, "bmj": K.kCU_BMJ, "tiedtke": K.kCU_TIEDTKE, "nsas": K.kCU_NSAS}[cfg["cu"]]
    opt.lsm_options.update_interval = ui
    opt.lsm_options.sfc_layer_thickness = SFC_LAYER
    opt.parameters.dz_levels = c["dz_levels"]; opt.parameters.dx = float(c["dx"]); opt.parameters.ideal = True
    mp_var_request(opt); radiation.ra_var_request(opt); pbl.pbl_var_request(opt); surface.lsm_var_request(opt); convection.cu_var_request(opt)
    return opt


def device_tile(cfg, opt, c, dq, g, comm=None, device=0, nc=None, tab=None):
    """a domain_t on the image's grid holding the image's cut, every slot of the configuration initialised in the reference's order"""
    import ra_oracle as R
    from icar_amd import radiation, pbl, surface, convection
    from icar_amd.domain import domain_t
    from icar_amd.microphysics import mp_init
    from icar_amd.advection import adv_init
    from icar_amd.constants import ADVECTION_ORDER
    from icar_amd.capi import lib, check
    from util import KVAR
    d = domain_t(g, device=device, dx=float(c["dx"]), comm=comm)
    d.load_case(c)
    ny, nx = d.ny, d.nx
    for k in R.OUTPUTS[1:]:
        d.set(k, np.full((ny, nx), R.SENTINEL, f32))
    d.exchange_vars = [n for n in ADVECTION_ORDER if opt.vars_to_advect.get(n, 0) > 0]
    assert d.exchange_vars == [KVAR[k] for k in advected(cfg)], (d.exchange_vars, advected(cfg))
    if cfg["lsm"] == "noah":
        import lsm_noah_driver_oracle as LN
        import noah_oracle as N
        d._noah_win = None
        surface.noah_tables(d, tab)
        A = LN.state0(nc)
        for k, m in (("tsk", "skin_temperature"), ("hfx", "sensible_heat"), ("lh", "latent_heat"), ("znt", "roughness_z0")):
            A[k] = c[m].copy()
        A["qsfc"] = c["water_vapor"][:, 0, :].copy()
        for k in ("ivgtyp", "isltyp", "vegfra", "tmn"):
            N.device_set(d, k, nc[k])
        N.device_set(d, "smois", nc["smois0"]); N.device_set(d, "tslb", nc["tslb0"])
        for k in ("albedo", "snow", "snowh", "canwat", "lai", "z0", "qsfc", "qfx"):
            N.device_set(d, k, A[k])
    mp_init(opt, d); adv_init(d, opt); radiation.rad_init(d, opt); pbl.pbl_init(d, opt)
    if cfg["lsm"] == "noah":
        surface.noah_init(d, opt, fndsnowh=False)
    else:
        surface.lsm_init(d, opt)
    convection.init_convection(d, opt)
    if cfg["pbl"] == "ysu":
        pbl.ysu_set(d, "ground_surf_temperature", c["ground_surf_temperature"])
    radiation.rad_calendar(d, *ANCHOR)
    if cfg["lsm"] == "noah":
        d.configure(opt, forced=FORCED, diagnostics=True)
        d.diagnostic_update(3)                                                   # temperature, surface_pressure, the 10 m winds: lsm_init reads them
        surface.noah_couple(d)
    for k, a in dq.items():
        if isinstance(a, np.ndarray):
            d.set_dqdt(k, a)
    if cfg["adv"] == "mpdata-exact":
        check(lib().icar_hip_mpdata_exact(d.ctx, 1), "mpdata_exact")
    return d


def device_fields(cfg, d):
    """what a configuration is compared in: {group: {name: array}}.  "exchanged": the 3-D fields of the exchange list (every cell of the
    memory is compared); the other groups in the owned cells"""
    import ra_oracle as R
    import sfc_oracle as S
    from icar_amd import pbl, convection
    from util import MEMBER
    out = {"exchanged": {n: d.get(MEMBER[n]) for n in advected(cfg)}}
    out["state"] = {n: d.get(n) for n in ("u", "v", "w", "pressure")}
    out["state"].update({n: d.get(MEMBER[n]) for n in SCALARS if n not in advected(cfg)})
    out["surface"] = {k: d.get(k) for k in S.STATE2 + R.OUTPUTS[1:] + ["accumulated_precipitation"]}
    if cfg["lsm"] == "noah":
        import lsm_noah_driver_oracle as LN
        import noah_oracle as N
        out["noah"] = {k: LN.device_get(d, k) for k in N.OUT + LN.DRV}
    if cfg["pbl"] == "ysu":
        out["ysu"] = {k: pbl.ysu_get(d, k) for k in YSU_ARRAYS}
    if cfg["cu"] == "bmj":
        import bmj_oracle as B
        out["cu"] = {k: convection.cu_get(d, k) for k in B.CU_ARRAYS}
    elif cfg["cu"] == "tiedtke":
        import tiedtke_oracle as T
        got = T.device_state(d)
        out["cu"] = {k: got[k] for k in T.TEND + T.OUT2 + ["ktype", "accumulated_convective_pcp"]}
    elif cfg["cu"] == "nsas":
        import nsas_oracle as NS
        got = NS.device_state(d)
        out["cu"] = {k: got[k] for k in NS.TEND + NS.OUT2 + ["accumulated_convective_pcp"]}
    return out


YSU_ARRAYS = ["hpbl", "kpbl", "exch_h", "psim", "psih", "regime", "ri", "windspd", "hol", "tend_u", "tend_v", "tend_th", "tend_qv", "tend_qc", "tend_qi"]


def chain_fields(cfg, ch):
    """the chain's arrays under the names of device_fields"""
    import ra_oracle as R
    import sfc_oracle as S
    out = {"exchanged": {n: ch.s[n] for n in advected(cfg)}}
    out["state"] = {n: ch.s[n] for n in ("u", "v", "w", "pressure")}
    out["state"].update({n: ch.s[n] for n in SCALARS if n not in advected(cfg)})
    out["surface"] = {k: ch.sfc[k] for k in S.STATE2}
    out["surface"].update({k: ch.rad2d[k] for k in R.OUTPUTS[1:]})
    out["surface"]["accumulated_precipitation"] = ch.acc
    if cfg["lsm"] == "noah":
        import lsm_noah_driver_oracle as LN
        import noah_oracle as N
        out["noah"] = {k: ch.noah[k] for k in N.OUT + LN.DRV}
    if cfg["pbl"] == "ysu":
        out["ysu"] = {k: ch.ys[k] for k in YSU_ARRAYS}
    if cfg["cu"] == "bmj":
        import bmj_oracle as B
        out["cu"] = {k: ch.cu[k] for k in B.CU_ARRAYS}
    elif cfg["cu"] == "tiedtke":
        import tiedtke_oracle as T
        out["cu"] = {k: ch.cu[k] for k in T.TEND + T.OUT2 + ["ktype", "accumulated_convective_pcp"]}
    elif cfg["cu"] == "nsas":
        import nsas_oracle as NS
        out["cu"] = {k: ch.cu[k] for k in NS.TEND + NS.OUT2 + ["accumulated_convective_pcp"]}
    return out


def nbits(a, b):
    """the number of values of a that differ from b in a bit (REAL(8) and INTEGER(4) arrays included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize, (a.shape, b.shape, a.dtype, b.dtype)
    v = np.uint64 if a.dtype.itemsize == 8 else np.uint32
    return int((a.view(v) != b.view(v)).sum())


def own(a, sl):
    """the owned cells of a (ny[, nz], nx) array of an image's memory; staggered arrays lose their extra row / column"""
    return a[sl[0]][..., sl[1]]
