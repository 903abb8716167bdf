"""TEST INFRASTRUCTURE: loader of tests/support/noah_oracle.c (the CPU restatement of lsm_noah and LSM_NOAH_INIT as lsm_driver.f90 calls
them: the product's own cell header icar_amd/csrc/noah_column.h compiled for the host) and the recipe of the Noah test cases.  The
library is compiled with gcc -O2 -ffp-contract=off on first use.

A case is a tile of land, water and land-ice cells with the state lsm_init leaves (allocate_noah_data's initial values, the two floors
of lsm_driver.f90:674-675, LSM_NOAH_INIT) and a forcing per carried call: the lowest level's temperature, humidity and pressure, the
two radiation fluxes, the precipitation of the step, the exchange coefficient CHS and the Richardson number.  Between the calls nothing
but the forcing changes: the model's state is what the last call left."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "support", "noah_oracle.c")
HDR = os.path.join(HERE, "..", "icar_amd", "csrc", "noah_column.h")
LIB = os.path.join(HERE, "support", "libnoah_oracle.so")
TABLES = os.path.join(HERE, "golden", "noah_tables.npz")
f32 = np.float32
NSOIL, NLUS, NSLTYPE, NSLOPE = 4, 50, 30, 30
# MODIFIED_IGBP_MODIS_NOAH (options%lsm_options: urban / ice / water / lake_category)
ISURBAN, ISICE, ISWATER, ISLAKE = 13, 15, 17, 21
LAND_VEG = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 18, 19, 20]          # without urban, ice, water and lakes
LAND_SOIL = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 19]     # without 14 (water)
kLC_LAND, kLC_WATER = 1, 2

# noah_column.h's flags
D = {n: 1 << b for b, n in enumerate(
    ["SFLX", "WATER", "LANDICE", "NOPAC", "SNOPAC_MELT", "SNOPAC_NOMELT", "NEW_SNOW", "RAIN_BARE", "RAIN_VEG", "DRIP", "DEW", "CANRES",
     "NO_CANRES", "SMFLX_TWO", "SMFLX_ONE", "SRT_FROZEN", "FRH2O_ITER", "FRH2O_FALLBACK", "SNKSRC_POS", "SNKSRC_NEG", "TDFCND_FROZEN",
     "TDFCND_UNFROZEN", "SNFRAC_BELOW", "SNFRAC_FULL", "SNOWH_REDERIVED", "SNOW_WARM", "SNOW_COLD", "SOIL14", "VEG25_27", "URBAN",
     "SSTEP_MAX", "SSTEP_MIN", "FRZGRA", "FRH2O_BADLOG"])}

# the tables' members in NoahTables' order
T_INT_ARR = ["nrotbl"]
T_VEG = ["snuptbl", "rstbl", "rgltbl", "hstbl", "maxalb", "emissmintbl", "emissmaxtbl", "laimintbl", "laimaxtbl", "z0mintbl", "z0maxtbl",
         "albedomintbl", "albedomaxtbl"]
T_SOIL = ["bb", "drysmc", "f11", "maxsmc", "refsmc", "satpsi", "satdk", "satdw", "wltsmc", "qtz"]
T_GEN = ["topt_data", "cmcmax_data", "cfactr_data", "rsmax_data", "sbeta_data", "fxexp_data", "csoil_data", "salp_data", "refdk_data",
         "refkdt_data", "frzk_data", "zbot_data", "lvcoef_data"]
T_INT = ["bare", "lucats", "slcats", "slpcats"]


class NoahTables(ctypes.Structure):
    _fields_ = ([(n, ctypes.POINTER(ctypes.c_int)) for n in T_INT_ARR] + [(n, ctypes.POINTER(ctypes.c_float)) for n in T_VEG + T_SOIL + ["slope_data"]]
                + [(n, ctypes.c_float) for n in T_GEN] + [(n, ctypes.c_int) for n in T_INT])


_lib = None
_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def bitdiff(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def build(force=False):
    if force or not os.path.exists(LIB) or max(os.path.getmtime(SRC), os.path.getmtime(HDR)) > os.path.getmtime(LIB):
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", LIB, "-lm"])
    return LIB


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
        _lib.noah_oracle_fields.restype = ctypes.c_char_p
        assert _lib.noah_oracle_sizeof_tables() == ctypes.sizeof(NoahTables)
    return _lib


def fields():
    """the order in which noah_oracle_run takes its arrays, read from the header"""
    return lib().noah_oracle_fields().decode().split()


def load_tables(path=TABLES):
    """the tables as the reference parsed them (tests/golden/noah_tables.npz): a dict of arrays with the reference's extents"""
    z = np.load(path)
    return {k: z[k] for k in z.files}


def c_tables(tab):
    """NoahTables over the arrays of tab, which must outlive it"""
    t = NoahTables()
    keep = []
    for n in T_INT_ARR:
        a = np.ascontiguousarray(tab[n], np.int32); keep.append(a)
        setattr(t, n, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    for n in T_VEG + T_SOIL + ["slope_data"]:
        a = np.ascontiguousarray(tab[n], f32); keep.append(a)
        setattr(t, n, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    for n in T_GEN:
        setattr(t, n, float(tab[n]))
    for n in T_INT:
        setattr(t, n, int(tab[n]))
    t._keep = keep
    return t


# ---- the seeded cases of the golden fixtures (tests/golden/make_golden_noah.py) -----------------------------------------------------
# t: the lowest level's mean temperature per call [K]; sw: the downward shortwave's maximum per call [W m-2]; pr: the share of cells with
# precipitation and its maximum [mm per call], per call; dt: lsm_dt
CASES = {
    "noah_a_snowfall_melt_24x12": dict(nx=24, ny=12, seed=1, dt=1800.0, t=[266.0, 268.0, 271.0, 276.0, 280.0, 283.0], sw=[0, 150, 300, 700, 850, 900],
                                       pr=[[0.7, 4.0], [0.6, 3.0], [0.3, 2.0], [0.2, 2.0], [0.0, 0.0], [0.1, 1.0]], snow0=0.3),
    "noah_b_thaw_freeze_26x11": dict(nx=26, ny=11, seed=2, dt=3600.0, t=[278.0, 274.0, 270.0, 264.0, 268.0, 277.0], sw=[500, 200, 0, 0, 100, 600],
                                     pr=[[0.3, 6.0], [0.3, 3.0], [0.4, 2.0], [0.3, 1.0], [0.0, 0.0], [0.2, 5.0]], snow0=0.1, soil_t=274.5),
    "noah_c_summer_rain_24x12": dict(nx=24, ny=12, seed=3, dt=900.0, t=[291.0, 296.0, 300.0, 294.0], sw=[200, 800, 950, 0],
                                     pr=[[0.8, 12.0], [0.3, 2.0], [0.0, 0.0], [0.5, 8.0]], snow0=0.0, soil_t=290.0, wet=True),
    "noah_d_deep_pack_23x13": dict(nx=23, ny=13, seed=4, dt=2400.0, t=[258.0, 262.0, 270.0, 275.0, 279.0], sw=[0, 250, 500, 800, 900],
                                   pr=[[0.5, 6.0], [0.4, 4.0], [0.2, 1.0], [0.0, 0.0], [0.1, 2.0]], snow0=0.8, snow_max=250.0, soil_t=268.0,
                                   fndsnowh=True),
    "noah_e_night_dew_25x12": dict(nx=25, ny=12, seed=5, dt=1200.0, t=[281.0, 277.0, 274.5, 272.5, 276.0], sw=[0, 0, 0, 0, 300],
                                   pr=[[0.0, 0.0], [0.2, 1.0], [0.3, 1.5], [0.3, 1.0], [0.0, 0.0]], snow0=0.15, soil_t=276.0, humid=True),
    "noah_f_urban_bare_24x12": dict(nx=24, ny=12, seed=6, dt=600.0, t=[272.0, 273.5, 275.0, 271.0, 269.0, 274.0], sw=[100, 400, 600, 50, 0, 500],
                                    pr=[[0.5, 2.0], [0.5, 2.0], [0.4, 3.0], [0.4, 1.0], [0.3, 1.0], [0.2, 1.0]], snow0=0.4, soil_t=272.5,
                                    urban=0.25, bare=0.2),
}
SEEDS = {"seed_g": dict(nx=22, ny=10, seed=7, dt=1500.0, t=[269.0, 273.0, 277.0, 271.0], sw=[0, 400, 700, 100],
                        pr=[[0.5, 3.0], [0.4, 2.0], [0.2, 2.0], [0.5, 3.0]], snow0=0.3, soil_t=273.0),
         "seed_h": dict(nx=18, ny=9, seed=8, dt=3000.0, t=[285.0, 279.0, 272.0, 266.0, 274.0], sw=[600, 300, 0, 0, 500],
                        pr=[[0.3, 5.0], [0.3, 3.0], [0.4, 3.0], [0.3, 1.0], [0.1, 1.0]], snow0=0.0, soil_t=280.0, fndsnowh=True)}

IO3 = ["smois", "tslb", "sh2o", "smcrel"]
# what lsm_noah writes; on a land-ice cell the reference stores locals that SFLX alone sets in the arrays of ICE_UNSET (noah_column.h)
OUT2 = ["tsk", "hfx", "qfx", "lh", "grdflx", "smstav", "smstot", "sfcrunoff", "udrunoff", "albedo", "albbck", "znt", "z0", "emiss", "snowc",
        "qsfc", "snow", "snowh", "canwat", "chs2", "chklowq", "lai", "snotime", "acsnom", "acsnow", "snopcx", "potevp", "noahres", "flx4",
        "fvb", "fbur", "fgsn"]
OUT = OUT2 + IO3
ICE_UNSET = ["albedo", "znt", "hfx", "qfx", "lh", "grdflx", "qsfc", "potevp", "noahres", "smstav", "sfcrunoff", "acsnom", "snopcx", "flx4",
             "fvb", "fbur", "fgsn"]


def ncalls(p):
    return len(p["t"])


def qsat(t, p):
    es = 611.2 * np.exp(17.67 * (t - 273.15) / (t - 29.65))
    return 0.622 * es / (p - es)


def make_case(tab, nx, ny, seed, dt, t, sw, pr, snow0, snow_max=60.0, soil_t=None, wet=False, humid=False, urban=0.04, bare=0.06,
              fndsnowh=False):
    """the static fields, the state before lsm_init's LSM_NOAH_INIT, and the forcing of every call"""
    rng = np.random.default_rng(21000 + seed)
    s2, s3 = (ny, nx), (ny, NSOIL, nx)
    u = rng.random(s2)
    xland = np.where(u < 0.12, kLC_WATER, kLC_LAND)
    xland[0, :2] = kLC_WATER                                                  # every tile has water ...
    veg = rng.choice(LAND_VEG, s2)
    veg = np.where(rng.random(s2) < urban, ISURBAN, veg)
    veg = np.where(rng.random(s2) < bare, 16, veg)
    veg = np.where(rng.random(s2) < 0.05, ISICE, veg)
    veg[-1, -1] = ISICE                                                       # ... and land ice
    xland[-1, -1] = kLC_LAND
    veg = np.where(xland == kLC_WATER, ISWATER, veg)
    soil = rng.choice(LAND_SOIL, s2)
    soil = np.where(rng.random(s2) < 0.06, 14, soil)                          # soil "water" under land: reset to 7 by :768-774
    soil = np.where(veg == ISICE, 16, soil)
    soil = np.where(xland == kLC_WATER, 14, soil)
    vegfra = np.where(rng.random(s2) < 0.15, 0.0, rng.uniform(1.0, 99.0, s2))
    vegfra = np.where(rng.random(s2) < 0.05, 100.0, vegfra)
    maxsmc = np.asarray(tab["maxsmc"], np.float64)[soil - 1]
    wlt = np.asarray(tab["wltsmc"], np.float64)[soil - 1]
    lo, hi = (0.75, 0.995) if wet else (0.15, 0.97)
    smois = wlt[:, None, :] + (maxsmc - wlt)[:, None, :] * rng.uniform(lo, hi, s3)
    smois = np.where((xland == kLC_WATER)[:, None, :], 1.0, smois)
    t0 = float(t[0])
    tmn = (t0 if soil_t is None else soil_t) + 4.0 + rng.normal(0, 1.5, s2)
    top = (t0 if soil_t is None else soil_t) + rng.normal(0, 1.5, s2)
    w = np.array([0.05, 0.25, 0.7, 1.5])[None, :, None] / 3.0
    tslb = top[:, None, :] * (1 - w) + tmn[:, None, :] * w + rng.normal(0, 0.3, s3)
    tsk = top + rng.normal(0, 1.0, s2)
    snow = np.where(rng.random(s2) < snow0, rng.uniform(0.05, snow_max, s2), 0.0)
    snow = np.where(xland == kLC_WATER, 0.0, snow)
    snowh = np.where(rng.random(s2) < 0.5, 0.0, snow * 0.004)                  # an input snow height, missing (0) in half the cells
    lai = rng.uniform(0.5, 4.0, s2)
    canwat = np.where(rng.random(s2) < 0.4, rng.uniform(0.0, 4.0e-4, s2), 0.0)
    z0 = rng.uniform(0.01, 0.5, s2)
    albedo = rng.uniform(0.1, 0.3, s2)
    c = dict(nx=nx, ny=ny, dt=f32(dt), fndsnowh=bool(fndsnowh), xland=xland.astype(f32), ivgtyp=veg.astype(np.int32), isltyp=soil.astype(np.int32),
             vegfra=vegfra.astype(f32), tmn=tmn.astype(f32), shdmin=np.zeros(s2, f32), shdmax=np.full(s2, 100, f32), cqs2=np.full(s2, 0.01, f32),
             smois0=smois.astype(f32), tslb0=tslb.astype(f32), tsk0=tsk.astype(f32), snow0=snow.astype(f32), snowh0=snowh.astype(f32),
             lai0=lai.astype(f32), canwat0=canwat.astype(f32), z00=z0.astype(f32), albedo0=albedo.astype(f32), forcing=[])
    psfc = 101000.0 - 30000.0 * rng.random(s2) * (np.arange(nx)[None, :] / max(nx - 1, 1))
    for n in range(len(t)):
        ta = t[n] + rng.normal(0, 1.8, s2)
        p1 = psfc + rng.normal(0, 60, s2)
        p2 = p1 - rng.uniform(250.0, 700.0, s2)
        rh = rng.uniform(0.85, 1.02, s2) if humid else rng.uniform(0.25, 1.0, s2)
        qv = rh * qsat(ta, 0.5 * (p1 + p2))
        qgh = qsat(ta + rng.normal(0.3, 0.5, s2), p1)
        swd = sw[n] * rng.uniform(0.3, 1.0, s2)
        glw = 0.75 * 5.67e-8 * ta ** 4 * rng.uniform(0.9, 1.2, s2)
        share, amount = pr[n]
        rain = np.where(rng.random(s2) < share, rng.uniform(0.0, 1.0, s2) ** 2 * amount, 0.0)
        chs = rng.uniform(5.0e-4, 3.0e-2, s2)
        rib = rng.uniform(-0.6, 0.6, s2)
        c["forcing"].append({k: v.astype(f32) for k, v in dict(qv=qv, p8w1=p1, p8w2=p2, t=ta, qgh=qgh, swdown=swd, glw=glw, rainbl=rain,
                                                             chs=chs, rib=rib).items()})
    return c


def tile_of(c):
    return 1, c["nx"], 1, c["ny"]


def state0(c):
    """allocate_noah_data's initial values (lsm_driver.f90:425-520), domain%albedo in ALBEDO, the two floors of :674-675"""
    ny, nx = c["ny"], c["nx"]
    s2, s3 = (ny, nx), (ny, NSOIL, nx)
    A = {k: np.zeros(s2, f32) for k in OUT2}
    A.update(smstav=np.full(s2, 0.5, f32), albedo=c["albedo0"].copy(), albbck=np.full(s2, 0.17, f32), emiss=np.full(s2, 0.99, f32),
             snoalb=np.full(s2, 0.8, f32), tsk=c["tsk0"].copy(), snow=c["snow0"].copy(), snowh=c["snowh0"].copy(), lai=c["lai0"].copy(),
             canwat=c["canwat0"].copy(), z0=c["z00"].copy(), znt=c["z00"].copy(), chs2=np.zeros(s2, f32))
    A["tslb"] = np.where(c["tslb0"] < 200, f32(200), c["tslb0"]).astype(f32)
    A["smois"] = np.where(c["smois0"] < f32(0.0001), f32(0.0001), c["smois0"]).astype(f32)
    A["sh2o"] = np.full(s3, 0.25, f32)
    A["smcrel"] = np.zeros(s3, f32)
    A["diag"] = np.zeros(s2, np.uint64)
    return A


def lsm_init(tab, c, A, tile=None):
    """LSM_NOAH_INIT's per-cell part as lsm_init calls it (:672-707): canopy_water is restored afterwards"""
    its, ite, jts, jte = tile or tile_of(c)
    ci = ctypes.c_int
    keep = A["canwat"].copy()
    T = c_tables(tab)
    bad = lib().noah_oracle_init(ci(c["nx"]), ci(c["ny"]), ci(its), ci(ite), ci(jts), ci(jte), ci(int(c["fndsnowh"])), ctypes.byref(T), _p(c["ivgtyp"]),
                                 _p(c["isltyp"]), _p(A["tslb"]), _p(A["smois"]), _p(A["sh2o"]), _p(A["snoalb"]), _p(A["snow"]), _p(A["snowh"]),
                                 _p(A["canwat"]), _p(A["diag"]))
    assert bad == 0
    A["canwat"][...] = keep
    c["xland"][(c["ivgtyp"] == ISWATER) | (c["ivgtyp"] == ISLAKE)] = kLC_WATER           # lsm_driver.f90:710


def lsm_noah(tab, c, A, n, tile=None, dt=None):
    """lsm_noah with the forcing of call n (0-based) on the tile; A is read and written"""
    its, ite, jts, jte = tile or tile_of(c)
    F = c["forcing"][n]
    ptr = []
    for k in fields():
        a = F[k] if k in F else c[k] if k in c else A[k]
        assert a.flags.c_contiguous and a.dtype in (f32, np.int32), k
        ptr.append(a.ctypes.data)
    arr = (ctypes.c_void_p * len(ptr))(*ptr)
    ci = ctypes.c_int
    T = c_tables(tab)
    lib().noah_oracle_run(ci(c["nx"]), ci(c["ny"]), ci(its), ci(ite), ci(jts), ci(jte), ctypes.c_float(float(c["dt"] if dt is None else dt)),
                          ci(ISURBAN), ci(ISICE), ctypes.byref(T), arr, _p(A["diag"]))


def ice_cells(c):
    return (c["xland"] < 1.5) & (c["ivgtyp"] == ISICE)


def fingerprint(c):
    s = sum(float(np.asarray(c[k], np.float64).sum()) for k in c if isinstance(c[k], np.ndarray))
    return s + sum(float(np.asarray(v, np.float64).sum()) for F in c["forcing"] for v in F.values())


# ---- the same on the device -------------------------------------------------------------------------------------------------------
# lsm_noah's arguments that are fields of the context, and those that are ICAR_NOAH_* arrays (icar_amd.surface.NOAH_ARRAYS)
FIELD_OF = {"tsk": "skin_temperature", "hfx": "sensible_heat", "lh": "latent_heat", "qfx": "qfx", "qsfc": "qsfc", "znt": "roughness_z0",
            "swdown": "shortwave", "glw": "longwave"}
NOAH_OF = {"qgh": "qgh", "tmn": "soil_deep_temperature", "vegfra": "vegfrac", "shdmin": "shdmin", "shdmax": "shdmax", "snoalb": "snoalb",
           "rainbl": "current_precipitation", "cqs2": "cqs2", "chs": "chs", "rib": "ri", "grdflx": "ground_heat_flux", "smstav": "smstav",
           "smstot": "soil_totalmoisture", "sfcrunoff": "sfcrunoff", "udrunoff": "udrunoff", "albedo": "albedo", "albbck": "albbck", "z0": "z0",
           "emiss": "emiss", "snowc": "snowc", "snow": "snow_water_equivalent", "snowh": "snow_height", "canwat": "canopy_water", "chs2": "chs2",
           "chklowq": "chklowq", "lai": "lai", "snotime": "snotime", "acsnom": "acsnom", "acsnow": "acsnow", "snopcx": "snopcx", "potevp": "potevp",
           "noahres": "noahres", "flx4": "flx4", "fvb": "fvb", "fbur": "fbur", "fgsn": "fgsn", "smois": "soil_water_content",
           "tslb": "soil_temperature", "sh2o": "sh2o", "smcrel": "smcrel", "ivgtyp": "veg_type", "isltyp": "soil_type"}


def options_of(c):
    from icar_amd.options import options_t
    opt = options_t()
    opt.physics.landsurface = 3
    opt.physics.advection = opt.physics.microphysics = 0
    return opt


def device_set(d, k, a, win=None):
    """one of lsm_noah's arguments, by its name there; win = (rows, columns) slices of the case's arrays that the domain's memory holds"""
    from icar_amd import surface
    a = np.asarray(a)
    if win is not None:
        a = a[win[0]][..., win[1]]
    if k == "xland":
        d.set("land_mask", a.astype(np.int32))
    elif k in FIELD_OF:
        d.set(FIELD_OF[k], a)
    else:
        surface.noah_set(d, NOAH_OF[k], a)


def device_get(d, k):
    from icar_amd import surface
    return d.get(FIELD_OF[k]) if k in FIELD_OF else surface.noah_get(d, NOAH_OF[k])


def device_forcing(d, c, n, win=None):
    """the forcing of call n: the atmosphere's lowest levels, the radiation and what lsm() would compute in front of the call"""
    F = c["forcing"][n]
    cut = (lambda a: a) if win is None else (lambda a: a[win[0]][..., win[1]])
    two = lambda a, b: np.ascontiguousarray(np.stack([cut(a), cut(b)], axis=1))
    d.set("water_vapor", two(F["qv"], F["qv"]))
    d.set("temperature", two(F["t"], F["t"]))
    d.set("pressure_interface", two(F["p8w1"], F["p8w2"]))
    for k in ("swdown", "glw", "qgh", "rainbl", "chs", "rib"):
        device_set(d, k, F[k], win)


def device_domain(tab, c, grid=None, init=True, land_mask=True):
    """a domain_t holding the case before lsm_init (state0, but the soil arrays as the case has them: the two floors are lsm_init's), the
    tables on the device, and -- init -- icar_hip_lsm_init run; land_mask=False: domain%land_mask is never uploaded"""
    from icar_amd import surface
    from icar_amd.domain import domain_t
    from icar_amd.grid import grid_t
    win = None
    if grid is None:
        grid = grid_t().set_grid_dimensions(c["nx"], c["ny"], 2, 1, 1)
    else:
        win = (slice(grid.jms - 1, grid.jme), slice(grid.ims - 1, grid.ime))
    d = domain_t(grid, device=0, dx=1000.0)
    d._noah_win = win
    surface.noah_tables(d, tab)
    A = state0(c)
    if land_mask:
        device_set(d, "xland", c["xland"], win)
    for k in ("ivgtyp", "isltyp", "vegfra", "tmn"):
        device_set(d, k, c[k], win)
    device_set(d, "smois", c["smois0"], win)
    device_set(d, "tslb", c["tslb0"], win)
    for k in ("albedo", "snow", "snowh", "canwat", "lai", "tsk", "z0", "znt"):
        device_set(d, k, A[k], win)
    for k in ("hfx", "lh", "qfx", "qsfc"):
        device_set(d, k, A[k], win)
    if init:
        surface.noah_init(d, options_of(c), fndsnowh=c["fndsnowh"])
    return d


def device_put(d, A, keys=OUT + ["snoalb"]):
    for k in keys:
        device_set(d, k, A[k], d._noah_win)


def device_state(d, keys=OUT):
    return {k: device_get(d, k) for k in keys}
