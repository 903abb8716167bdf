"""Inputs, shape lists and numpy restatements for the geometry sweep of the streaming, wind-balance and CFL rows
(tests/test_gpu_step_rows_geometry.py on the device, tests/test_step_rows_inputs.py for what the inputs and the oracle alone must
meet).  Needs no GPU.

The restatements below are written from the reference's Fortran statements (src/main/time_step.f90, src/physics/wind.f90,
src/objects/domain_obj.f90), one whole-array numpy float32 expression per statement, NOT from oracle/step_oracle.c: a second,
independent statement of what the kernels of icar_amd/csrc/step.hip, cfl.hip and iterative_winds.hip have to compute.  Arrays are
C-order (ny, nz, nx) == Fortran (i, k, j); u is (ny, nz, nx+1), v is (ny+1, nz, nx)."""
import numpy as np
from icar_amd import ideal

f32 = np.float32
RD = f32(287.058)                # src/constants/icar_constants.f90:391
HILL = 100.0                     # metres.  With the 900 m of test_gpu_step_rows.py the ideal case's Gal-Chen jacobian
                                 # (H_s - terrain) / H_s is negative for nz <= 5 (H_s = 50 + 75 + 125 + 200 + 300 = 750 m)
PLANT = f32(-1.0e5)

# widths that put an edge on each kernel: waves of cells (63, 64, 65), waves of nx + 1 faces (63, 64), waves of nx - 2 interior
# cells (65, 66, 67), blocks of 256 (255, 256, 257), the smallest tile a context takes (3 x 3 x 2)
WIDTHS = [3, 4, 5, 6, 63, 64, 65, 66, 67, 127, 128, 129, 255, 256, 257]
LEVELS = [2, 3, 4, 5, 8, 9]      # at 37 x 4: the four-level tiles of k_diag_face, nz = 2 (level 0 extrapolates from the top level)
BIG = (131, 65, 63)              # 536 445 cells (n3 % 4 = 1), 540 540 u faces: a second trip of every 2048 x 256 grid-stride loop
PLANT_SHAPE = (70, 5, 4)
LATER_CALL_WIDTHS = (3, 64, 257)


def width_shapes():
    """[(nx, ny, nz)] over WIDTHS: ny alternates 3, 4, nz runs through 2, 3, 4, 5 (shifted by one every fourth width, so that the
    pairs (ny, nz) change too); n3 % 4 takes all four values (tests/test_step_rows_inputs.py asserts it)"""
    return [(nx, 3 + n % 2, 2 + (n + n // 4) % 4) for n, nx in enumerate(WIDTHS)]


def level_shapes():
    return [(37, 4, nz) for nz in LEVELS]


def check_case(c):
    """what every case of the sweep must meet: all fields finite, all four jacobians positive"""
    for k, a in c.items():
        if isinstance(a, np.ndarray):
            assert np.isfinite(a).all(), f"{k}: not finite at {c['nx']}x{c['ny']}x{c['nz']}"
    for k in ("jacobian", "jacobian_u", "jacobian_v", "jacobian_w"):
        assert float(c[k].min()) > 0, f"{k}: {float(c[k].min())} at {c['nx']}x{c['ny']}x{c['nz']}"
    return c


def case(nx, ny, nz, seed=3):
    """the case() of tests/test_gpu_step_rows.py over a 100 m hill (HILL above)"""
    c = ideal.make_case(nx, ny, nz, hill_height=HILL, noise=0.02, seed=seed)
    rng = np.random.default_rng(seed)
    c["u"] = (c["u"] + rng.standard_normal(c["u"].shape).astype(np.float32)).astype(np.float32)
    c["v"] = (c["v"] + rng.standard_normal(c["v"].shape).astype(np.float32)).astype(np.float32)
    c["dzdx"] = (0.05 * rng.standard_normal(c["u"].shape)).astype(np.float32)
    c["dzdy"] = (0.05 * rng.standard_normal(c["v"].shape)).astype(np.float32)
    return check_case(c)


def plant_sites(nx, ny, nz):
    """(array, (j, k, i)) of the planted extremes: the first and the last face / cell of each wind array, the u faces on both
    sides of a wave edge, and the w that the top level reads as "the level below\""""
    return [("u", (0, 0, 0)), ("u", (ny - 1, nz - 1, nx)), ("u", (2, 1, 63)), ("u", (2, 1, 64)),
            ("v", (0, 0, 0)), ("v", (ny, nz - 1, nx - 1)),
            ("w", (0, 0, 0)), ("w", (ny - 1, nz - 1, nx - 1)), ("w", (ny - 1, nz - 2, nx - 1))]


def planted_cases(seed=17):
    """(the unplanted 70 x 5 x 4 case, [(label, copy of it with one wind value set to PLANT)])"""
    nx, ny, nz = PLANT_SHAPE
    base = case(nx, ny, nz, seed=seed)
    out = []
    for name, at in plant_sites(nx, ny, nz):
        c = dict(base)
        c[name] = base[name].copy()
        c[name][at] = PLANT
        out.append((f"{name}[{at[0]},{at[1]},{at[2]}]", c))
    return base, out


BIG_PLANT_INDICES = ("last", 131072, 524288)     # n - 1 ; the first element of the second trip of 512 x 256 and of 2048 x 256 threads


def big_planted_cases(base):
    """[(label, copy of the BIG case with PLANT at one linear index of u, v and w)]"""
    out = []
    for at in BIG_PLANT_INDICES:
        c = dict(base)
        for name in ("u", "v", "w"):
            c[name] = base[name].copy()
            c[name].reshape(-1)[c[name].size - 1 if at == "last" else at] = PLANT
        out.append((f"uvw.flat[{at}]", c))
    return out


def rotation(nx, ny, seed=0):
    """sintheta, costheta (REAL(8), (ny, nx)) of a grid rotated by a random angle in every column"""
    theta = np.random.default_rng(seed).uniform(-np.pi, np.pi, (ny, nx))
    return np.sin(theta), np.cos(theta)


# ---- restatements -----------------------------------------------------------------------------------------------------------
def max_courant(u, v, w, dz, dx):
    """time_step.f90:264-289 (cfl_strictness 3, use_density false)"""
    dx = f32(dx)
    dz = np.asarray(dz, f32)[None, :, None]
    below = np.concatenate([w[:, :1, :], w[:, :-1, :]], axis=1)                                 # :266-270 zoffset
    current_wind = (np.maximum(np.abs(u[:, :, :-1]), np.abs(u[:, :, 1:])) / dx                  # :282
                    + np.maximum(np.abs(v[:-1]), np.abs(v[1:])) / dx                            # :283
                    + np.maximum(np.abs(w), np.abs(below)) / dz)                                # :284
    assert current_wind.dtype == np.float32
    return f32(max(f32(0), current_wind.max()))                                                 # :234, :286


def maxabs(x):
    """maxval(abs(x)) of time_step.f90:246-258, :300-301"""
    return f32(np.abs(x).max())


def dt_formula(strict, mu, mv, mw, cell, factor=0.9):
    """time_step.f90:231-318 from the four maxima: (maxwind3d, dt), all REAL(4)"""
    sqrt3 = f32(f32(np.sqrt(f32(3.0))) * f32(1.001))                                            # :231
    m1 = max(max(mu, mv), mw)                                                                   # :246-247
    want = {1: f32(m1 * sqrt3),                                                                 # :250
            2: max(m1, f32(cell * f32(0.577350269))),                                           # :293, :304
            3: cell, 4: f32(cell * sqrt3),                                                      # :310
            5: f32(f32(mu + mv) + mw)}[strict]                                                  # :258
    return want, f32(f32(factor) / want)                                                        # :318


def balance_uvw(u, v, jaco_u, jaco_v, jaco_w, dz, dx):
    """wind.f90:81-169 over calc_divergence(horz_only) :203-210"""
    u_met = u * jaco_u                                                                          # :203
    v_met = v * jaco_v                                                                          # :205
    diff_U = u_met[:, :, 1:] - u_met[:, :, :-1]                                                 # :207
    diff_V = v_met[1:] - v_met[:-1]                                                             # :208
    div = (diff_U + diff_V) / f32(dx)                                                           # :210
    w = np.zeros_like(div)                                                                      # :104
    for k in range(div.shape[1]):
        if k == 0:
            w[:, k] = f32(0) - div[:, k] * dz[:, k] / jaco_w[:, k]                              # :144
        else:
            w[:, k] = (w[:, k - 1] * jaco_w[:, k - 1] - div[:, k] * dz[:, k]) / jaco_w[:, k]    # :146
    assert w.dtype == np.float32
    return w


def interface(x):
    """time_step.f90:88-89 (pressure), :97-98 (temperature)"""
    xi = np.empty_like(x)
    xi[:, 1:] = (x[:, :-1] + x[:, 1:]) / f32(2)
    xi[:, 0] = x[:, 0] + (x[:, 0] - x[:, 1]) / f32(2)
    return xi


def diagnostics(c, exner):
    """time_step.f90:88-108 and :164-194 from the case and the exner field (:85, the one library call of the routine, is taken
    from whoever is compared): temperature, density, the interface values, the mass-point winds and w_real (interior cells; the
    halo ring of the returned w_real is NaN)"""
    p, u, v, w = c["pressure"], c["u"], c["v"], c["w"]
    out = {"pressure_interface": interface(p)}
    out["surface_pressure"] = out["pressure_interface"][:, 0, :].copy()                         # :93
    t = c["potential_temperature"] * exner                                                      # :96
    out["temperature"] = t
    out["temperature_interface"] = interface(t)
    out["density"] = p / (RD * t)                                                               # :101
    out["u_mass"] = (u[:, :, 1:] + u[:, :, :-1]) / f32(2)                                       # :105
    out["v_mass"] = (v[1:] + v[:-1]) / f32(2)                                                   # :108
    ny, nz, nx = w.shape
    wr = np.full((ny, nz, nx), np.nan, np.float32)
    lastw = np.zeros((ny - 2, nx - 2), np.float32)                                              # :164
    for z in range(nz):
        uw = u[1:-1, z, 1:-1] * c["dzdx"][1:-1, z, 1:-1]                                          # :174  (ims+1:ime, jms+1:jme-1)
        vw = v[1:-1, z, 1:-1] * c["dzdy"][1:-1, z, 1:-1]                                          # :176  (ims+1:ime-1, jms+1:jme)
        currw = w[1:-1, z, 1:-1]                                                                # :182
        wr[1:-1, z, 1:-1] = ((uw[:, :-1] + uw[:, 1:]) * f32(0.5) + (vw[:-1] + vw[1:]) * f32(0.5)
                             + c["jacobian"][1:-1, z, 1:-1] * (lastw + currw) * f32(0.5))       # :190-192
        lastw = currw                                                                           # :193
    out["w_real"] = wr
    for k, a in out.items():
        assert a.dtype == np.float32, k
    return out


def forcing_mask(shape, west, east, south, north):
    """domain_obj.f90:2412-2423: the cells a force_boundaries variable is updated in"""
    m = np.zeros(shape, bool)
    if west: m[1:-1, :, 0] = True                                                               # :2413 (ims, :, jms+1:jme-1)
    if east: m[1:-1, :, -1] = True                                                              # :2416
    if south: m[0] = True                                                                       # :2419
    if north: m[-1] = True                                                                      # :2422
    return m


def apply_forcing(x, dqdt, dt, force_boundaries, west=1, east=1, south=1, north=1):
    """domain_obj.f90:2406-2428: REAL + (REAL * REAL(8)) in double, rounded once on assignment; returns the new array"""
    m = forcing_mask(x.shape, west, east, south, north) if force_boundaries else np.ones(x.shape, bool)
    new = (x.astype(np.float64) + (dqdt.astype(np.float64) * np.float64(dt))).astype(np.float32)
    return np.where(m, new, x)


def enforce_limits(x):
    """domain_obj.f90:2230-2241: where (x < 0) x = 0"""
    return np.where(x < 0, f32(0), x)
