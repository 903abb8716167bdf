"""Inputs, launch layouts and shape lists of the horizontal sweeps of the advection (tests/test_gpu_mpdata_rows.py on the device,
tests/test_mpdata_rows_inputs.py for what the lists, the inputs and the oracle alone must meet).  Needs no GPU.

The fused MPDATA kernel (icar_amd/csrc/mpdata.hip) lays a launch out by nx (x tiles of 58 outputs), ny and the scalar count (y chunks,
the last of them shorter), nz (level ranges, levels per thread) and deals the work items (tile, chunk, range, scalar) to the XCDs;
each chunk marches through warm-up, steady pairs and a tail whose lengths depend on where the chunk lies.  geometry() asks the
product's own header (mpdata_geometry.h) through the probe library; the row counts of the lists are found by scanning it, so that a
layout formula that moves takes the lists with it -- or fails test_mpdata_rows_inputs.py where a class is no longer reached."""
import ctypes
import numpy as np
from icar_amd import ideal
from icar_amd._fields import N_ADVECTABLE
from util import roughen_winds

# the advectable scalars in the dispatch order (constants.ADVECTION_ORDER), by their case names
FIELDS = ["water_vapor", "cloud_water", "rain", "snow", "potential_temperature", "cloud_ice", "graupel", "ice_number", "rain_number",
          "snow_number", "graupel_number"]
assert len(FIELDS) == N_ADVECTABLE
NAMES = ["water_vapor", "cloud_water", "potential_temperature"]      # the three scalars of the width, row and range sweeps
NY_MAX = 300
XOUT = 58                      # outputs of an x tile (MP_XOUT; test_mpdata_rows_inputs.py holds it to the probe)


# ---- the layout ----------------------------------------------------------------------------------------------------------------
def geometry(probe, nx, ny, nz, nv=len(NAMES)):
    """the launch of one corrective iteration: ntile, nkr, kstore, kb, nw, nchunk, clen, exact, nitem and per chunk
    {ja, jb, rows, P0, s0, s1, npair, ntail, north} (north: the chunk's last row is the last row inside the ring)"""
    out = (ctypes.c_int * (8 + 7 * max(1, (ny - 2) // 16 + 1)))()
    rc = probe.icar_probe_mpdata_geometry(int(nx), int(nz), int(ny), int(nv), out)
    assert rc == 0, f"icar_probe_mpdata_geometry({nx}, {nz}, {ny}, {nv}) = {rc}"
    g = dict(zip(("ntile", "nkr", "kstore", "kb", "nw", "nchunk", "clen", "exact"), out[:8]))
    g["exact"] = bool(g["exact"])
    g["nitem"] = g["ntile"] * g["nchunk"] * g["nkr"] * nv
    g["chunks"] = []
    for ch in range(g["nchunk"]):
        c = dict(zip(("ja", "jb", "P0", "s0", "s1", "npair", "ntail"), out[8 + 7 * ch:15 + 7 * ch]))
        c["rows"] = c["jb"] - c["ja"] + 1
        c["north"] = c["jb"] == ny - 2
        g["chunks"].append(c)
    g["last_rows"] = g["chunks"][-1]["rows"]
    return g


def march_class(chunk):
    """(steady pairs: 0, 1 or 2 for two and more; generic tail steps)"""
    return (min(chunk["npair"], 2), chunk["ntail"])


def shape_nv(shape):
    return len(shape[3])


def smallest_ny(probe, nx, nz, want, nv=len(NAMES)):
    """the smallest ny <= NY_MAX whose layout meets want(geometry)"""
    for ny in range(3, NY_MAX + 1):
        if want(geometry(probe, nx, ny, nz, nv)):
            return ny
    raise AssertionError(f"no ny <= {NY_MAX} at nx = {nx}, nz = {nz}, nv = {nv} has the wanted layout")


# ---- the shape lists: (nx, ny, nz, names) -----------------------------------------------------------------------------------------
def widths():
    """every tile width 3 .. 130 and 174 .. 178 (the third tile's seam) at 6 rows and 9 levels (2 levels per thread, 5 waves, the
    kernel's general template); at 8 levels (1 per thread, 8 waves, the template whose waves hold exactly the column) the widths
    around nx = 3, one full tile and two full tiles -- and the seams 63 / 64 / 126 / 127 of the exact mode's tiles"""
    w9 = list(range(3, 131)) + list(range(174, 179))
    w8 = list(range(3, 9)) + list(range(58, 67)) + list(range(116, 129))
    return [(nx, 6, 9, NAMES) for nx in w9] + [(nx, 6, 8, NAMES) for nx in w8]


ROW_WIDTHS = (5, 61)           # one x tile; two, the second owning one column


def row_counts(probe, nx, nz=9):
    """every ny 3 .. 70, the smallest ny whose last chunk has 1 .. 6 rows, the smallest ny of 2, of 3 and of 8 or more chunks"""
    nys = set(range(3, 71))
    for r in range(1, 7):
        nys.add(smallest_ny(probe, nx, nz, lambda g: g["nchunk"] > 1 and g["last_rows"] == r))
    nys.add(smallest_ny(probe, nx, nz, lambda g: g["nchunk"] == 2))
    nys.add(smallest_ny(probe, nx, nz, lambda g: g["nchunk"] == 3))
    nys.add(smallest_ny(probe, nx, nz, lambda g: g["nchunk"] >= 8))
    return sorted(nys)


def chunk_class(chunk):
    """a chunk's march class and whether it touches the north ring"""
    return march_class(chunk) + (chunk["north"],)


def march_classes(probe):
    """{(pairs, tail, north): the first shape that has such a chunk} over every ny <= NY_MAX, the sweeps' widths and level counts and
    1 .. 11 scalars, the row sweep's own (9 levels, three scalars) first: every march the layout formula can produce up to NY_MAX rows"""
    first = {}
    for nz in (9, 8, 41, 80):
        for nx in ROW_WIDTHS:
            for nv in [len(NAMES)] + [n for n in range(1, N_ADVECTABLE + 1) if n != len(NAMES)]:
                for ny in range(3, NY_MAX + 1):
                    for ch in geometry(probe, nx, ny, nz, nv)["chunks"]:
                        first.setdefault(chunk_class(ch), (nx, ny, nz, NAMES if nv == len(NAMES) else FIELDS[:nv]))
    return first


def classes_of(probe, shapes):
    return {chunk_class(ch) for s in shapes for ch in geometry(probe, s[0], s[1], s[2], shape_nv(s))["chunks"]}


def rows(probe):
    """row_counts() at both widths; then, for every march class that none of those shapes has (a class that three scalars on 9 levels
    do not reach up to NY_MAX rows), the first shape of march_classes() that has it"""
    out = [(nx, ny, 9, NAMES) for nx in ROW_WIDTHS for ny in row_counts(probe, nx)]
    have = classes_of(probe, out)
    return out + [s for k, s in sorted(march_classes(probe).items()) if k not in have]


def scalars():
    """1 .. 11 scalars on a single-item shape (5 x 10: nitem = nv) and on two tiles x several chunks (61 x 40)"""
    return [(nx, ny, 9, FIELDS[:nv]) for (nx, ny) in ((5, 10), (61, 40)) for nv in range(1, N_ADVECTABLE + 1)]


RANGE_NAMES = {3: NAMES, 2: [NAMES[0], NAMES[2]], 1: [NAMES[2]]}


def ranges(probe):
    """2 and 3 level ranges (41 and 80 levels) x 40 rows and the row counts whose last chunk has 1 and 2 rows, on two x tiles.  The
    chunk count is chosen by the number of work items, ranges and scalars included: with three scalars and three ranges no row
    count up to 800 leaves a last chunk of 1 or 2 rows, so a shape takes the most scalars (3, 2, 1) with which one up to NY_MAX does."""
    out = []
    for nz in (41, 80):
        out.append((61, 40, nz, NAMES))
        for r in (1, 2):
            for nv in (3, 2, 1):
                try:
                    ny = smallest_ny(probe, 61, nz, lambda g: g["nchunk"] > 1 and g["last_rows"] == r, nv)
                except AssertionError:
                    continue
                out.append((61, ny, nz, RANGE_NAMES[nv]))
                break
            else:
                raise AssertionError(f"no ny <= {NY_MAX} at nx = 61, nz = {nz} has a last chunk of {r} rows with 1 .. 3 scalars")
    return out


_LISTS = {}


def lists(probe):
    if not _LISTS:
        _LISTS.update({"widths": widths(), "rows": rows(probe), "scalars": scalars(), "ranges": ranges(probe)})
    return _LISTS


def group(shapes, g, ngroups):
    """the g-th of ngroups contiguous parts of a list, each shape with its index in the whole list"""
    n = len(shapes)
    return [(t, shapes[t]) for t in range(g * n // ngroups, (g + 1) * n // ngroups)]


def with_variants(shapes):
    """indices of the shapes that also run the other forms of the scheme: every fourth, the first and the last"""
    return sorted(set(range(0, len(shapes), 4)) | {0, len(shapes) - 1})


# ---- the inputs ----------------------------------------------------------------------------------------------------------------
def column_case(oracle, nz, nx=70, ny=10):
    """A 70 x 10 tile (two x tiles of the fused kernel, one of them partial; steady and generic steps of the y march) of nz levels.
    The level thicknesses differ from level to level (100 .. 300 m: a level read from the wrong slot shows), the top stays below
    25 km (the ideal case's own profile reaches the top of its pressure formula near 90 levels), and u, v carry white noise
    (w rebalanced), so that the limiter works on nearly every face."""
    f32 = np.float32
    c = ideal.make_case(nx, ny, nz, hill_height=1000.0, noise=0.01, n_hydro=1, uniform_dz=200.0)
    dzl = (f32(100.0) + f32(50.0) * ((np.arange(nz) * 3) % 5).astype(f32)).astype(f32)
    c["dz_levels"] = dzl
    c["advection_dz"] = np.ascontiguousarray(np.broadcast_to(dzl[None, :, None], (ny, nz, nx))).astype(f32)
    c["dz_mass"] = (c["advection_dz"] * c["jacobian"]).astype(f32)
    return roughen_winds(c, oracle, 0.5)


# per scalar: (magnitude, offset, amplitude) of  magnitude x (offset + amplitude x pattern), pattern in 0 .. 1
CONTENT = {"water_vapor": (1e-2, 0.3, 1.0), "cloud_water": (1e-4, 0.2, 1.0), "rain": (3e-4, 0.1, 1.0), "snow": (2e-4, 0.4, 1.0),
           "potential_temperature": (1.0, 290.0, 30.0), "cloud_ice": (2e-5, 0.25, 1.0), "graupel": (5e-4, 0.15, 1.0),
           "ice_number": (1e4, 0.5, 1.0), "rain_number": (1e3, 0.35, 1.0), "snow_number": (3e3, 0.45, 1.0), "graupel_number": (7e2, 0.05, 1.0)}
SEED = 2100


def zero_block(m, nx, ny, nz):
    """the block of exact zeros of scalar m: a third of each extent (at least one cell), placed by m"""
    wx, wy, wz = max(1, nx // 3), max(1, ny // 3), max(1, nz // 3)
    i0, j0, k0 = (1 + 2 * m) % (nx - wx + 1), (1 + 3 * m) % (ny - wy + 1), m % (nz - wz + 1)
    return (slice(j0, j0 + wy), slice(k0, k0 + wz), slice(i0, i0 + wx))


def edge_mask(m, nx, ny, nz):
    """the cells beyond scalar m's sharp edge (an oblique plane through the tile, its direction and place by m): 2.5 x the field"""
    jj, kk, ii = np.meshgrid(np.arange(ny), np.arange(nz), np.arange(nx), indexing="ij")
    s = (1 + m % 3) * ii * (ny + 1) + (1 + m % 2) * jj * (nx + 1) + kk * (1 if m % 4 else -1)
    return s > np.quantile(s, 0.35 + 0.03 * m)


def rows_case(oracle, nx, ny, nz, names=FIELDS, seed=SEED):
    """column_case's tile (a hill, level thicknesses that differ from level to level, white noise on u and v with w rebalanced) of any
    shape from 3 x 3 up, and all eleven advectable scalars with content of their own: a magnitude, an offset and a pattern per scalar
    (a wave whose direction differs from scalar to scalar + white noise), one sharp oblique edge (2.5 x) and one block of exact zeros,
    each placed by the scalar's index -- a swapped scalar, tile, chunk or level range is wrong in every cell.  (The ideal case's
    hydrometeors follow a blob in the tile's middle and vanish on thin tiles.)  names: the scalars to fill, each as it is in the full set."""
    c = column_case(oracle, nz, nx, ny)
    jj, kk, ii = np.meshgrid(np.arange(ny, dtype=np.float64), np.arange(nz, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    for m, n in enumerate(FIELDS):
        if n not in names:
            continue
        mag, off, amp = CONTENT[n]
        rng = np.random.default_rng(seed + m)
        wave = 0.5 + 0.5 * np.sin(0.37 * (1 + m % 4) * ii + 0.53 * (1 + m % 3) * jj + 0.71 * (1 + m % 2) * kk + 0.9 * m)
        pat = 0.7 * wave + 0.3 * rng.uniform(0.0, 1.0, (ny, nz, nx))
        q = mag * (off + amp * pat)
        q = np.where(edge_mask(m, nx, ny, nz), 2.5 * q, q)
        q[zero_block(m, nx, ny, nz)] = 0.0
        c[n] = np.ascontiguousarray(q, np.float32)
    return c


def check_case(c, names=FIELDS):
    """what every case must meet: finite, positive jacobians and density, every scalar non-zero in at least half of its cells, with
    its block of exact zeros and a sharp edge (neighbouring non-zero cells along x, y or z that differ by a factor of 1.5 and more)"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    for k, a in c.items():
        if isinstance(a, np.ndarray):
            assert np.isfinite(a).all(), f"{k}: not finite"
    for k in ("jacobian", "jacobian_u", "jacobian_v", "jacobian_w", "density", "advection_dz"):
        assert (c[k] > 0).all(), f"{k}: not positive"
    for m, n in enumerate(FIELDS):
        if n not in names:
            continue
        q = c[n]
        assert q.shape == (ny, nz, nx) and q.dtype == np.float32
        assert (q >= 0).all() and (q != 0).mean() >= 0.5, f"{n}: non-zero in {float((q != 0).mean()):.2f} of the cells"
        assert not q[zero_block(m, nx, ny, nz)].any() and q[zero_block(m, nx, ny, nz)].size > 0, f"{n}: no block of exact zeros"
        sharp = False
        for ax in range(3):
            a, b = np.moveaxis(q, ax, 0)[:-1].astype(np.float64), np.moveaxis(q, ax, 0)[1:].astype(np.float64)
            both = (a > 0) & (b > 0)
            sharp |= bool((np.maximum(a, b)[both] > 1.5 * np.minimum(a, b)[both]).any())
        assert sharp, f"{n}: no sharp edge"
    for a in range(len(names)):
        for b in range(a + 1, len(names)):
            assert not np.array_equal(c[names[a]], c[names[b]])


def ring(q):
    """the boundary ring of a (ny, nz, nx) field: rows 0 and ny-1, columns 0 and nx-1, every level"""
    return np.concatenate([q[0].ravel(), q[-1].ravel(), q[:, :, 0].ravel(), q[:, :, -1].ravel()])


def nudged(c, names):
    """the case with every cell of every input of the advection moved up by one float ulp.  The scalars' exact zeros stay zeros: an
    empty cell carries no rounding error, and util.local_rel_err wants an empty neighbourhood reproduced exactly."""
    d = dict(c)
    for k in list(names) + ["u", "v", "w", "density", "jacobian", "jacobian_u", "jacobian_v", "jacobian_w", "advection_dz", "dz_levels"]:
        up = np.nextafter(c[k], np.float32(np.inf)).astype(np.float32)
        d[k] = np.where(c[k] == 0, c[k], up) if k in names else up
    return d
