"""convection driver mirror (src/physics/cu_driver.f90): cu_var_request / init_convection / convect, plus the scheme on its own.

convection = kCU_BMJ (Betts-Miller-Janjic, src/physics/cu_bmj.f90), kCU_TIEDTKE (src/physics/cu_tiedtke.f90, through cu_init,
which takes domain%znu) and kCU_NSAS (src/physics/cu_nsas.f90, through convection_init, which takes domain%dx) are built; kCU_SIMPLE
and kCU_KAINFR are refused because the reference has no branch for them.  The slot's own arrays (CLDEFI, RAINCV, CUTOP, CUBOT, accumulated_convective_pcp, tend%th, tend%qv) have no field
id: cu_get / cu_set move them by the ICAR_CU_* names below, tiedtke_get / tiedtke_set the Tiedtke scheme's (tend%qc, tend%qi,
PRATEC, KTYPE) by the ICAR_TIEDTKE_* names, nsas_get / nsas_set the NSAS scheme's (tend%qc, tend%qi, PRATEC, HBOT, HTOP, hpbl) by
the ICAR_NSAS_* names."""
import ctypes
import numpy as np
from .capi import lib, check
from .constants import kCU_BMJ, kCU_NSAS, kCU_TIEDTKE, kNO_STOCHASTIC


# enum icar_hip_cu_array (include/icar_hip.h)
CU_CLDEFI, CU_ACC_CONV_PCP, CU_RAINCV, CU_CUTOP, CU_CUBOT, CU_TEND_TH, CU_TEND_QV, CU_N = range(8)
CU_NAMES = {"cldefi": CU_CLDEFI, "accumulated_convective_pcp": CU_ACC_CONV_PCP, "raincv": CU_RAINCV, "cutop": CU_CUTOP, "cubot": CU_CUBOT,
            "tend_th": CU_TEND_TH, "tend_qv": CU_TEND_QV}
# BMJINIT's tables in the order of icar_hip_cu_tables, with their Fortran shapes
CU_TABLES = (("QS0", (134,)), ("SQS", (134,)), ("PTBL", (76, 134)), ("THE0", (76,)), ("STHE", (76,)), ("TTBL", (134, 76)),
             ("THE0Q", (152,)), ("STHEQ", (152,)), ("TTBLQ", (440, 152)))


# enum icar_hip_tiedtke_array (include/icar_hip.h)
TIEDTKE_TEND_QC, TIEDTKE_TEND_QI, TIEDTKE_PRATEC, TIEDTKE_KTYPE, TIEDTKE_N = range(5)
TIEDTKE_NAMES = {"tend_qc": TIEDTKE_TEND_QC, "tend_qi": TIEDTKE_TEND_QI, "pratec": TIEDTKE_PRATEC, "ktype": TIEDTKE_KTYPE}
# enum icar_hip_nsas_array (include/icar_hip.h)
NSAS_TEND_QC, NSAS_TEND_QI, NSAS_PRATEC, NSAS_HBOT, NSAS_HTOP, NSAS_HPBL, NSAS_N = range(7)
NSAS_NAMES = {"tend_qc": NSAS_TEND_QC, "tend_qi": NSAS_TEND_QI, "pratec": NSAS_PRATEC, "hbot": NSAS_HBOT, "htop": NSAS_HTOP, "hpbl": NSAS_HPBL}


def cu_var_request(options):
    """cu_driver.f90:43-91: the kVARS the Tiedtke, NSAS and BMJ branches allocate, advect and write to restart files"""
    if options.physics.convection == kCU_NSAS:                                       # :59-73
        options.alloc_vars(["water_vapor", "potential_temperature", "temperature", "cloud_water", "cloud_ice", "precipitation",
                            "convective_precipitation", "exner", "dz_interface", "density", "pressure_interface", "pressure",
                            "sensible_heat", "latent_heat", "u", "v", "w", "land_mask", "tend_qv", "tend_th", "tend_qc", "tend_qi", "tend_qs",
                            "tend_qr", "tend_u", "tend_v", "hpbl"])
        options.advect_vars(["potential_temperature", "water_vapor"])
        options.restart_vars(["water_vapor", "potential_temperature", "temperature", "cloud_water", "cloud_ice", "precipitation",
                              "convective_precipitation", "sensible_heat", "latent_heat", "u", "v", "pressure", "hpbl"])
        return
    if options.physics.convection == kCU_TIEDTKE:
        options.alloc_vars(["water_vapor", "potential_temperature", "temperature", "cloud_water", "cloud_ice", "precipitation",
                            "convective_precipitation", "exner", "dz_interface", "density", "pressure_interface", "pressure",
                            "sensible_heat", "latent_heat", "u", "v", "w", "land_mask", "tend_qv", "tend_th", "tend_qc", "tend_qi", "tend_qs",
                            "tend_qr", "tend_u", "tend_v", "tend_qv_pbl", "tend_qv_adv", "znu"])
        options.advect_vars(["potential_temperature", "water_vapor"])
        options.restart_vars(["water_vapor", "potential_temperature", "temperature", "cloud_water", "cloud_ice", "precipitation",
                              "convective_precipitation", "sensible_heat", "latent_heat", "u", "v", "pressure"])
        return
    if options.physics.convection != kCU_BMJ:
        return
    options.alloc_vars(["water_vapor", "potential_temperature", "temperature", "cloud_water", "cloud_ice", "precipitation",
                        "convective_precipitation", "exner", "dz_interface", "density", "pressure_interface", "pressure",
                        "sensible_heat", "latent_heat", "u", "v", "w", "land_mask", "tend_qv", "tend_th", "tend_qc", "tend_qi", "tend_qs",
                        "tend_qr", "tend_u", "tend_v", "kpbl"])
    options.advect_vars(["potential_temperature", "water_vapor"])
    options.restart_vars(["water_vapor", "potential_temperature", "temperature", "cloud_water", "cloud_ice", "precipitation",
                          "convective_precipitation", "sensible_heat", "latent_heat", "u", "v", "pressure", "kpbl"])


def cu_configure(domain, convection, stochastic_cu=float(kNO_STOCHASTIC), tendency_fraction=1.0, tend_qv_fraction=-1.0, tend_qc_fraction=-1.0,
                 tend_th_fraction=-1.0, tend_qi_fraction=-1.0):
    """icar_hip_cu_configure: options%physics%convection and options%cu_options; with kCU_BMJ the slot's arrays, BMJINIT's tables and
    the column workspace are made on the first call"""
    check(lib().icar_hip_cu_configure(domain.ctx, int(convection), float(stochastic_cu), float(tendency_fraction), float(tend_qv_fraction),
                                      float(tend_qc_fraction), float(tend_th_fraction), float(tend_qi_fraction)), "icar_hip_cu_configure")
    inherit = lambda f: float(tendency_fraction) if f < 0 else float(f)
    domain._cu_key = (0,) if int(convection) == 0 else (int(convection), float(stochastic_cu), float(tendency_fraction), inherit(tend_qv_fraction),
                                                       inherit(tend_qc_fraction), inherit(tend_th_fraction), inherit(tend_qi_fraction))


def cu_init(domain, convection, stochastic_cu=float(kNO_STOCHASTIC), tendency_fraction=1.0, tend_qv_fraction=-1.0, tend_qc_fraction=-1.0,
            tend_th_fraction=-1.0, tend_qi_fraction=-1.0, znu=None):
    """icar_hip_cu_init: init_convection with every scheme that is built.  0 and kCU_BMJ: what cu_configure does.  kCU_TIEDTKE: znu
    (default: domain.znu) goes to the device; tend%qc, tend%qi, PRATEC, KTYPE and the column workspace are made"""
    z = domain.znu if znu is None else znu
    if z is not None:
        z = np.ascontiguousarray(z, np.float32)
        if int(convection) == kCU_TIEDTKE and z.shape != (domain.nz,):
            raise ValueError(f"znu: shape {z.shape} != ({domain.nz},)")
    check(lib().icar_hip_cu_init(domain.ctx, int(convection), float(stochastic_cu), float(tendency_fraction), float(tend_qv_fraction),
                                 float(tend_qc_fraction), float(tend_th_fraction), float(tend_qi_fraction),
                                 None if z is None else z.ctypes.data_as(ctypes.c_void_p)), "icar_hip_cu_init")
    inherit = lambda f: float(tendency_fraction) if f < 0 else float(f)
    domain._cu_key = (0,) if int(convection) == 0 else (int(convection), float(stochastic_cu), float(tendency_fraction), inherit(tend_qv_fraction),
                                                       inherit(tend_qc_fraction), inherit(tend_th_fraction), inherit(tend_qi_fraction))


def convection_init(domain, convection, stochastic_cu=float(kNO_STOCHASTIC), tendency_fraction=1.0, tend_qv_fraction=-1.0, tend_qc_fraction=-1.0,
                    tend_th_fraction=-1.0, tend_qi_fraction=-1.0, znu=None, dx=None):
    """icar_hip_convection_init: init_convection with every scheme that is built.  0, kCU_BMJ and kCU_TIEDTKE: what cu_init does.
    kCU_NSAS: dx (default: domain.dx) is kept; tend%qc, tend%qi, PRATEC, HBOT, HTOP, hpbl and the column workspace are made"""
    z = domain.znu if znu is None else znu
    if z is not None:
        z = np.ascontiguousarray(z, np.float32)
        if int(convection) == kCU_TIEDTKE and z.shape != (domain.nz,):
            raise ValueError(f"znu: shape {z.shape} != ({domain.nz},)")
    d = float(getattr(domain, "dx", 0.0) if dx is None else dx)
    check(lib().icar_hip_convection_init(domain.ctx, int(convection), float(stochastic_cu), float(tendency_fraction), float(tend_qv_fraction),
                                         float(tend_qc_fraction), float(tend_th_fraction), float(tend_qi_fraction),
                                         None if z is None else z.ctypes.data_as(ctypes.c_void_p), d), "icar_hip_convection_init")
    inherit = lambda f: float(tendency_fraction) if f < 0 else float(f)
    domain._cu_key = (0,) if int(convection) == 0 else (int(convection), float(stochastic_cu), float(tendency_fraction), inherit(tend_qv_fraction),
                                                       inherit(tend_qc_fraction), inherit(tend_th_fraction), inherit(tend_qi_fraction))


def init_convection(domain, options):
    """init_convection (cu_driver.f90:97-253): the options to the library; CLDEFI = AVGEFI, the tables of BMJINIT; kCU_TIEDTKE goes
    to cu_init with domain.znu, kCU_NSAS to convection_init with domain.dx"""
    o = options.cu_options
    if options.physics.convection == kCU_NSAS:
        convection_init(domain, options.physics.convection, o.stochastic_cu, o.tendency_fraction, o.tend_qv_fraction, o.tend_qc_fraction,
                        o.tend_th_fraction, o.tend_qi_fraction)
        return
    if options.physics.convection == kCU_TIEDTKE:
        cu_init(domain, options.physics.convection, o.stochastic_cu, o.tendency_fraction, o.tend_qv_fraction, o.tend_qc_fraction,
                o.tend_th_fraction, o.tend_qi_fraction)
        return
    cu_configure(domain, options.physics.convection, o.stochastic_cu, o.tendency_fraction, o.tend_qv_fraction, o.tend_qc_fraction,
                 o.tend_th_fraction, o.tend_qi_fraction)


def convect(domain, options, dt):
    """convect(domain, options, dt) (cu_driver.f90:255-514) on the tile its..kte of the domain's grid; dt a REAL(4) like real(dt%seconds())"""
    if options.physics.convection == 0:
        return
    domain.configure(options)
    check(lib().icar_hip_convect(domain.ctx, float(dt)), "icar_hip_convect")


def cu_bmj(domain, dt, its, ite, jts, jte):
    """the call of BMJDRV alone (cu_driver.f90:434-465) on a range of columns, the levels those of the configured step (else kms..kme)"""
    check(lib().icar_hip_cu_bmj(domain.ctx, float(dt), int(its), int(ite), int(jts), int(jte)), "icar_hip_cu_bmj")


def cu_tiedtke(domain, dt, its, ite, jts, jte):
    """the call of CU_TIEDTKE alone (cu_driver.f90:303-330) on a range of columns, the levels those of the configured step (else kms..kme)"""
    check(lib().icar_hip_cu_tiedtke(domain.ctx, float(dt), int(its), int(ite), int(jts), int(jte)), "icar_hip_cu_tiedtke")


def cu_nsas(domain, dt, its, ite, jts, jte):
    """the call of cu_nsas alone (cu_driver.f90:363-417) on a range of columns, the levels those of the configured step (else kms..kme)"""
    check(lib().icar_hip_cu_nsas(domain.ctx, float(dt), int(its), int(ite), int(jts), int(jte)), "icar_hip_cu_nsas")


def _nsas_shape(domain, which):
    return (domain.ny, domain.nz, domain.nx) if which in (NSAS_TEND_QC, NSAS_TEND_QI) else (domain.ny, domain.nx)


def nsas_set(domain, name, array):
    which = NSAS_NAMES[name] if isinstance(name, str) else int(name)
    a = np.ascontiguousarray(array, np.float32)
    if a.shape != _nsas_shape(domain, which):
        raise ValueError(f"{name}: shape {a.shape} != {_nsas_shape(domain, which)}")
    check(lib().icar_hip_nsas_upload(domain.ctx, which, a.ctypes.data_as(ctypes.c_void_p)), f"icar_hip_nsas_upload {name}")


def nsas_get(domain, name):
    which = NSAS_NAMES[name] if isinstance(name, str) else int(name)
    a = np.empty(_nsas_shape(domain, which), np.float32)
    check(lib().icar_hip_nsas_download(domain.ctx, which, a.ctypes.data_as(ctypes.c_void_p)), f"icar_hip_nsas_download {name}")
    return a


def _tiedtke_shape(domain, which):
    return (domain.ny, domain.nz, domain.nx) if which in (TIEDTKE_TEND_QC, TIEDTKE_TEND_QI) else (domain.ny, domain.nx)


def tiedtke_set(domain, name, array):
    which = TIEDTKE_NAMES[name] if isinstance(name, str) else int(name)
    a = np.ascontiguousarray(array, np.int32 if which == TIEDTKE_KTYPE else np.float32)
    if a.shape != _tiedtke_shape(domain, which):
        raise ValueError(f"{name}: shape {a.shape} != {_tiedtke_shape(domain, which)}")
    check(lib().icar_hip_tiedtke_upload(domain.ctx, which, a.ctypes.data_as(ctypes.c_void_p)), f"icar_hip_tiedtke_upload {name}")


def tiedtke_get(domain, name):
    which = TIEDTKE_NAMES[name] if isinstance(name, str) else int(name)
    a = np.empty(_tiedtke_shape(domain, which), np.int32 if which == TIEDTKE_KTYPE else np.float32)
    check(lib().icar_hip_tiedtke_download(domain.ctx, which, a.ctypes.data_as(ctypes.c_void_p)), f"icar_hip_tiedtke_download {name}")
    return a


def cu_reset(domain):
    """CLDEFI = AVGEFI, accumulated_convective_pcp = 0"""
    check(lib().icar_hip_cu_reset(domain.ctx), "icar_hip_cu_reset")


def _shape(domain, which):
    return (domain.ny, domain.nz, domain.nx) if which in (CU_TEND_TH, CU_TEND_QV) else (domain.ny, domain.nx)


def cu_set(domain, name, array):
    which = CU_NAMES[name] if isinstance(name, str) else int(name)
    a = np.ascontiguousarray(array, np.float32)
    if a.shape != _shape(domain, which):
        raise ValueError(f"{name}: shape {a.shape} != {_shape(domain, which)}")
    check(lib().icar_hip_cu_upload(domain.ctx, which, a.ctypes.data_as(ctypes.c_void_p)), f"icar_hip_cu_upload {name}")


def cu_get(domain, name):
    which = CU_NAMES[name] if isinstance(name, str) else int(name)
    a = np.empty(_shape(domain, which), np.float32)
    check(lib().icar_hip_cu_download(domain.ctx, which, a.ctypes.data_as(ctypes.c_void_p)), f"icar_hip_cu_download {name}")
    return a


def cu_tables(domain):
    """{name: array (C order: the Fortran shape reversed)} of BMJINIT's tables as they sit on the device"""
    n = ctypes.c_size_t()
    check(lib().icar_hip_cu_tables(domain.ctx, None, 0, ctypes.byref(n)), "icar_hip_cu_tables")
    block = np.empty(n.value, np.float32)
    check(lib().icar_hip_cu_tables(domain.ctx, block.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)), "icar_hip_cu_tables")
    out, o = {}, 0
    for name, shape in CU_TABLES:
        cnt = int(np.prod(shape))
        out[name] = block[o:o + cnt].reshape(shape[::-1]).copy()
        o += cnt
    return out


def cu_finalize(options, domain=None):
    """the slot is switched off (its arrays stay until the context goes)"""
    if domain is not None:
        cu_configure(domain, 0)
