"""radiation driver mirror (src/physics/ra_driver.f90): ra_var_request / rad_init / rad, plus ra_simple on an explicit tile and
the calendar anchor the library needs of domain%model_time.

Only the simple scheme (kRA_SIMPLE, src/physics/ra_simple.f90: Reiff et al. 1984 shortwave, Idso and Jackson 1969 longwave, Xu and
Randall 1996 cloud fraction) is built; kRA_BASIC has no branch in the reference's driver either, kRA_RRTMG is refused by the
library."""
from .capi import lib, check
from .constants import kRA_SIMPLE

GREGORIAN, NOLEAP, THREESIXTY = 0, 1, 2                 # time_h.f90:22


def ra_var_request(options):
    """ra_driver.f90:110-129 (ra_simple_var_request), as written."""
    if options.physics.radiation == kRA_SIMPLE:
        options.alloc_vars(["pressure", "potential_temperature", "exner", "cloud_fraction", "water_vapor", "cloud_water", "rain_in_air",
                            "snow_in_air", "shortwave", "longwave", "cloud_ice", "graupel_in_air"])
        options.advect_vars(["potential_temperature"])
        options.restart_vars(["pressure", "potential_temperature", "shortwave", "longwave", "cloud_fraction"])


def _days_from_civil(y, m, d):
    """days since 1970-01-01 of a proleptic Gregorian date (integer arithmetic)"""
    y -= m <= 2
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m + (-3 if m > 2 else 9)) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


_NOLEAP_START = [0, 31, 59, 90, 120, 151, 181, 212, 243, 273, 304, 334]


def calendar_anchor(year, month, day, hour=0, minute=0, second=0, calendar=GREGORIAN):
    """(seconds since 1 January 00:00 of `year`, days of `year`, days of `year + 1`) of a date, from integer arithmetic: what
    icar_hip_rad_calendar takes, with year_start_seconds = model clock at that date - the first number."""
    if calendar == GREGORIAN:
        start = _days_from_civil(year, 1, 1)
        days = _days_from_civil(year, month, day) - start
        yd, nyd = _days_from_civil(year + 1, 1, 1) - start, _days_from_civil(year + 2, 1, 1) - _days_from_civil(year + 1, 1, 1)
    elif calendar == NOLEAP:
        days, yd, nyd = _NOLEAP_START[month - 1] + day - 1, 365, 365
    elif calendar == THREESIXTY:
        days, yd, nyd = (month - 1) * 30 + day - 1, 360, 360
    else:
        raise ValueError("calendar is GREGORIAN (0), NOLEAP (1) or THREESIXTY (2)")
    return days * 86400 + hour * 3600 + minute * 60 + second, yd, nyd


def rad_calendar(domain, calendar, year_start_seconds, year_days, next_year_days):
    """icar_hip_rad_calendar: the calendar and, on the library's clock (domain.model_time_seconds), 1 January 00:00 of the model
    time's year with the lengths of that year and the next."""
    check(lib().icar_hip_rad_calendar(domain.ctx, int(calendar), float(year_start_seconds), float(year_days), float(next_year_days)), "icar_hip_rad_calendar")


def rad_init(domain, options, date=None, calendar=GREGORIAN):
    """radiation_init (ra_driver.f90:167-195) -> ra_simple_init (ra_simple.f90:62-81: cos_lat_m / sin_lat_m, made on the device from
    ICAR_F_LATITUDE at the first call): hands options%physics%radiation to the library.  date = (year, month, day, hour, minute,
    second) of the model clock's present value sets the calendar anchor as well."""
    check(lib().icar_hip_rad_configure(domain.ctx, int(options.physics.radiation)), "icar_hip_rad_configure")
    domain._rad_key = int(options.physics.radiation)
    if date is not None:
        into, yd, nyd = calendar_anchor(*date, calendar=calendar)
        rad_calendar(domain, calendar, domain.model_time_seconds - into, yd, nyd)


def rad(domain, options, dt):
    """rad(domain, options, dt) (ra_driver.f90:197-285): ra_simple with F_runlw on the tile its..kte of the domain's grid, dt a
    REAL(4) like real(dt%seconds())."""
    if options.physics.radiation != kRA_SIMPLE:
        return
    domain.configure(options)
    check(lib().icar_hip_rad(domain.ctx, float(dt)), "icar_hip_rad")


def ra_simple(domain, dt, its, ite, jts, jte, kts, kte, runlw=True):
    """ra_simple(...) (ra_simple.f90:191-272) on an explicit tile of the domain's fields (icar_hip_ra_simple) at the model clock."""
    check(lib().icar_hip_ra_simple(domain.ctx, float(dt), int(its), int(ite), int(jts), int(jte), int(kts), int(kte), int(bool(runlw))), "icar_hip_ra_simple")


def rad_finalize(options, domain=None):
    """the scheme is switched off (the context frees cos_lat_m / sin_lat_m when it is destroyed)"""
    if domain is not None:
        check(lib().icar_hip_rad_configure(domain.ctx, 0), "icar_hip_rad_configure")
        domain._rad_key = 0
