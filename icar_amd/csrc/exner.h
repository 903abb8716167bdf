// icar_amd/csrc/exner.h -- exner_function (atm_utilities.f90:682-691), one definition for diagnostic_update's cell kernel (step.hip)
// and for the Thompson launches that compute exner from the pressure themselves (mp_thompson.hip): a sub-step's results are the
// same bits either way only while both evaluate this one expression.  Include after glibc_flt32.h (with or without its tables in LDS).
#pragma once
constexpr float ICAR_RD = 287.058f, ICAR_CP = 1012.0f;     // Rd, cp: src/constants/icar_constants.f90:391-393

// (p/po)**(Rd/cp): the C library's powf, bit for bit what the compiled reference computes; po = 100000 (an integer in the
// reference => p/100000.), IEEE division
__device__ __forceinline__ float exner_function(float pressure)
{
    return gf_powf(pressure / 100000.0f, ICAR_RD / ICAR_CP);
}
