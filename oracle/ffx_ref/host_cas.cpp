// CasSetup of the reference's ffx_cas.h, included the way the plugin's CASEffect.cpp includes it and called with its argument list
// (test infrastructure only; compiled by `make -C oracle ref` with the reference's effects directory on the include path).
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include "ffx_a.h"
#include "ffx_cas.h"

extern "C" void ffx_ref_cas_setup(float sharpness, uint32_t* const1)
{
    AU1 tmp[4] = {0, 0, 0, 0}, c1[4] = {0, 0, 0, 0};
    CasSetup(tmp, c1, sharpness, 0.0f, 0.0f, 0.0f, 0.0f);
    for (int i = 0; i < 4; i++) const1[i] = c1[i];
}
