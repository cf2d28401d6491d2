// FsrEasuCon of the reference's ffx_fsr1.h, included the way the plugin's FSREffect.cpp includes it and called with its argument list
// (test infrastructure only; compiled by `make -C oracle ref` with the reference's effects directory on the include path).
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include "ffx_a.h"
#include "ffx_fsr1.h"

extern "C" void ffx_ref_easu_con(float rw, float rh, float W, float H, float ow, float oh, uint32_t* con)
{
    AU1 c[4][4] = {};
    FsrEasuCon(c[0], c[1], c[2], c[3], rw, rh, W, H, ow, oh);
    for (int i = 0; i < 16; i++) con[i] = c[i / 4][i % 4];
}
