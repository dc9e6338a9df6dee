// mxfp4_capi.cpp — host-only C API over mxfp4_host.h.
//
// Built by g++ into libmi355x_mxfp4.so with no HIP dependency, so the
// quantizer can be loaded and tested on any machine.

#include "mxfp4_host.h"

static char g_mxfp4_error[256] = "";

extern "C" {

const char* lg_mxfp4_last_error() { return g_mxfp4_error; }

// x[rows][k] f32 -> packed[rows][k/2], scales[rows][k/32] and (optional)
// deq[rows][k]. Returns 0, or -1 with lg_mxfp4_last_error() set.
int lg_mxfp4_quantize(const float* x, int rows, int k, unsigned char* packed,
                      unsigned char* scales, float* deq_or_null)
{
    return mxfp4::quantize(x, rows, k, packed, scales, deq_or_null,
                           g_mxfp4_error, sizeof(g_mxfp4_error));
}

}  // extern "C"
