// The part of common.h that needs no HIP: what host-only code (scan_plan.h, and through it the stand-alone scan_plan_check.cpp)
// shares with the translation units of libbasic_hip.so.  common.h includes it; nothing here may include a HIP header.
#pragma once
#include <string>

#include "../../include/basic_hip.h"

namespace basic {

// The library defines it in core.hip (basic_last_error reports the message); a stand-alone program brings its own.
void set_error(const std::string &msg);

#define BASIC_REQUIRE(cond, msg)            \
    do {                                    \
        if (!(cond)) {                      \
            ::basic::set_error(msg);        \
            return BASIC_ERR_INVALID;       \
        }                                   \
    } while (0)

// Canonical summation block of the masked convolution (mconv.hip header comment): channels of one (tap, input group) slab
// whose products form ONE fp32 MFMA / FMA chain; the persistent scan-line kernel (scanline.hip) sums in the same blocks.
#define BASIC_MCONV_BLOCK_CHANNELS 64

}  // namespace basic
