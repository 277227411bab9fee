// TEST INFRASTRUCTURE - not part of the product.  The host-only part of the C ABI (readmap.inc, rowsbatch.inc, signalplan.inc, bedtext.inc: the
// alignment walk, the row builder of a worker batch, the plan of a signal batch, the BED formatter) compiled by gcc with
// -fsanitize=address,undefined, so that tests/test_asan_host.py can drive it with valid and with corrupted container tables and see every
// out-of-bounds access, and the stand-alone drivers (tests/*_asan_driver.cpp) can include it as it is.
// The sources are the product's own files, included where they lie, and their declarations are the product's (csrc/host.h, its part that
// needs no HIP); only the definition of the error slot, which the product keeps in deepmod_hip.hip, is restated here.
#include "../../deepmod_amd/csrc/host.h"

namespace dmhost {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

}  // namespace dmhost

extern "C" const char* dm_last_error(void) { return g_err.c_str(); }

#include "../../deepmod_amd/csrc/readmap.inc"
#include "../../deepmod_amd/csrc/rowsbatch.inc"
#include "../../deepmod_amd/csrc/signalplan.inc"
#include "../../deepmod_amd/csrc/bedtext.inc"
