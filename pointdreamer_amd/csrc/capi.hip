// libpdhip: version + thread-local error message (never throws across the C ABI).
#include "common.h"
#include <string.h>

namespace pdhip {
static thread_local char g_err[512] = "";
int g_lab_units = 0;
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---- the carve log (common.h): the calling thread's Carve::take calls since the log was switched on, at most CARVE_LOG_CAP of them kept
__thread int g_carve_log = 0;
static constexpr int CARVE_LOG_CAP = 256;
static thread_local struct { const void* base; size_t off, bytes; } g_carve_regions[CARVE_LOG_CAP];
static thread_local int g_carve_count = 0;                 // recorded + dropped
void carve_record(const void* base, size_t off, size_t bytes) {
    if (g_carve_count < CARVE_LOG_CAP) g_carve_regions[g_carve_count] = {base, off, bytes};
    ++g_carve_count;
}
}  // namespace pdhip

extern "C" int pdhip_debug_carve_log(int on) {
    const int old = pdhip::g_carve_log;
    pdhip::g_carve_log = on ? 1 : 0;
    pdhip::g_carve_count = 0;
    return old;
}
extern "C" int pdhip_debug_carve_log_read(uint64_t* triples, int capacity) {
    const int kept = pdhip::g_carve_count < pdhip::CARVE_LOG_CAP ? pdhip::g_carve_count : pdhip::CARVE_LOG_CAP;
    for (int i = 0; triples && i < kept && i < capacity; ++i) {
        triples[3 * i + 0] = (uint64_t)(uintptr_t)pdhip::g_carve_regions[i].base;
        triples[3 * i + 1] = (uint64_t)pdhip::g_carve_regions[i].off;
        triples[3 * i + 2] = (uint64_t)pdhip::g_carve_regions[i].bytes;
    }
    return pdhip::g_carve_count;
}

extern "C" int pdhip_version(void) { return 211; }
// number of translation units of THIS library that were compiled with a wrong-result PD_LAB_* switch (common.h); 0 for a product build
extern "C" int pdhip_lab_build(void) { return pdhip::g_lab_units; }
extern "C" const char* pdhip_last_error(void) { return pdhip::g_err; }
