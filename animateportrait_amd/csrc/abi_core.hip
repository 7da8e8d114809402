// abi_core.hip -- what the whole library shares behind its C ABI: the thread-local error text (common.h: fail, last_error_buf)
// and the version queries.
#include "common.h"

namespace apamd {

static thread_local char g_err[512];
char* last_error_buf() { return g_err; }
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace apamd

using namespace apamd;

extern "C" {

const char* ap_version(void) { return "animateportrait_amd 0.3 (gfx950)"; }
int32_t ap_abi_version(void) { return AP_ABI_VERSION; }
const char* ap_last_error(void) { return last_error_buf(); }

int32_t ap_switch_names(int32_t kind, char* buf, int32_t cap) {
    if (kind < SWK_ROUTE || kind > SWK_BUILD_ONLY || (!buf && cap > 0)) return fail(AP_ERR_INVALID, "switch_names: kind %d", kind);
    int32_t need = 1;
    for (int s = 0; s < SW_COUNT; ++s)
        if (switch_row(s).kind == kind) need += (int32_t)strlen(switch_row(s).name) + 1;
    if (need > cap) return need;
    char* p = buf;
    for (int s = 0; s < SW_COUNT; ++s)
        if (switch_row(s).kind == kind) p += sprintf(p, "%s\n", switch_row(s).name);
    *p = 0;
    return need;
}

}  // extern "C"
