// What the translation units of libapdata.so share: the thread-local error message apd_last_error() returns.
#pragma once

namespace apd {

extern thread_local char g_err[256];

// writes the message, returns `code`
int fail(int code, const char* fmt, long a = 0, long b = 0, long c = 0, long d = 0);

}  // namespace apd
