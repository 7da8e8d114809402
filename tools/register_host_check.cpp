// Stand-alone host program for tools/register_host_check.py: the argument checks of apq_rigid_register
// (csrc/seq/seq_register_checks.h), compiled for the host with -fsanitize=address,undefined.  Every case calls
// apq::check_rigid_register on addresses inside (or deliberately beside) real allocations of the sizes the call would touch and
// compares the code and the message with what the case expects; the checks never dereference a pointer, which the sanitiser
// would report if they did on the one-past and misaligned addresses used here.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../animateportrait_amd/csrc/seq/seq_register_checks.h"

namespace {

int failures = 0;

void expect(const char* what, int rc, int want_rc, const char* want_text) {
    const char* msg = rc == APQ_OK ? "" : apq::err_buf();
    const bool ok = rc == want_rc && (want_rc == APQ_OK || strstr(msg, want_text) != nullptr);
    printf("%-44s rc %2d %s%s\n", what, rc, ok ? "ok" : "FAILED: ", ok ? "" : msg);
    if (!ok) ++failures;
}

}  // namespace

int main() {
    const int T = 130;
    std::vector<float> in((size_t)T * APQ_LM_C), out((size_t)T * APQ_LM_C), std_face(APQ_LM_C);
    std::vector<double> pose((size_t)T * 12);
    float *pi = in.data(), *po = out.data(), *ps = std_face.data();
    double* pp = pose.data();
    const int all = APQ_REG_CENTER | APQ_REG_NO_X_ROT;

    // served
    for (int flags : {0, APQ_REG_CENTER, APQ_REG_NO_X_ROT, all, APQ_REG_REGISTER}) {
        expect("served, pose, separate", apq::check_rigid_register(pi, ps, po, pp, T, flags), APQ_OK, "");
        expect("served, no pose, in place", apq::check_rigid_register(pi, ps, pi, nullptr, T, flags), APQ_OK, "");
    }
    expect("served, T = 1", apq::check_rigid_register(pi, ps, po, pp, 1, all), APQ_OK, "");
    expect("served, out right behind in", apq::check_rigid_register(pi, ps, pi + 65 * APQ_LM_C, nullptr, 65, all), APQ_OK, "");
    expect("served, in right behind out", apq::check_rigid_register(pi + 65 * APQ_LM_C, ps, pi, nullptr, 65, all), APQ_OK, "");
    // (addresses only: 65536 rows reach far past any allocation made here)
    const float* const far_rows = reinterpret_cast<const float*>((uintptr_t)1 << 40);
    const float* const far_std = reinterpret_cast<const float*>((uintptr_t)1 << 39);
    expect("served, T = APQ_MAX_T", apq::check_rigid_register(far_rows, far_std, far_rows, nullptr, APQ_MAX_T, all), APQ_OK, "");

    // refused, by name
    expect("null in", apq::check_rigid_register(nullptr, ps, po, pp, T, all), APQ_ERR_INVALID, "null in");
    expect("null std", apq::check_rigid_register(pi, nullptr, po, pp, T, all), APQ_ERR_INVALID, "null std");
    expect("null out", apq::check_rigid_register(pi, ps, nullptr, pp, T, all), APQ_ERR_INVALID, "null out");
    expect("T = 0", apq::check_rigid_register(pi, ps, po, pp, 0, all), APQ_ERR_INVALID, "T = 0");
    expect("T = -5", apq::check_rigid_register(pi, ps, po, pp, -5, all), APQ_ERR_INVALID, "T = -5");
    expect("T above the grid", apq::check_rigid_register(pi, ps, pi, nullptr, APQ_MAX_T + 1, all), APQ_ERR_UNSUPPORTED, "T = 65537");
    expect("unknown flag", apq::check_rigid_register(pi, ps, po, pp, T, 8), APQ_ERR_INVALID, "unknown flags = 8");
    expect("negative flags", apq::check_rigid_register(pi, ps, po, pp, T, -1), APQ_ERR_INVALID, "unknown flags");
    expect("register + center", apq::check_rigid_register(pi, ps, po, pp, T, APQ_REG_REGISTER | APQ_REG_CENTER), APQ_ERR_INVALID, "excludes");
    expect("register + no_x_rot", apq::check_rigid_register(pi, ps, po, pp, T, APQ_REG_REGISTER | APQ_REG_NO_X_ROT), APQ_ERR_INVALID, "excludes");
    const char* odd = reinterpret_cast<const char*>(pi) + 2;
    expect("misaligned in", apq::check_rigid_register(odd, ps, po, pp, T - 1, all), APQ_ERR_UNSUPPORTED, "in is not 4-byte");
    expect("misaligned std", apq::check_rigid_register(pi, reinterpret_cast<const char*>(ps) + 1, po, pp, T, all), APQ_ERR_UNSUPPORTED, "std is not 4-byte");
    expect("misaligned out", apq::check_rigid_register(pi, ps, reinterpret_cast<const char*>(po) + 2, pp, T - 1, all), APQ_ERR_UNSUPPORTED, "out is not 4-byte");
    expect("misaligned pose", apq::check_rigid_register(pi, ps, po, reinterpret_cast<const char*>(pp) + 4, T - 1, all), APQ_ERR_UNSUPPORTED, "pose is not 8-byte");
    expect("out one row into in", apq::check_rigid_register(pi, ps, pi + APQ_LM_C, nullptr, T - 1, all), APQ_ERR_INVALID, "out overlaps in");
    expect("out one float before in", apq::check_rigid_register(pi + 1, ps, pi, nullptr, T - 1, all), APQ_ERR_INVALID, "out overlaps in");
    expect("out last float on in's first", apq::check_rigid_register(pi + 65 * APQ_LM_C - 1, ps, pi, nullptr, 65, all), APQ_ERR_INVALID, "out overlaps in");
    expect("std inside out", apq::check_rigid_register(pi, po + 7 * APQ_LM_C, po, pp, T, all), APQ_ERR_INVALID, "out overlaps std");
    expect("pose inside out", apq::check_rigid_register(pi, ps, po, reinterpret_cast<double*>(po + 2), 10, all), APQ_ERR_INVALID, "pose overlaps out");
    expect("pose inside in", apq::check_rigid_register(pi, ps, po, reinterpret_cast<double*>(pi + 2), 10, all), APQ_ERR_INVALID, "pose overlaps in");
    expect("pose on std", apq::check_rigid_register(pi, ps, po, reinterpret_cast<double*>(ps), 1, all), APQ_ERR_INVALID, "pose overlaps std");

    printf(failures ? "FAILED: %d cases\n" : "all cases as expected\n", failures);
    return failures ? 1 : 0;
}
