// The host side of libapstyle.so -- the argument checks and launch planners of animateportrait_amd/csrc/style/style_checks.h --
// as a stand-alone program, so that it can run under the host sanitisers.  No device, no HIP:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/style_host_check.cpp -o style_host_check
//   ./style_host_check
//
// It sweeps every call over the corners of its served region and past each limit, with pointers that are never dereferenced
// (any non-null value stands in), and checks what a plan promises: one workgroup per output plane, a workgroup size the kernels
// are built for, an output plane inside the caller's tensor, a message for every refusal.  Exit status 0: all held.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../animateportrait_amd/csrc/style/style_checks.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, long a = 0, long b = 0, long c = 0, long d = 0) {
    if (ok) return;
    ++failures;
    fprintf(stderr, "FAILED: %s (%ld %ld %ld %ld); last message: %s\n", what, a, b, c, d, aps::err_buf());
}

const void* const P = reinterpret_cast<const void*>(0x100000);

void plan_holds(const aps::PlanePlan& pl, long planes, long oh, long ow) {
    expect(pl.planes == planes && pl.planes >= 1 && pl.planes <= APS_MAX_PLANES, "one workgroup per plane", pl.planes, planes);
    expect(pl.threads == 256 || pl.threads == 1024, "workgroup size", pl.threads);
    expect(pl.OH == oh && pl.OW == ow, "output plane", pl.OH, pl.OW, oh, ow);
    expect((long long)pl.planes * pl.OH * pl.OW <= APS_MAX_ELEMS, "output inside the index range");
}

void refused(int rc, const char* what) {
    expect(rc < 0 && strlen(aps::err_buf()) > 0, what, rc);
    aps::err_buf()[0] = 0;
}

}  // namespace

int main() {
    const int sides[] = {1, 2, 3, 5, 7, 16, 64, 255, 256, 257, 4095, APS_MAX_SIDE, APS_MAX_SIDE + 1};
    const int chans[] = {1, 2, 3, 4, 6, 8, 128, 4096};
    const int batch[] = {1, 2, 16, 65535, 65536};
    long served = 0, turned_down = 0;
    for (int N : batch)
        for (int C : chans)
            for (int H : sides)
                for (int W : sides) {
                    const long long planes = (long long)N * C, elems = planes * H * W;
                    const bool shape_ok = H <= APS_MAX_SIDE && W <= APS_MAX_SIDE && planes <= APS_MAX_PLANES && elems <= APS_MAX_ELEMS;
                    aps::PlanePlan pl{};
                    // lin_coeffs
                    int rc = aps::plan_lin_coeffs(P, P, P, P, P, P, P, N, C, H, W, N > 1, &pl);
                    if (shape_ok && (long)H * W >= 2) { expect(rc == APS_OK, "lin_coeffs serves", N, C, H, W); plan_holds(pl, planes, H, W); ++served; }
                    else { refused(rc, "lin_coeffs refuses"); ++turned_down; }
                    // affine_apply, with and without statistics
                    for (int stats = 0; stats < 2; ++stats) {
                        rc = aps::plan_affine_apply(P, P, P, P, stats ? P : nullptr, stats ? P : nullptr, N, C, H, W, stats, &pl);
                        if (shape_ok) { expect(rc == APS_OK, "affine_apply serves", N, C, H, W); plan_holds(pl, planes, H, W); ++served; }
                        else { refused(rc, "affine_apply refuses"); ++turned_down; }
                    }
                    // plane_combine
                    for (int mode = APS_JOIN; mode <= APS_STAT; ++mode) {
                        const bool stat = mode == APS_STAT;
                        rc = aps::plan_plane_combine(mode, P, P, P, P, N, C, H, W, 2 * H, 2 * W, 0, stat ? nullptr : P, P, stat ? nullptr : P, &pl);
                        bool ok = shape_ok;
                        long oh = H, ow = W;
                        if (mode == APS_JOIN) ok = ok && C % 4 == 0;
                        if (mode == APS_POOL2) { ok = ok && H >= 2 && W >= 2; oh = H / 2; ow = W / 2; }
                        if (mode == APS_UP2ADD) {
                            oh = 2L * H; ow = 2L * W;
                            ok = ok && oh <= APS_MAX_SIDE && ow <= APS_MAX_SIDE && planes * oh * ow <= APS_MAX_ELEMS;
                        }
                        if (ok) { expect(rc == APS_OK, "plane_combine serves", mode, N * (long)C, H, W); plan_holds(pl, planes, oh, ow); ++served; }
                        else { refused(rc, "plane_combine refuses"); ++turned_down; }
                    }
                }
    // the refusals that do not depend on the shape
    aps::PlanePlan pl{};
    refused(aps::plan_lin_coeffs(nullptr, P, P, P, P, P, P, 1, 4, 8, 8, 0, &pl), "null x");
    refused(aps::plan_lin_coeffs(P, P, P, P, nullptr, P, P, 1, 4, 8, 8, 0, &pl), "null workspace");
    refused(aps::plan_lin_coeffs(P, P, P, P, P, P, P, 1, 4, 8, 8, 2, &pl), "per_sample flag");
    refused(aps::plan_lin_coeffs(P, P, P, P, P, P, P, 1, 4, 1, 1, 0, &pl), "H W = 1");
    refused(aps::plan_lin_coeffs(P, P, P, P, P, P, P, -1, 4, 8, 8, 0, &pl), "negative N");
    refused(aps::plan_affine_apply(P, P, P, nullptr, nullptr, nullptr, 1, 4, 8, 8, 0, &pl), "null y");
    refused(aps::plan_affine_apply(P, P, P, P, P, nullptr, 1, 4, 8, 8, 0, &pl), "half a statistics pair");
    refused(aps::plan_affine_apply(P, P, P, P, nullptr, nullptr, 1, 4, 8, 8, 7, &pl), "activation");
    refused(aps::plan_plane_combine(-1, P, P, P, P, 1, 4, 8, 8, 0, 0, 0, P, nullptr, nullptr, &pl), "mode below");
    refused(aps::plan_plane_combine(5, P, P, P, P, 1, 4, 8, 8, 0, 0, 0, P, nullptr, nullptr, &pl), "mode above");
    refused(aps::plan_plane_combine(APS_JOIN, P, P, nullptr, P, 1, 4, 8, 8, 0, 0, 0, P, nullptr, nullptr, &pl), "JOIN null part");
    refused(aps::plan_plane_combine(APS_JOIN, P, P, P, P, 1, 6, 8, 8, 0, 0, 0, P, nullptr, nullptr, &pl), "JOIN C % 4");
    refused(aps::plan_plane_combine(APS_UP2ADD, P, P, nullptr, nullptr, 1, 4, 8, 8, 16, 15, 0, P, nullptr, nullptr, &pl), "UP2ADD skip shape");
    refused(aps::plan_plane_combine(APS_UP2ADD, P, P, nullptr, nullptr, 1, 4, 8, 8, 8, 8, 0, P, nullptr, nullptr, &pl), "UP2ADD skip of the input's size");
    refused(aps::plan_plane_combine(APS_SUM3, P, P, nullptr, nullptr, 1, 4, 8, 8, 0, 0, 0, P, nullptr, nullptr, &pl), "SUM3 null term");
    refused(aps::plan_plane_combine(APS_SUM3, P, P, P, nullptr, 1, 4, 8, 8, 0, 0, 1, P, nullptr, nullptr, &pl), "flags outside STAT");
    refused(aps::plan_plane_combine(APS_STAT, P, nullptr, nullptr, nullptr, 1, 4, 8, 8, 0, 0, 2, nullptr, P, nullptr, &pl), "STAT flags");
    refused(aps::plan_plane_combine(APS_STAT, P, nullptr, nullptr, nullptr, 1, 4, 8, 8, 0, 0, 0, P, P, nullptr, &pl), "STAT with y");
    refused(aps::plan_plane_combine(APS_STAT, P, nullptr, nullptr, nullptr, 1, 4, 8, 8, 0, 0, 0, nullptr, nullptr, nullptr, &pl), "STAT without mean_out");
    expect(aps::plan_plane_combine(APS_UP2ADD, P, nullptr, nullptr, nullptr, 1, 4, 8, 8, 0, 0, 0, P, nullptr, nullptr, &pl) == APS_OK, "null skip");
    expect(aps::plan_plane_combine(APS_STAT, P, nullptr, nullptr, nullptr, 2, 128, 64, 64, 0, 0, APS_STAT_RELU, nullptr, P, nullptr, &pl) == APS_OK, "STAT relu");
    // messages never overrun the buffer: the longest one, with the largest numbers
    refused(aps::check_shape("plane_combine UP2ADD output", 2147483647, 2147483647, 2147483647, 2147483647), "huge");
    printf("style_host_check: %ld plans served, %ld refused, %d failures\n", served, turned_down, failures);
    return failures ? 1 : 0;
}
