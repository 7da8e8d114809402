// The argument checks of apq_mel_frames / apq_speaker_head (csrc/seq/seq_speaker_checks.h) in a stand-alone host program, for the
// host sanitisers: no device, no Python.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/seq_speaker_host_check.cpp -o /tmp/spk_check && /tmp/spk_check
#include <stdio.h>
#include <string.h>

#include "../animateportrait_amd/csrc/seq/seq_speaker_checks.h"

static int failures = 0;

static void expect(int got, int want, const char* reason, const char* what) {
    const bool named = !reason || strstr(apq::err_buf(), reason) != nullptr;
    if (got != want || !named) {
        printf("FAIL %s: code %d (want %d), message '%s' (want '%s')\n", what, got, want, apq::err_buf(), reason ? reason : "");
        ++failures;
    }
}

int main() {
    alignas(16) static char mem[64];
    const void* a = mem;
    const void* odd4 = mem + 2;
    const void* odd8 = mem + 4;

    // mel frames: the served region's corners, then one refusal per rule
    expect(apq::check_mel_frames(a, a, a, a, 25600, 400, 160, 40, 2), APQ_OK, nullptr, "mel 400/160/40");
    expect(apq::check_mel_frames(a, a, a, a, 201, 400, 160, 40, 2), APQ_OK, nullptr, "mel L = 201");
    expect(apq::check_mel_frames(a, a, a, a, 513, 1024, 256, 80, 1), APQ_OK, nullptr, "mel 1024/256/80");
    expect(apq::check_mel_frames(a, a, a, a, 9, 16, 16, 1, 1), APQ_OK, nullptr, "mel 16/16/1");
    expect(apq::check_mel_frames(a, a, a, a, 2147483647, 1024, 1024, 128, 2), APQ_ERR_UNSUPPORTED, "T = 2097152", "mel L = INT_MAX");
    expect(apq::check_mel_frames(a, a, a, a, 2147483647, 400, 1, 40, 2), APQ_ERR_UNSUPPORTED, "T = 2147483648", "mel hop 1 at INT_MAX");
    expect(apq::check_mel_frames(a, a, a, a, 160 * 65535 + 159, 400, 160, 40, 2), APQ_OK, nullptr, "mel T = 65536");
    expect(apq::check_mel_frames(nullptr, a, a, a, 25600, 400, 160, 40, 2), APQ_ERR_INVALID, "null x", "mel null x");
    expect(apq::check_mel_frames(a, nullptr, a, a, 25600, 400, 160, 40, 2), APQ_ERR_INVALID, "null window", "mel null window");
    expect(apq::check_mel_frames(a, a, nullptr, a, 25600, 400, 160, 40, 2), APQ_ERR_INVALID, "null basis", "mel null basis");
    expect(apq::check_mel_frames(a, a, a, nullptr, 25600, 400, 160, 40, 2), APQ_ERR_INVALID, "null out", "mel null out");
    expect(apq::check_mel_frames(a, a, a, a, 0, 400, 160, 40, 2), APQ_ERR_INVALID, "L = 0", "mel L = 0");
    expect(apq::check_mel_frames(a, a, a, a, -2147483647 - 1, 400, 160, 40, 2), APQ_ERR_INVALID, "L = -2147483648", "mel L = INT_MIN");
    expect(apq::check_mel_frames(a, a, a, a, 25600, 400, 0, 40, 2), APQ_ERR_INVALID, "hop = 0", "mel hop 0");
    expect(apq::check_mel_frames(a, a, a, a, 25600, 400, 160, 0, 2), APQ_ERR_INVALID, "n_mels = 0", "mel n_mels 0");
    expect(apq::check_mel_frames(a, a, a, a, 25600, 400, 160, 40, 3), APQ_ERR_INVALID, "power = 3", "mel power 3");
    expect(apq::check_mel_frames(a, a, a, a, 25600, 401, 160, 40, 2), APQ_ERR_UNSUPPORTED, "is odd", "mel odd n_fft");
    expect(apq::check_mel_frames(a, a, a, a, 25600, 1026, 160, 40, 2), APQ_ERR_UNSUPPORTED, "n_fft = 1026", "mel n_fft 1026");
    expect(apq::check_mel_frames(a, a, a, a, 25600, 2147483646, 160, 40, 2), APQ_ERR_UNSUPPORTED, "n_fft = 2147483646", "mel n_fft huge");
    expect(apq::check_mel_frames(a, a, a, a, 200, 400, 160, 40, 2), APQ_ERR_UNSUPPORTED, "L = 200", "mel L = n_fft / 2");
    expect(apq::check_mel_frames(a, a, a, a, 25600, 400, 160, 129, 2), APQ_ERR_UNSUPPORTED, "n_mels = 129", "mel n_mels 129");
    expect(apq::check_mel_frames(a, a, a, a, 25600, 400, 401, 40, 2), APQ_ERR_UNSUPPORTED, "hop = 401", "mel hop above n_fft");
    expect(apq::check_mel_frames(odd4, a, a, a, 25600, 400, 160, 40, 2), APQ_ERR_UNSUPPORTED, "x is not", "mel x misaligned");
    expect(apq::check_mel_frames(a, odd8, a, a, 25600, 400, 160, 40, 2), APQ_ERR_UNSUPPORTED, "window is not 8-byte", "mel window misaligned");
    expect(apq::check_mel_frames(a, a, odd4, a, 25600, 400, 160, 40, 2), APQ_ERR_UNSUPPORTED, "basis is not", "mel basis misaligned");
    expect(apq::check_mel_frames(a, a, a, odd4, 25600, 400, 160, 40, 2), APQ_ERR_UNSUPPORTED, "out is not", "mel out misaligned");

    expect(apq::check_speaker_head(a, a, a, a, a, 1), APQ_OK, nullptr, "head B = 1");
    expect(apq::check_speaker_head(a, a, a, a, a, APQ_SPK_MAX_B), APQ_OK, nullptr, "head B = 4096");
    expect(apq::check_speaker_head(a, a, a, a, a, 0), APQ_ERR_INVALID, "B = 0", "head B = 0");
    expect(apq::check_speaker_head(a, a, a, a, a, -2147483647 - 1), APQ_ERR_INVALID, "B = -2147483648", "head B = INT_MIN");
    expect(apq::check_speaker_head(a, a, a, a, a, 4097), APQ_ERR_UNSUPPORTED, "B = 4097", "head B = 4097");
    expect(apq::check_speaker_head(a, a, a, a, a, 2147483647), APQ_ERR_UNSUPPORTED, "B = 2147483647", "head B = INT_MAX");
    expect(apq::check_speaker_head(nullptr, a, a, a, a, 24), APQ_ERR_INVALID, "null h", "head null h");
    expect(apq::check_speaker_head(a, nullptr, a, a, a, 24), APQ_ERR_INVALID, "null w", "head null w");
    expect(apq::check_speaker_head(a, a, nullptr, a, a, 24), APQ_ERR_INVALID, "null b", "head null b");
    expect(apq::check_speaker_head(a, a, a, nullptr, a, 24), APQ_ERR_INVALID, "null partial", "head null partial");
    expect(apq::check_speaker_head(a, a, a, a, nullptr, 24), APQ_ERR_INVALID, "null embed", "head null embed");
    expect(apq::check_speaker_head(odd4, a, a, a, a, 24), APQ_ERR_UNSUPPORTED, "h is not", "head h misaligned");
    expect(apq::check_speaker_head(a, odd4, a, a, a, 24), APQ_ERR_UNSUPPORTED, "w is not", "head w misaligned");
    expect(apq::check_speaker_head(a, a, odd4, a, a, 24), APQ_ERR_UNSUPPORTED, "b is not", "head b misaligned");
    expect(apq::check_speaker_head(a, a, a, odd4, a, 24), APQ_ERR_UNSUPPORTED, "partial is not", "head partial misaligned");
    expect(apq::check_speaker_head(a, a, a, a, odd4, 24), APQ_ERR_UNSUPPORTED, "embed is not", "head embed misaligned");

    printf(failures ? "%d checks failed\n" : "seq_speaker_checks.h: all checks passed\n", failures);
    return failures ? 1 : 0;
}
