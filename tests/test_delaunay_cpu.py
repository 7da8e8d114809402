"""CPU (-m "not gpu"): the region ap_delaunay serves, as its predicate states it, and the defaults of the entry points that
can triangulate on the device -- 'host' everywhere: the device triangulation is opt-in."""
import inspect

import pytest

TCAP_MAX = 60 * 1024 // (12 * 4)        # rows of ap_motion_grid's LDS table


@pytest.mark.parametrize('n, p, tcap, served', [
    (1, 3, 1, True), (65535, 128, TCAP_MAX, True), (1, 128, 1, True), (65535, 3, TCAP_MAX, True), (16, 76, 152, True),
    (0, 76, 152, False), (65536, 76, 152, False), (-1, 76, 152, False),
    (1, 2, 152, False), (1, 129, 152, False), (1, 0, 152, False),
    (1, 76, 0, False), (1, 76, TCAP_MAX + 1, False), (1, 76, -5, False), (1, 76, 2 ** 31 - 1, False),
])
def test_served_region_corners(n, p, tcap, served):
    from animateportrait_amd import _capi as C
    assert C.lib().ap_delaunay_ok(n, p, tcap) == int(served)


def test_abi_version_and_export_count():
    from animateportrait_amd import _capi as C
    assert C.ABI_VERSION == 17 and C.lib().ap_abi_version() == 17
    assert len(C.SIGNATURES) == 96 and 'ap_delaunay' in C.SIGNATURES and 'ap_delaunay_ok' in C.SIGNATURES


def test_refused_calls_return_an_error_without_a_device():
    """null pointers and sizes outside the region are turned away before anything touches the device"""
    import ctypes
    from animateportrait_amd import _capi as C
    lib = C.lib()
    assert lib.ap_delaunay(None, 1, 76, 152, None, None, None) < 0
    buf = (ctypes.c_int32 * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for n, p, tcap in ((1, 2, 8), (1, 129, 300), (0, 76, 152), (1, 76, TCAP_MAX + 1)):
        assert lib.ap_delaunay(ptr, n, p, tcap, ptr, ptr, None) < 0
        assert lib.ap_last_error()
    assert list(buf) == [0] * 8


def test_unknown_triangulation_is_refused():
    import numpy as np
    from animateportrait_amd.data.motion import cal_motion256
    from animateportrait_amd.stream import ClipStreamer
    lm = np.zeros((68, 2), np.float32)
    with pytest.raises(ValueError):
        cal_motion256(lm, lm, triangulate='bogus')
    with pytest.raises(ValueError):
        ClipStreamer(None, triangulate='bogus')


def test_host_triangulation_stays_the_default():
    from animateportrait_amd import end2end
    from animateportrait_amd.data.motion import cal_motion256
    from animateportrait_amd.stream import ClipStreamer
    assert inspect.signature(cal_motion256).parameters['triangulate'].default == 'host'
    assert inspect.signature(ClipStreamer.__init__).parameters['triangulate'].default == 'host'
    parser = end2end.make_parser()
    assert parser.get_default('triangulate') == 'host'
    assert parser.parse_known_args(['--photo', 'p', '--out', 'o', '--triangulate', 'device'])[0].triangulate == 'device'
