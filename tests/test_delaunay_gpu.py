"""GPU (-m gpu): ap_delaunay, the device triangulation behind cal_motion256(triangulate='device').

Expected values: ``scipy.spatial.Delaunay`` for point sets in general position, and ``contract_delaunay`` below -- a numpy
restatement of the contract in include/animateportrait_amd.h (brute force over triples, fp64, the dedupe rule and the fan
rule) -- for degenerate ones, where scipy's choice among cocircular points is its own.  Both are compared exactly: the
contract makes the result unique, rows in lexicographic order.  ap_delaunay is called through the C ABI into buffers with a
sentinel page on both sides, which must come back untouched."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from conftest import linf

pytestmark = pytest.mark.gpu

PAGE_INTS = 4096 // 4
SENTINEL = 0x7FC0BEEF                                   # a NaN pattern as int32

# the reference's 8 border points (data/motion.py: EDGES), 4 of them duplicates
EDGES32 = np.array([[0, 0], [255, 255], [0, 255], [255, 0], [0, 255], [255, 0], [255, 255], [255, 255]], dtype=np.float32)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch.device('cuda:0')


# ---------------------------------------------------------------- expected values

def _orient(px, py, qx, qy, rx, ry):
    return (qx - px) * (ry - py) - (qy - py) * (rx - px)


def contract_delaunay(pts):
    """The contract, restated: (T, 3) int32 rows a < b < c in lexicographic order."""
    p32 = np.ascontiguousarray(pts, dtype=np.float32)
    bits = p32.view(np.uint32)
    live = [i for i in range(len(p32)) if not any((bits[j] == bits[i]).all() for j in range(i))]   # bit-equal to an earlier point: dead
    idx = np.array(live, dtype=np.int64)
    nl = len(idx)
    if nl < 3:
        return np.zeros((0, 3), np.int32)
    x, y = p32[idx, 0].astype(np.float64), p32[idx, 1].astype(np.float64)
    triples = np.array(list(itertools.combinations(range(nl), 3)), dtype=np.int64)                # lexicographic
    d = np.arange(nl)[None, :]
    keep = []
    for part in np.array_split(triples, max(1, len(triples) * nl // 1_000_000)):
        a, b, c = part[:, 0:1], part[:, 1:2], part[:, 2:3]
        o = _orient(x[a], y[a], x[b], y[b], x[c], y[c])
        ob = _orient(x[b], y[b], x[c], y[c], x[a], y[a])
        ax, ay, bx, by, cx, cy = x[a] - x[d], y[a] - y[d], x[b] - x[d], y[b] - y[d], x[c] - x[d], y[c] - y[d]
        al, bl, cl = ax * ax + ay * ay, bx * bx + by * by, cx * cx + cy * cy
        det = ax * (by * cl - bl * cy) - ay * (bx * cl - bl * cx) + al * (bx * cy - by * cx)      # in-circle, relative to d
        s = np.where(o > 0, det, -det)
        other = (d != a) & (d != b) & (d != c)
        inside, on = other & (s > 0), other & (s == 0)
        od = _orient(x[b], y[b], x[c], y[c], x[d], y[d])
        a_side = ((ob > 0) & (od > 0)) | ((ob < 0) & (od < 0))
        ok = (o != 0)[:, 0] & ~inside.any(1) & ~(on & (d < a)).any(1) & ~(on & ~a_side).any(1)    # (i) (ii) (iii) (iv)
        keep.append(part[ok])
    return idx[np.concatenate(keep)].astype(np.int32).reshape(-1, 3)


def scipy_delaunay(pts):
    """scipy's triangles in the contract's form: lowest duplicate, ascending vertices, rows sorted."""
    from scipy.spatial import Delaunay
    p32 = np.ascontiguousarray(pts, dtype=np.float32)
    bits = p32.view(np.uint32)
    first = np.array([min(j for j in range(i + 1) if (bits[j] == bits[i]).all()) for i in range(len(p32))])
    t = np.sort(first[Delaunay(p32.astype(np.float64)).simplices], axis=1)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))].astype(np.int32)


def face_like(seed):
    """68 points uniform(20, 235) as float32 + the 8 border points: general position apart from the duplicates"""
    return np.concatenate([np.random.default_rng(seed).uniform(20, 235, (68, 2)).astype(np.float32), EDGES32])


# ---------------------------------------------------------------- the call, inside sentinel pages

def delaunay(pts, tcap, dev):
    """pts (N, P, 2) -> (rc, tri (N, tcap, 3), count (N,)) on the CPU; asserts the pages around tri and count."""
    from animateportrait_amd import _capi as C
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    n, p = pts.shape[:2]
    ntri = n * tcap * 3
    buf = torch.full((PAGE_INTS + ntri + PAGE_INTS + n + PAGE_INTS,), SENTINEL, dtype=torch.int32, device=dev)
    tri, count = buf[PAGE_INTS:PAGE_INTS + ntri], buf[2 * PAGE_INTS + ntri:2 * PAGE_INTS + ntri + n]
    pd = torch.from_numpy(pts).to(dev)
    rc = C.lib().ap_delaunay(ctypes.c_void_p(pd.data_ptr()), n, p, tcap, ctypes.c_void_p(tri.data_ptr()),
                             ctypes.c_void_p(count.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    host = buf.cpu()
    guard = torch.cat([host[:PAGE_INTS], host[PAGE_INTS + ntri:2 * PAGE_INTS + ntri], host[2 * PAGE_INTS + ntri + n:]])
    assert bool((guard == SENTINEL).all()), 'ap_delaunay wrote outside tri / count'
    return rc, host[PAGE_INTS:PAGE_INTS + ntri].view(n, tcap, 3).numpy(), host[2 * PAGE_INTS + ntri:2 * PAGE_INTS + ntri + n].numpy()


def assert_sets(pts, expected, tcap, dev):
    rc, tri, count = delaunay(pts, tcap, dev)
    assert rc == 0
    for i, exp in enumerate(expected):
        assert count[i] == len(exp), (i, count[i], len(exp))
        assert np.array_equal(tri[i, :len(exp)], exp), i
        assert (tri[i, len(exp):] == -1).all(), i
    return tri, count


# ---------------------------------------------------------------- 1. general position

def test_general_position_equals_scipy(dev):
    pts = np.stack([face_like(s) for s in (1, 2, 3)])
    exp = [scipy_delaunay(p) for p in pts]
    assert all(len(e) == 138 for e in exp)                       # 72 live points, 4 on the hull: 2 * 72 - 2 - 4
    tri, _ = assert_sets(pts, exp, 152, dev)
    again = delaunay(pts, 152, dev)[1]
    assert np.array_equal(tri, again)                            # same input, same bits


# ---------------------------------------------------------------- 2. degenerate inputs

SMALL = {
    'one triangle': ([[0, 0], [0, 1], [1, 0]], 1),
    'collinear': ([[0, 0], [1, 1], [2, 2]], 0),
    'unit square': ([[0, 0], [0, 1], [1, 1], [1, 0]], 2),
    'square and centre': ([[0, 0], [0, 2], [2, 2], [2, 0], [1, 1]], 4),
    'all identical': ([[3, 3]] * 5, 0),
}


@pytest.mark.parametrize('name', list(SMALL))
def test_small_sets_equal_the_contract(dev, name):
    pts, ntri = SMALL[name]
    pts = np.array(pts, dtype=np.float32)
    exp = contract_delaunay(pts)
    assert len(exp) == ntri
    tri, _ = assert_sets(pts[None], [exp], 2 * len(pts), dev)
    if name == 'unit square':
        assert (tri[0, :2, 0] == 0).all()                        # fanned from vertex 0


def hull_area2(p):
    """twice the area of the convex hull of integer points (monotone chain), exact in int64"""
    q = sorted(set(map(tuple, p.tolist())))
    if len(q) < 3:
        return 0

    def half(seq):
        h = []
        for r in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (r[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (r[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(r)
        return h
    h = half(q)[:-1] + half(q[::-1])[:-1]
    return abs(sum(h[i][0] * h[(i + 1) % len(h)][1] - h[(i + 1) % len(h)][0] * h[i][1] for i in range(len(h))))


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_integer_points_tile_their_hull(dev, seed):
    """30 points of [0, 12)^2: duplicates, collinear runs, cocircular quadruples"""
    p = np.random.default_rng(seed).integers(0, 12, (30, 2))
    exp = contract_delaunay(p)
    tri, count = assert_sets(p.astype(np.float32)[None], [exp], 60, dev)
    t = tri[0, :count[0]].astype(np.int64)
    q = p.astype(np.int64)
    a, b, c = q[t[:, 0]], q[t[:, 1]], q[t[:, 2]]
    o = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    assert (o != 0).all()
    assert int(np.abs(o).sum()) == hull_area2(q)                 # a tiling of the hull: no overlap, no gap
    ad, bd, cd = (v[:, None, :] - q[None, :, :] for v in (a, b, c))                    # (T, P, 2) relative to each point
    al, bl, cl = ((v ** 2).sum(-1) for v in (ad, bd, cd))
    det = (ad[..., 0] * (bd[..., 1] * cl - bl * cd[..., 1]) - ad[..., 1] * (bd[..., 0] * cl - bl * cd[..., 0])
           + al * (bd[..., 0] * cd[..., 1] - bd[..., 1] * cd[..., 0]))
    assert (det * np.sign(o)[:, None] <= 0).all()                # every open circumdisc is empty


def test_largest_point_count(dev):
    p = np.random.default_rng(5).uniform(0, 255, (128, 2)).astype(np.float32)
    exp = contract_delaunay(p)
    assert np.array_equal(exp, scipy_delaunay(p))
    assert_sets(p[None], [exp], 256, dev)


def test_sets_of_different_live_counts_in_one_call(dev):
    a = face_like(11)
    b = a.copy()
    b[40:] = b[7]                                                # 41 live points
    assert_sets(np.stack([a, b]), [contract_delaunay(a), contract_delaunay(b)], 152, dev)


# ---------------------------------------------------------------- 3. capacity

def test_one_row_too_few(dev):
    p = face_like(4)
    nt = len(scipy_delaunay(p))
    rc, tri, count = delaunay(p[None], nt - 1, dev)
    assert rc == 0 and count[0] == -1 and (tri == -1).all()
    rc, tri, count = delaunay(p[None], nt, dev)                  # exactly enough
    assert rc == 0 and count[0] == nt and (tri >= 0).all()


# ---------------------------------------------------------------- 4. refusals

@pytest.mark.parametrize('n, p, tcap', [(1, 2, 8), (1, 129, 300), (0, 76, 152), (1, 76, 60 * 1024 // 48 + 1)])
def test_refusals_launch_nothing(dev, n, p, tcap):
    from animateportrait_amd import _capi as C
    lib = C.lib()
    assert lib.ap_delaunay_ok(n, p, tcap) == 0
    buf = torch.full((1 << 16,), SENTINEL, dtype=torch.int32, device=dev)
    pts = torch.zeros((max(n, 1) * p * 2,), dtype=torch.float32, device=dev)
    rc = lib.ap_delaunay(ctypes.c_void_p(pts.data_ptr()), n, p, tcap, ctypes.c_void_p(buf.data_ptr()),
                         ctypes.c_void_p(buf[1 << 15:].data_ptr()), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert rc < 0 and bool((buf == SENTINEL).all())
    assert lib.ap_delaunay_ok(1, 76, 152) == 1
    assert lib.ap_delaunay(None, 1, 76, 152, ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(buf[1 << 15:].data_ptr()), None) < 0


# ---------------------------------------------------------------- 5. the motion grid through the new path

def test_motion_grid_with_device_triangulation(dev, golden):
    from animateportrait_amd.data.motion import cal_motion256, check_triangulations
    gd = golden('motion.npz')
    lm0 = np.stack([gd['lm0_%d' % i].numpy() for i in range(2)])
    lm = np.stack([gd['lm_%d' % i].numpy() for i in range(2)])
    got = cal_motion256(lm0, lm, device=dev, triangulate='device')
    assert got.shape == (2, 256, 256, 2) and got.is_cuda
    for i in range(2):
        assert linf(got[i], gd['motion_%d' % i]) < 2e-5          # the bound of test_motion_grid_rasteriser
    rng = np.random.default_rng(6)
    a0 = rng.uniform(20, 235, (16, 68, 2)).astype(np.float32)
    a1 = rng.uniform(20, 235, (16, 68, 2)).astype(np.float32)
    host = cal_motion256(a0, a1, device=dev)
    device = cal_motion256(a0, a1, device=dev, triangulate='device')
    assert linf(device, host) < 2e-5                             # same triangles in another order: ties on shared edges
    ident = cal_motion256(lm[0], lm[0], device=dev, triangulate='device')
    ax = torch.arange(256., device=dev) / 127.5 - 1
    assert linf(ident[0, :, :, 0], ax.view(1, 256).expand(256, 256)) < 1e-5
    assert linf(ident[0, :, :, 1], ax.view(256, 1).expand(256, 256)) < 1e-5
    on_dev = cal_motion256(torch.from_numpy(a0).to(dev), torch.from_numpy(a1).to(dev), device=dev, triangulate='device')
    assert torch.equal(on_dev, device)
    check_triangulations(dev)                                    # nothing overflowed


# ---------------------------------------------------------------- 6. no host round trip

def test_device_path_is_capturable(dev):
    """cal_motion256(triangulate='device') on static device landmarks, captured in a graph on one stream and replayed on
    another frame's landmarks: a copy to the host, a synchronisation or an upload inside the call would fail the capture."""
    from animateportrait_amd.data.motion import cal_motion256, check_triangulations
    rng = np.random.default_rng(8)
    frames = torch.from_numpy(rng.uniform(20, 235, (3, 4, 68, 2)).astype(np.float32)).to(dev)     # [frame][batch]
    s0, s1 = frames[0, :].clone(), frames[1, :].clone()          # the static inputs
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        cal_motion256(s0, s1, device=dev, triangulate='device')  # warm-up: the flag and the border points exist from here on
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = cal_motion256(s0, s1, device=dev, triangulate='device')
    s1.copy_(frames[2])
    graph.replay()
    torch.cuda.synchronize()
    eager = cal_motion256(frames[0], frames[2], device=dev, triangulate='device')
    assert torch.equal(out, eager)
    check_triangulations(dev)


# ---------------------------------------------------------------- 7. the sticky flag

def test_overflow_is_remembered_once(dev):
    from animateportrait_amd.data.motion import triangulate_device, check_triangulations
    check_triangulations(dev)
    pts = torch.from_numpy(np.stack([face_like(1), face_like(2)])).to(dev)
    tri, count = triangulate_device(pts)
    assert tri.shape == (2, 152, 3) and count.tolist() == [138, 138]
    check_triangulations(dev)
    tri, count = triangulate_device(pts, tcap=100)
    triangulate_device(pts)                                      # a good call afterwards does not clear it
    assert count.tolist() == [-1, -1] and bool((tri == -1).all())
    with pytest.raises(RuntimeError, match='more triangles'):
        check_triangulations(dev)
    check_triangulations(dev)                                    # read and cleared
