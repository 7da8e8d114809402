// OpenCV's integer line / circle drawing rules as per-pixel predicates, the project's one statement of them: the draw2
// rasterisers apd_landmark_map and apd_landmark_vis (libapdata) and ap_lip_line_mask, ap_landmark_discs and ap_circle_rows
// (libapamd, landmark_masks.hip) all test pixels through these functions (host and device: a stand-alone host program runs
// the same functions under sanitizers, tools/raster_host_check.cpp).
//
// OpenCV 4.2 draws cv2.line(thickness) incrementally: ThickLine -> the quad p +- dp through FillConvexPoly at 16.16 fixed
// point (its outline by Line2, its interior by scanlines whose edge positions advance by a rounded slope per row) plus a
// filled Circle at both ends (rule quoted in oracle/cv_raster.py).  Every one of those steps has a closed form in the row /
// column index, so a segment is described once -- four Line2 runs, the two scanline chains as (first row, start, slope)
// pieces, two circle centres -- and any pixel can then be tested against the description with integer arithmetic that gives
// the very pixels the incremental walk would have set.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define APD_HD __host__ __device__ inline
#else
#define APD_HD inline
#endif

namespace apd_raster {

constexpr int SH = 16;
constexpr long long ONE = 1LL << SH, HALF = ONE >> 1;
constexpr int COORD_MAX = 1 << 20;       // rounded coordinates are clamped here: 16.16 products stay far inside int64
constexpr int MAX_RADIUS = 31;

struct CircleRows { int hw[MAX_RADIUS + 1]; };      // hw[|dy|]: half width of the filled circle's row, -1 = no pixel

// the octant walk of OpenCV's Circle(..., fill)
inline CircleRows circle_rows(int r) {
    CircleRows t;
    for (int i = 0; i <= MAX_RADIUS; ++i) t.hw[i] = -1;
    int err = 0, dx = r, dy = 0, plus = 1, minus = (r << 1) - 1;
    while (dx >= dy) {
        if (dx > t.hw[dy]) t.hw[dy] = dx;
        if (dy > t.hw[dx]) t.hw[dx] = dy;
        ++dy;
        err += plus;
        plus += 2;
        if (err > 0) { err -= minus; --dx; minus -= 2; }
    }
    return t;
}

// np.round(v).astype(int): ties to even.  NaN and values beyond +-COORD_MAX land on the clamp.
APD_HD int round_coord(float v) {
    const float r = rintf(v);
    return (int)fminf(fmaxf(r, (float)-COORD_MAX), (float)COORD_MAX);
}

// int(v) of the Python binding (getlipline): truncation toward zero, then the same clamp
APD_HD int trunc_coord(float v) {
    const float r = truncf(v);
    return (int)fminf(fmaxf(r, (float)-COORD_MAX), (float)COORD_MAX);
}

APD_HD bool circle_covers(const CircleRows& rows, int radius, int cx, int cy, int x, int y) {
    const int dy = y > cy ? y - cy : cy - y;
    if (dy > radius) return false;
    const int dx = x > cx ? x - cx : cx - x;
    return dx <= rows.hw[dy];
}

// one Line2 run: pixel (a0 + k, (b0 + k step) >> 16) for k = 0 .. count along the major axis, plus the end pixel
struct Edge {
    long long b0, step;
    int a0, count, ex, ey, xmajor;
};

APD_HD void build_edge(Edge& e, long long x1, long long y1, long long x2, long long y2) {
    long long dx = x2 - x1, dy = y2 - y1;
    const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    if (ax > ay) {
        if (dx < 0) { long long t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; dy = -dy; }
        e.step = (dy * ONE) / (ax | 1);                       // C division: toward zero
        e.count = (int)((x2 - x1) >> SH);
        e.a0 = (int)((x1 + HALF) >> SH);
        e.b0 = y1 + HALF;
        e.xmajor = 1;
    } else {
        if (dy < 0) { long long t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; dx = -dx; }
        e.step = (dx * ONE) / (ay | 1);
        e.count = (int)((y2 - y1) >> SH);
        e.a0 = (int)((y1 + HALF) >> SH);
        e.b0 = x1 + HALF;
        e.xmajor = 0;
    }
    e.ex = (int)((x2 + HALF) >> SH);
    e.ey = (int)((y2 + HALF) >> SH);
}

APD_HD bool edge_covers(const Edge& e, int x, int y) {
    if (x == e.ex && y == e.ey) return true;
    const long long k = (long long)(e.xmajor ? x : y) - e.a0;
    if (k < 0 || k > e.count) return false;
    return ((e.b0 + k * e.step) >> SH) == (e.xmajor ? y : x);
}

// one side of FillConvexPoly's scanline walk: from row yf[j] on, the edge is at xs[j] + (y - yf[j]) dx[j]
struct Chain {
    long long xs[3], dx[3];
    int yf[3], n;
};

struct Fill {
    Chain c[2];
    int y0, y1;                   // rows [y0, y1) are filled; empty when y1 <= y0
};

// the edge bookkeeping of FillConvexPoly for a quad, run once per event (a chain reaching its vertex) instead of once per row
APD_HD void build_fill(Fill& f, const long long (&vx)[4], const long long (&vy)[4], int H, int W) {
    constexpr int NP = 4;
    f.y0 = f.y1 = 0;
    f.c[0].n = f.c[1].n = 0;
    int imin = 0;
    long long ymin = vy[0], ymax = vy[0], xmin = vx[0], xmax = vx[0];
    for (int i = 0; i < NP; ++i) {
        if (vy[i] < ymin) { ymin = vy[i]; imin = i; }
        ymax = vy[i] > ymax ? vy[i] : ymax;
        xmax = vx[i] > xmax ? vx[i] : xmax;
        xmin = vx[i] < xmin ? vx[i] : xmin;
    }
    xmin = (xmin + HALF) >> SH; xmax = (xmax + HALF) >> SH;
    ymin = (ymin + HALF) >> SH; ymax = (ymax + HALF) >> SH;
    if (xmax < 0 || ymax < 0 || xmin >= W || ymin >= H) return;
    if (ymax > H - 1) ymax = H - 1;
    int e_idx[2] = {imin, imin};
    const int e_di[2] = {1, NP - 1};
    long long e_ye[2] = {ymin, ymin};
    int edges = NP;
    long long y = ymin;
    for (;;) {
        for (int i = 0; i < 2; ++i) {
            if (y >= e_ye[i]) {
                int idx0 = e_idx[i];
                int idx = (idx0 + e_di[i]) % NP;
                for (;;) {
                    if (--edges < 0) break;
                    const long long ty = (vy[idx] + HALF) >> SH;
                    if (ty > y) {
                        Chain& c = f.c[i];
                        if (c.n < 3) {
                            c.yf[c.n] = (int)y;
                            c.xs[c.n] = vx[idx0];
                            c.dx[c.n] = ((vx[idx] - vx[idx0]) * 2 + (ty - y)) / (2 * (ty - y));
                            ++c.n;
                        }
                        e_ye[i] = ty;
                        e_idx[i] = idx;
                        break;
                    }
                    idx0 = idx;
                    idx = (idx + e_di[i]) % NP;
                }
            }
        }
        if (edges < 0) break;                                  // row y and everything below stays unfilled
        const long long next = e_ye[0] < e_ye[1] ? e_ye[0] : e_ye[1];
        if (next > ymax) { y = ymax + 1; break; }
        y = next;
    }
    f.y0 = (int)(ymin < 0 ? 0 : ymin);
    f.y1 = (int)y;
    if (f.c[0].n == 0 || f.c[1].n == 0) f.y1 = f.y0;
}

APD_HD long long chain_x(const Chain& c, int y) {
    int j = c.n - 1;
    while (j > 0 && c.yf[j] > y) --j;
    return c.xs[j] + (long long)(y - c.yf[j]) * c.dx[j];
}

APD_HD bool fill_covers(const Fill& f, int x, int y) {
    if (y < f.y0 || y >= f.y1) return false;
    const long long a = chain_x(f.c[0], y), b = chain_x(f.c[1], y);
    const long long l = a > b ? b : a, r = a > b ? a : b;
    return x >= ((l + HALF) >> SH) && x <= ((r + HALF) >> SH);
}

// cv2.line(img, p0, p1, color, thickness) between two integer points
struct Segment {
    Fill fill;
    Edge edge[4];
    int cx0, cy0, cx1, cy1;       // end circles, radius (thickness + 1) >> 1
    int bx0, bx1, by0, by1;       // every pixel of the segment lies in this box (inclusive)
    int quad;                     // 0: the points coincide, only the circles are drawn
};

APD_HD int cap_radius(int thickness) { return (int)((((long long)thickness << (SH - 1)) + HALF) >> SH); }

// rows [row0, row1) are the only ones the caller will test: a segment that misses them gets an empty box and no description
APD_HD void build_segment(Segment& s, int px0, int py0, int px1, int py1, int thickness, int H, int W, int row0, int row1) {
    const long long x0 = px0 * ONE, y0 = py0 * ONE, x1 = px1 * ONE, y1 = py1 * ONE;
    const int rad = cap_radius(thickness);
    s.cx0 = px0; s.cy0 = py0; s.cx1 = px1; s.cy1 = py1;
    s.quad = 0;
    s.fill.y0 = s.fill.y1 = 0;
    int bx0 = (px0 < px1 ? px0 : px1) - rad, bx1 = (px0 > px1 ? px0 : px1) + rad;
    int by0 = (py0 < py1 ? py0 : py1) - rad, by1 = (py0 > py1 ? py0 : py1) + rad;
    const double dx = (double)(x0 - x1) * (1.0 / 65536.0), dy = (double)(y1 - y0) * (1.0 / 65536.0);
    double r = dx * dx + dy * dy;
    long long vx[4], vy[4];
    if (fabs(r) > 2.220446049250313e-16) {
        const long long tf = (long long)thickness << (SH - 1);
        r = ((double)tf + (thickness & 1) * 65536.0 * 0.5) / sqrt(r);
        const long long dpx = (long long)rint(dy * r), dpy = (long long)rint(dx * r);       // cvRound
        vx[0] = x0 + dpx; vx[1] = x0 - dpx; vx[2] = x1 - dpx; vx[3] = x1 + dpx;
        vy[0] = y0 + dpy; vy[1] = y0 - dpy; vy[2] = y1 - dpy; vy[3] = y1 + dpy;
        s.quad = 1;
        for (int i = 0; i < 4; ++i) {                       // + 2: the rounded slopes drift by far less than a pixel in an image
            const int qx = (int)((vx[i] + HALF) >> SH), qy = (int)((vy[i] + HALF) >> SH);
            bx0 = qx - 2 < bx0 ? qx - 2 : bx0; bx1 = qx + 2 > bx1 ? qx + 2 : bx1;
            by0 = qy - 2 < by0 ? qy - 2 : by0; by1 = qy + 2 > by1 ? qy + 2 : by1;
        }
    }
    if (bx1 < 0 || bx0 >= W || by1 < row0 || by0 >= row1) {
        s.bx0 = s.by0 = 1; s.bx1 = s.by1 = 0; s.quad = 0;
        return;
    }
    s.bx0 = bx0; s.bx1 = bx1; s.by0 = by0; s.by1 = by1;
    if (s.quad) {
        for (int i = 0; i < 4; ++i) build_edge(s.edge[i], vx[(i + 3) & 3], vy[(i + 3) & 3], vx[i], vy[i]);
        build_fill(s.fill, vx, vy, H, W);
    }
}

APD_HD bool segment_covers(const Segment& s, const CircleRows& cap, int rad, int x, int y) {
    if (x < s.bx0 || x > s.bx1 || y < s.by0 || y > s.by1) return false;
    if (circle_covers(cap, rad, s.cx0, s.cy0, x, y) || circle_covers(cap, rad, s.cx1, s.cy1, x, y)) return true;
    if (!s.quad) return false;
    for (int i = 0; i < 4; ++i)
        if (edge_covers(s.edge[i], x, y)) return true;
    return fill_covers(s.fill, x, y);
}

}  // namespace apd_raster
