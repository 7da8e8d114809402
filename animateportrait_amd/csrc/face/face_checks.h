// Host side of libapface.so that needs no device: the error buffer, the argument checks behind every *_ok predicate, the
// nets' layer tables and the workspace sizes.  Plain C++.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include "../../../include/animateportrait_face.h"

namespace apf {

inline char* err_buf() {
    static thread_local char buf[256] = "";
    return buf;
}

inline int fail(int code, const char* fmt, long a = 0, long b = 0, long c = 0, long d = 0) {
    snprintf(err_buf(), 256, fmt, a, b, c, d);
    return code;
}

inline bool side_ok(int v) { return v >= 1 && v <= APF_MAX_SIDE; }

inline int check_image(const char* what, const void* img, int H, int W) {
    if (!img) return snprintf(err_buf(), 256, "%s: null image", what), APF_ERR_INVALID;
    if (!side_ok(H) || !side_ok(W)) return snprintf(err_buf(), 256, "%s: image %d x %d, served: 1..%d per axis", what, H, W, APF_MAX_SIDE), APF_ERR_UNSUPPORTED;
    return APF_OK;
}

inline int check_resize_level(const void* img, int H, int W, int oh, int ow, const void* out) {
    const int rc = check_image("resize_level", img, H, W);
    if (rc != APF_OK) return rc;
    if (!out) return fail(APF_ERR_INVALID, "resize_level: null out");
    if (!side_ok(oh) || !side_ok(ow)) return fail(APF_ERR_UNSUPPORTED, "resize_level: level %ld x %ld, served: 1..%ld per axis", oh, ow, APF_MAX_SIDE);
    return APF_OK;
}

// P-Net's map for a level of h x w
inline int pnet_map(int s) { return (s - 2 + 1) / 2 - 4; }

inline int check_pnet(const void* level, int h, int w, const void* params, const void* cand_count) {
    if (!level || !params || !cand_count) return fail(APF_ERR_INVALID, "pnet: null level / params / cand_count");
    if (h < APF_MIN_LEVEL || w < APF_MIN_LEVEL || h > APF_MAX_SIDE || w > APF_MAX_SIDE)
        return fail(APF_ERR_UNSUPPORTED, "pnet: level %ld x %ld, served: %ld..%ld per axis", h, w, APF_MIN_LEVEL, APF_MAX_SIDE);
    return APF_OK;
}

inline int check_stage1_level(const void* cand_idx, const void* cand_count, int mw, double scale, const void* cand_boxes,
                              const void* merged, const void* merged_count) {
    if (!cand_idx || !cand_count || !cand_boxes || !merged || !merged_count) return fail(APF_ERR_INVALID, "stage1_level: null pointer");
    if (mw < 1 || mw > APF_MAX_SIDE) return fail(APF_ERR_INVALID, "stage1_level: map width %ld", mw);
    if (!(scale > 0.0)) return fail(APF_ERR_INVALID, "stage1_level: scale is not positive");
    return APF_OK;
}

inline int64_t box_stage_ws_bytes(int cap_in) {
    if (cap_in < 1 || cap_in > APF_CAP_SORT) return -1;
    // filtered boxes (5 doubles), offsets (4 doubles), landmarks (10 floats), source index (int32, padded to 8 bytes)
    return (int64_t)cap_in * (5 * 8 + 4 * 8 + 10 * 4 + 8);
}

inline int check_box_stage(const void* in, int in_stride, const void* n_in, int cap_in, int mode, int late, const void* landmarks,
                           const void* out, const void* n_out, int cap_out, const void* ws) {
    if (!in || !n_in || !out || !n_out || !ws) return fail(APF_ERR_INVALID, "box_stage: null pointer");
    if (in_stride != 5 && in_stride != 9) return fail(APF_ERR_INVALID, "box_stage: row stride %ld (5: boxes, 9: boxes and offsets)", in_stride);
    if (cap_in < 1 || cap_in > APF_CAP_SORT) return fail(APF_ERR_UNSUPPORTED, "box_stage: cap_in = %ld, served: 1..%ld", cap_in, APF_CAP_SORT);
    if (cap_out < 1 || cap_out > APF_CAP_SORT) return fail(APF_ERR_UNSUPPORTED, "box_stage: cap_out = %ld, served: 1..%ld", cap_out, APF_CAP_SORT);
    if (mode != APF_NMS_UNION && mode != APF_NMS_MIN) return fail(APF_ERR_INVALID, "box_stage: NMS mode %ld", mode);
    if (late != 0 && late != 1) return fail(APF_ERR_INVALID, "box_stage: late = %ld", late);
    if (late && !landmarks) return fail(APF_ERR_INVALID, "box_stage: the last stage needs landmarks");
    return APF_OK;
}

inline int check_cutouts(const void* img, int H, int W, const void* boxes, const void* count, int cap, int size, const void* out) {
    const int rc = check_image("cutouts", img, H, W);
    if (rc != APF_OK) return rc;
    if (!boxes || !count || !out) return fail(APF_ERR_INVALID, "cutouts: null boxes / count / out");
    if (size != 24 && size != 48) return fail(APF_ERR_UNSUPPORTED, "cutouts: size %ld, served: 24 (R-Net) and 48 (O-Net)", size);
    if (cap < 1 || cap > APF_CAP_SORT) return fail(APF_ERR_UNSUPPORTED, "cutouts: cap = %ld, served: 1..%ld", cap, APF_CAP_SORT);
    return APF_OK;
}

// one layer of R-Net / O-Net's feature stack: a valid convolution with PReLU, or a ceil-mode max-pool of stride 2
struct Layer {
    int pool, k, cin, cout, in_side, out_side;
};

struct NetPlan {
    int side, n_layers, fc_in, fc_out, n_lm;
    Layer layers[7];
    long a_elems, b_elems;        // per-box floats of the two ping-pong buffers
};

inline int pool_out(int in, int k) {
    int o = (in - k + 1) / 2 + 1;
    if ((o - 1) * 2 >= in) --o;
    return o;
}

inline NetPlan net_plan(int net) {
    NetPlan p = {};
    const int rspec[][3] = {{0, 3, 28}, {1, 3, 0}, {0, 3, 48}, {1, 3, 0}, {0, 2, 64}};
    const int ospec[][3] = {{0, 3, 32}, {1, 3, 0}, {0, 3, 64}, {1, 3, 0}, {0, 3, 64}, {1, 2, 0}, {0, 2, 128}};
    const int (*spec)[3] = net == APF_NET_R ? rspec : ospec;
    p.n_layers = net == APF_NET_R ? 5 : 7;
    p.side = net == APF_NET_R ? 24 : 48;
    p.fc_out = net == APF_NET_R ? 128 : 256;
    p.n_lm = net == APF_NET_R ? 0 : 10;
    int side = p.side, c = 3;
    for (int i = 0; i < p.n_layers; ++i) {
        Layer& l = p.layers[i];
        l.pool = spec[i][0];
        l.k = spec[i][1];
        l.cin = c;
        l.cout = l.pool ? c : spec[i][2];
        l.in_side = side;
        l.out_side = l.pool ? pool_out(side, l.k) : side - l.k + 1;
        side = l.out_side;
        c = l.cout;
        const long elems = (long)c * side * side;
        long& buf = (i % 2 == 0) ? p.a_elems : p.b_elems;
        if (elems > buf) buf = elems;
    }
    p.fc_in = c * side * side;
    if (p.fc_out > p.b_elems) p.b_elems = p.fc_out;       // n_layers is odd: the stack ends in A, the hidden layer goes to B
    return p;
}

inline int64_t net_ws_bytes(int net, int cap) {
    if ((net != APF_NET_R && net != APF_NET_O) || cap < 1 || cap > APF_CAP_SORT) return -1;
    const NetPlan p = net_plan(net);
    return (int64_t)cap * (p.a_elems + p.b_elems) * 4;
}

inline int check_net(int net, const void* cuts, const void* count, int cap, const void* params, const void* ws, const void* probs,
                     const void* offsets, const void* landmarks) {
    if (net != APF_NET_R && net != APF_NET_O) return fail(APF_ERR_INVALID, "net: %ld is neither APF_NET_R nor APF_NET_O", net);
    if (!cuts || !count || !params || !ws || !probs || !offsets) return fail(APF_ERR_INVALID, "net: null pointer");
    if ((net == APF_NET_O) != (landmarks != nullptr)) return fail(APF_ERR_INVALID, "net: landmarks belong to O-Net, and only to it");
    if (cap < 1 || cap > APF_CAP_SORT) return fail(APF_ERR_UNSUPPORTED, "net: cap = %ld, served: 1..%ld", cap, APF_CAP_SORT);
    return APF_OK;
}

inline int check_crop_resize_cubic(const void* img, int H, int W, int x0, int y0, int size, int out_size, const void* out) {
    const int rc = check_image("crop_resize_cubic", img, H, W);
    if (rc != APF_OK) return rc;
    if (!out) return fail(APF_ERR_INVALID, "crop_resize_cubic: null out");
    if (!side_ok(size) || !side_ok(out_size)) return fail(APF_ERR_UNSUPPORTED, "crop_resize_cubic: cut %ld -> %ld, served: 1..%ld", size, out_size, APF_MAX_SIDE);
    const long lim = 4L * APF_MAX_SIDE;
    if (x0 < -lim || x0 > lim || y0 < -lim || y0 > lim) return fail(APF_ERR_INVALID, "crop_resize_cubic: corner (%ld, %ld) is out of range", x0, y0);
    return APF_OK;
}

// ---- FAN: box -> centre and scale -> the inverse transform's coefficients (the header states the order; nothing is fused:
// the face library is built with -ffp-contract=off, on the host as on the device)
struct FanFrame {
    double i00, i02x, i02y;        // X = i00 * px + i02x,  Y = i00 * py + i02y
};

inline bool fan_box_ok(double x0, double y0, double x1, double y1) {
    const double lim = 4.0 * APF_MAX_SIDE;
    // (sides from 1e-6 px: below that the transform's coefficients leave the range in which they are finite)
    return x1 - x0 >= 1e-6 && y1 - y0 >= 1e-6 && x0 >= -lim && y0 >= -lim && x1 <= lim && y1 <= lim;      // (false for a NaN)
}

inline FanFrame fan_frame(double x0, double y0, double x1, double y1, int S) {
    const double cx = x1 - (x1 - x0) / 2.0;
    const double cy = y1 - (y1 - y0) / 2.0 - (y1 - y0) * 0.12;
    const double scale = (x1 - x0 + y1 - y0) / 195.0;
    const double h = 200.0 * scale;
    const double a = (double)S / h;
    const double bx = (double)S * (0.5 - cx / h), by = (double)S * (0.5 - cy / h);
    return FanFrame{1.0 / a, -bx / a, -by / a};
}

struct FanWindow {
    int ulx, uly, w, h;
};

inline FanWindow fan_window(double x0, double y0, double x1, double y1, int R) {
    const FanFrame f = fan_frame(x0, y0, x1, y1, R);
    const int ulx = (int)(f.i00 * 1.0 + f.i02x), uly = (int)(f.i00 * 1.0 + f.i02y);
    const int brx = (int)(f.i00 * (double)R + f.i02x), bry = (int)(f.i00 * (double)R + f.i02y);
    return FanWindow{ulx, uly, brx - ulx, bry - uly};
}

inline int check_fan_crop(const void* img, int H, int W, double x0, double y0, double x1, double y1, int R, int flip, int order,
                          const void* out) {
    const int rc = check_image("fan_crop", img, H, W);
    if (rc != APF_OK) return rc;
    if (!out) return fail(APF_ERR_INVALID, "fan_crop: null out");
    if (R < 1 || R > APF_FAN_MAX_RES) return fail(APF_ERR_UNSUPPORTED, "fan_crop: R = %ld, served: 1..%ld", R, APF_FAN_MAX_RES);
    if (flip != 0 && flip != 1) return fail(APF_ERR_INVALID, "fan_crop: flip = %ld", flip);
    if (order != APF_FAN_RGB && order != APF_FAN_BGR) return fail(APF_ERR_INVALID, "fan_crop: channel order %ld", order);
    if (!fan_box_ok(x0, y0, x1, y1)) return fail(APF_ERR_INVALID, "fan_crop: the box has no positive size inside +-%ld", 4L * APF_MAX_SIDE);
    const FanWindow win = fan_window(x0, y0, x1, y1, R);
    if (win.w < 1 || win.h < 1 || win.w > 4 * APF_MAX_SIDE || win.h > 4 * APF_MAX_SIDE)
        return fail(APF_ERR_UNSUPPORTED, "fan_crop: window %ld x %ld, served: 1..%ld per axis", win.h, win.w, 4L * APF_MAX_SIDE);
    return APF_OK;
}

inline int check_fan_decode(const void* hm, int B, int Hm, const double* boxes, const void* out) {
    if (!hm || !boxes || !out) return fail(APF_ERR_INVALID, "fan_decode: null hm / boxes / out");
    if (B < 1) return fail(APF_ERR_INVALID, "fan_decode: B = %ld", B);
    if (Hm < 1) return fail(APF_ERR_INVALID, "fan_decode: Hm = %ld", Hm);
    if (B > APF_FAN_MAX_B) return fail(APF_ERR_UNSUPPORTED, "fan_decode: B = %ld, served: 1..%ld", B, APF_FAN_MAX_B);
    if (Hm > APF_FAN_MAX_RES) return fail(APF_ERR_UNSUPPORTED, "fan_decode: Hm = %ld, served: 1..%ld", Hm, APF_FAN_MAX_RES);
    for (int b = 0; b < B; ++b)
        if (!fan_box_ok(boxes[4 * b], boxes[4 * b + 1], boxes[4 * b + 2], boxes[4 * b + 3]))
            return fail(APF_ERR_INVALID, "fan_decode: box %ld has no positive size inside +-%ld", b, 4L * APF_MAX_SIDE);
    return APF_OK;
}

}  // namespace apf
