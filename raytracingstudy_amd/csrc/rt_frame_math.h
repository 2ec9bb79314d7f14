// rt_frame_math.h — the host arithmetic a frame's images depend on bit for
// bit, free of HIP and of the renderer's state: plain arrays in and out, f64
// operations in a fixed order (built with -ffp-contract=off like the rest).
// rt_frame.cpp calls it per frame; tests/native/frame_math_dump.cpp prints it
// for tests/test_frame_math.py, on the CPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace rtamd {

// The image-plane screen's basis (SceneArgs::prim_cam8, DESIGN.md 5.1 round
// 6): rows x, y, z, orthonormal in f64 and rounded to f32, z along the ray
// through the image centre (getRay's K and R, include/camera.h:24-41).
// Returns 1 when every primary ray of the W x H frame keeps (B d).z >= 0.1
// |B d| (checked at the image corners: the rays' directions are the cone
// they span, and the ratio is kept under positive combinations), else 0:
// the records then pass every sphere.
inline uint32_t cam8_basis(const float K[9], const float R[9], uint32_t W, uint32_t H, float B[9]) {
    auto ray = [&](double u, double v, double w[3]) {
        const double dx = (u - K[2]) / K[0], dy = (v - K[5]) / K[4];
        for (int i = 0; i < 3; ++i) w[i] = R[i] * dx + R[3 + i] * dy + R[6 + i];
    };
    double z[3], x[3] = {R[0], R[1], R[2]}, y[3];
    ray(0.5 * W, 0.5 * H, z);
    const double zn = sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2]);
    if (!(zn > 0.0) || !std::isfinite(zn)) {
        for (int i = 0; i < 9; ++i) B[i] = i % 4 == 0 ? 1.0f : 0.0f;
        return 0u;
    }
    for (double& t : z) t /= zn;
    const double xz = x[0] * z[0] + x[1] * z[1] + x[2] * z[2];
    for (int i = 0; i < 3; ++i) x[i] -= xz * z[i];
    double xn = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    if (!(xn > 1e-3)) {  // R's first column along the view: any perpendicular
        x[0] = fabs(z[0]) < 0.9 ? 1.0 : 0.0;
        x[1] = fabs(z[0]) < 0.9 ? 0.0 : 1.0;
        x[2] = 0.0;
        const double t = x[0] * z[0] + x[1] * z[1];
        for (int i = 0; i < 3; ++i) x[i] -= t * z[i];
        xn = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    }
    for (double& t : x) t /= xn;
    y[0] = z[1] * x[2] - z[2] * x[1];
    y[1] = z[2] * x[0] - z[0] * x[2];
    y[2] = z[0] * x[1] - z[1] * x[0];
    for (int i = 0; i < 3; ++i) {
        B[i] = static_cast<float>(x[i]);
        B[3 + i] = static_cast<float>(y[i]);
        B[6 + i] = static_cast<float>(z[i]);
    }
    uint32_t ok = 1u;
    for (int k = 0; k < 4; ++k) {
        double w[3], p[3];
        ray((k & 1) ? W : 0.0, (k & 2) ? H : 0.0, w);
        for (int i = 0; i < 3; ++i)
            p[i] = (double)B[3 * i] * w[0] + (double)B[3 * i + 1] * w[1] + (double)B[3 * i + 2] * w[2];
        const double pn = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        if (!(p[2] >= 0.1 * pn) || !std::isfinite(pn)) ok = 0u;
    }
    return ok;
}

// The light-plane screen's basis (FrameArgs::shd_e): an
// orthonormal {e1, e2} of the plane perpendicular to the shadow direction L,
// in f64 from the f32 L the kernel uses, then rounded.
inline void light_plane_basis(const float L[3], float e[6]) {
    double l[3] = {L[0], L[1], L[2]};
    const double ln = sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
    for (double& x : l) x /= ln;
    int kmin = 0;
    for (int i = 1; i < 3; ++i)
        if (fabs(l[i]) < fabs(l[kmin])) kmin = i;
    double e1[3] = {0.0, 0.0, 0.0};
    e1[kmin] = 1.0;
    const double al = l[kmin];
    for (int i = 0; i < 3; ++i) e1[i] -= al * l[i];
    const double n1 = sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    for (double& x : e1) x /= n1;
    const double e2[3] = {l[1] * e1[2] - l[2] * e1[1], l[2] * e1[0] - l[0] * e1[2],
                          l[0] * e1[1] - l[1] * e1[0]};
    for (int i = 0; i < 3; ++i) {
        e[i] = static_cast<float>(e1[i]);
        e[3 + i] = static_cast<float>(e2[i]);
    }
}

// The root box's farthest corner from the world origin.  With 1e-4 added (by
// the callers) it is M, the bound on |origin| and |centre| of every shadow
// test: the root box holds every sphere, and a shadow origin is a hit point
// moved 1e-5 off its sphere.
inline double root_reach(const float mn[3], const float mx[3]) {
    double m = 0.0;
    for (int c = 0; c < 8; ++c) {
        double q = 0.0;
        for (int i = 0; i < 3; ++i) {
            const double v = (c >> i) & 1 ? mx[i] : mn[i];
            q += v * v;
        }
        m = std::max(m, sqrt(q));
    }
    return m;
}

// The occluder lists' bounds (R_i, the self-exclusion) hold the rounding of
// the hit point p = o_cam + t d, which grows with the camera's distance: they
// were derived for |o_cam| + (the camera's distance to the root box's farthest
// corner) <= gate, gate = kOccCamGate M.  False from
// farther away, and for a non-finite origin: such a frame walks.
inline bool occ_camera_in_gate(const float o[3], const float mn[3], const float mx[3], double gate) {
    double far2 = 0.0, o2 = 0.0;
    for (int i = 0; i < 3; ++i) {
        const double oi = o[i];
        const double d = std::max(fabs(oi - mn[i]), fabs(oi - mx[i]));
        far2 += d * d;
        o2 += oi * oi;
    }
    return sqrt(o2) + sqrt(far2) <= gate;
}

// Superblock claim order (FrameArgs::sb_order, RT_SB_ORDER): the cells of a
// Hilbert curve over the next power-of-two square, those inside the nx x ny
// superblock grid in curve order, as row-major indices.  The level-1 counter
// hands claims to the XCDs in turn, so an XCD's successive superblocks lie a
// few steps apart along the curve, near each other in the image, instead of
// eight columns apart in row-major order.
inline std::vector<uint32_t> hilbert_order(uint32_t nx, uint32_t ny) {
    uint32_t n = 1;
    while (n < nx || n < ny) n *= 2u;
    std::vector<uint32_t> out;
    out.reserve(size_t(nx) * ny);
    for (uint64_t d = 0; d < uint64_t(n) * n; ++d) {
        uint32_t x = 0, y = 0;
        uint64_t t = d;
        for (uint32_t s = 1; s < n; s *= 2u) {
            const uint32_t rx = 1u & static_cast<uint32_t>(t / 2), ry = 1u & static_cast<uint32_t>(t ^ rx);
            if (ry == 0) {
                if (rx == 1) {
                    x = s - 1u - x;
                    y = s - 1u - y;
                }
                std::swap(x, y);
            }
            x += s * rx;
            y += s * ry;
            t /= 4;
        }
        if (x < nx && y < ny) out.push_back(y * nx + x);
    }
    return out;
}

// Which pixels a progressive frame's sums belong to (accum_pixels): the full
// frame (1, ids == null) or one tile list (FNV-1a over its size, ids and
// length; bit 1 set, so never 1).
inline uint64_t pixel_set_signature(const uint32_t* ids, uint32_t n, uint32_t ts) {
    if (!ids) return 1;
    uint64_t sig = 1469598103934665603ull ^ ts;
    for (uint32_t i = 0; i < n; ++i) sig = (sig ^ ids[i]) * 1099511628211ull;
    return (sig ^ n) * 1099511628211ull | 2u;
}

}  // namespace rtamd
