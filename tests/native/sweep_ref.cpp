// sweep_ref.cpp — the CPU reference of the swept-sphere query,
// a stand-alone program for tests/sweep_ref.py.
//
//   sweep_ref <spheres.f32> <rays.f32> <radii.f32> <flags> <out.u32>
//
// spheres.f32: m x {cx, cy, cz, r}; rays.f32: n x {origin xyz, tmin, dir xyz,
// tmax} (rt_ray); radii.f32: n x R; all raw little-endian float32.  flags: 1 =
// entry only, 2 = skip self.  For every cast it tests EVERY sphere (no octree)
// with the ray-sphere test of DESIGN.md 2.2 against the radius r + R, written
// here from that section with explicit fmaf and without the product's
// headers, and keeps the smallest (t, sphere index).  out.u32 holds n records
// {t bits, sphere index}, a miss {tmax bits, 0xFFFFFFFF}.
// Built with -ffp-contract=off: every rounding below is the one written.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

namespace {

// DESIGN.md 2.2 "Ray-sphere" with s for r: b = (o - c) . d by two FMAs on a
// product, q the component of o - c perpendicular to d, h = s^2 - |q|^2; the
// near root -b - sqrt(h), or (unless entry_only) the far root when the near
// one is not past tmin; accepted iff tmin < t < tmax.
bool isect(const float o[3], const float d[3], const float c[3], float s, float tmin, float tmax,
           bool entry_only, float* tout) {
    const float ocx = o[0] - c[0];
    const float ocy = o[1] - c[1];
    const float ocz = o[2] - c[2];
    const float b = fmaf(ocz, d[2], fmaf(ocy, d[1], ocx * d[0]));
    const float qx = fmaf(-b, d[0], ocx);
    const float qy = fmaf(-b, d[1], ocy);
    const float qz = fmaf(-b, d[2], ocz);
    const float qq = fmaf(qz, qz, fmaf(qy, qy, qx * qx));
    const float h = fmaf(s, s, -qq);
    if (h < 0.0f) return false;
    const float sq = sqrtf(h);
    float t = -b - sq;
    if (!(t > tmin)) {
        if (entry_only) return false;
        t = -b + sq;
    }
    if (!(t > tmin) || !(t < tmax)) return false;
    *tout = t;
    return true;
}

// origin and direction finite, R finite and >= 0, the direction of unit length
// to 2^-18 in f32
bool valid(const float o[3], const float d[3], float R) {
    for (int c = 0; c < 3; ++c)
        if (!isfinite(o[c]) || !isfinite(d[c])) return false;
    if (!isfinite(R) || !(R >= 0.0f)) return false;
    const float n2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    return fabsf(n2 - 1.0f) <= 0x1p-18f;
}

std::vector<float> read_f32(const char* path, size_t per) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "sweep_ref: cannot open %s\n", path);
        exit(2);
    }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 0 || static_cast<size_t>(bytes) % (per * sizeof(float)) != 0) {
        fprintf(stderr, "sweep_ref: %s is not a whole number of %zu-float records\n", path, per);
        exit(2);
    }
    std::vector<float> v(static_cast<size_t>(bytes) / sizeof(float));
    if (!v.empty() && fread(v.data(), sizeof(float), v.size(), f) != v.size()) {
        fprintf(stderr, "sweep_ref: short read of %s\n", path);
        exit(2);
    }
    fclose(f);
    return v;
}

uint32_t bits(float x) {
    uint32_t u;
    memcpy(&u, &x, sizeof(u));
    return u;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 6) {
        fprintf(stderr, "usage: sweep_ref <spheres.f32> <rays.f32> <radii.f32> <flags> <out.u32>\n");
        return 2;
    }
    const std::vector<float> sp = read_f32(argv[1], 4);
    const std::vector<float> rays = read_f32(argv[2], 8);
    const std::vector<float> radii = read_f32(argv[3], 1);
    const long flags = strtol(argv[4], nullptr, 10);
    const size_t m = sp.size() / 4, n = rays.size() / 8;
    if (radii.size() != n || flags < 0 || flags > 3) {
        fprintf(stderr, "sweep_ref: one radius per ray, flags 0..3\n");
        return 2;
    }
    const bool entry_only = (flags & 1) != 0, skip_self = (flags & 2) != 0;
    std::vector<uint32_t> out(2 * n);
    for (size_t i = 0; i < n; ++i) {
        const float* r = &rays[8 * i];
        const float o[3] = {r[0], r[1], r[2]}, d[3] = {r[4], r[5], r[6]};
        const float tmin = r[3], tmax = r[7], R = radii[i];
        float best_t = tmax;
        uint32_t best = 0xFFFFFFFFu;
        const bool ok = valid(o, d, R);
        for (size_t j = 0; ok && j < m; ++j) {
            if (skip_self && j == i) continue;
            const float s = sp[4 * j + 3] + R;  // one f32 add
            float t;
            if (!isect(o, d, &sp[4 * j], s, tmin, tmax, entry_only, &t)) continue;
            // t ascending (as floats: -0 == +0), then sphere index ascending: j only grows
            if (best == 0xFFFFFFFFu || t < best_t) {
                best_t = t;
                best = static_cast<uint32_t>(j);
            }
        }
        out[2 * i] = bits(best_t);
        out[2 * i + 1] = best;
    }
    FILE* f = fopen(argv[5], "wb");
    if (!f || (!out.empty() && fwrite(out.data(), sizeof(uint32_t), out.size(), f) != out.size())) {
        fprintf(stderr, "sweep_ref: cannot write %s\n", argv[5]);
        return 2;
    }
    fclose(f);
    return 0;
}
