// multihit_ref.cpp — the CPU reference of the ordered multi-hit query
// (DESIGN.md 5.9), a stand-alone program for tests/multihit_ref.py.
//
//   multihit_ref <spheres.f32> <rays.f32> <k> <out.u32>
//
// spheres.f32: m x {cx, cy, cz, r}; rays.f32: n x {origin xyz, tmin, dir xyz,
// tmax} (rt_ray); both raw little-endian float32.  For every ray it tests
// EVERY sphere (no octree) with the ray-sphere test of DESIGN.md 2.2, written
// here from that section with explicit fmaf, and keeps the k smallest
// (t, sphere index).  out.u32 holds n records of 2k + 2 words: k x {t bits,
// sphere index} (free slots {tmax bits, 0xFFFFFFFF}), min(k, size of the
// accepted set), and the size of the accepted set.
// Built with -ffp-contract=off: every rounding below is the one written.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace {

struct Hit {
    float t;
    uint32_t sphere;
};

// DESIGN.md 2.2 "Ray-sphere": b = (o - c) . d by two FMAs on a product, q the
// component of o - c perpendicular to d, h = r^2 - |q|^2; the near root
// -b - sqrt(h), or the far root when the near one is not past tmin; accepted
// iff tmin < t < tmax.
bool isect(const float o[3], const float d[3], const float s[4], float tmin, float tmax, float* tout) {
    const float ocx = o[0] - s[0];
    const float ocy = o[1] - s[1];
    const float ocz = o[2] - s[2];
    const float b = fmaf(ocz, d[2], fmaf(ocy, d[1], ocx * d[0]));
    const float qx = fmaf(-b, d[0], ocx);
    const float qy = fmaf(-b, d[1], ocy);
    const float qz = fmaf(-b, d[2], ocz);
    const float qq = fmaf(qz, qz, fmaf(qy, qy, qx * qx));
    const float h = fmaf(s[3], s[3], -qq);
    if (h < 0.0f) return false;
    const float sq = sqrtf(h);
    float t = -b - sq;
    if (!(t > tmin)) t = -b + sq;
    if (!(t > tmin) || !(t < tmax)) return false;
    *tout = t;
    return true;
}

std::vector<float> read_f32(const char* path, size_t per) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "multihit_ref: cannot open %s\n", path);
        exit(2);
    }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 0 || static_cast<size_t>(bytes) % (per * sizeof(float)) != 0) {
        fprintf(stderr, "multihit_ref: %s is not a whole number of %zu-float records\n", path, per);
        exit(2);
    }
    std::vector<float> v(static_cast<size_t>(bytes) / sizeof(float));
    if (!v.empty() && fread(v.data(), sizeof(float), v.size(), f) != v.size()) {
        fprintf(stderr, "multihit_ref: short read of %s\n", path);
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
    if (argc != 5) {
        fprintf(stderr, "usage: multihit_ref <spheres.f32> <rays.f32> <k> <out.u32>\n");
        return 2;
    }
    const std::vector<float> sp = read_f32(argv[1], 4);
    const std::vector<float> rays = read_f32(argv[2], 8);
    const long kl = strtol(argv[3], nullptr, 10);
    if (kl < 1 || kl > 4096) {
        fprintf(stderr, "multihit_ref: k out of range\n");
        return 2;
    }
    const size_t k = static_cast<size_t>(kl), m = sp.size() / 4, n = rays.size() / 8;
    std::vector<uint32_t> out(n * (2 * k + 2));
    std::vector<Hit> set;
    for (size_t i = 0; i < n; ++i) {
        const float* r = &rays[8 * i];
        const float o[3] = {r[0], r[1], r[2]}, d[3] = {r[4], r[5], r[6]};
        const float tmin = r[3], tmax = r[7];
        set.clear();
        // a ray with a NaN or infinite origin or direction component has an empty set
        bool finite = true;
        for (int c = 0; c < 3; ++c) finite = finite && isfinite(o[c]) && isfinite(d[c]);
        for (size_t j = 0; finite && j < m; ++j) {
            float t;
            if (isect(o, d, &sp[4 * j], tmin, tmax, &t)) set.push_back({t, static_cast<uint32_t>(j)});
        }
        // t ascending (as floats: -0 == +0), then sphere index ascending
        std::sort(set.begin(), set.end(), [](const Hit& a, const Hit& b) {
            return a.t < b.t || (a.t == b.t && a.sphere < b.sphere);
        });
        uint32_t* w = &out[i * (2 * k + 2)];
        for (size_t s = 0; s < k; ++s) {
            const bool held = s < set.size();
            w[2 * s] = bits(held ? set[s].t : tmax);
            w[2 * s + 1] = held ? set[s].sphere : 0xFFFFFFFFu;
        }
        w[2 * k] = static_cast<uint32_t>(std::min(k, set.size()));
        w[2 * k + 1] = static_cast<uint32_t>(set.size());
    }
    FILE* f = fopen(argv[4], "wb");
    if (!f || (!out.empty() && fwrite(out.data(), sizeof(uint32_t), out.size(), f) != out.size())) {
        fprintf(stderr, "multihit_ref: cannot write %s\n", argv[4]);
        return 2;
    }
    fclose(f);
    return 0;
}
