// Prints csrc/rt_closest_math.h's results (tests/test_closest_cpu.py).  Floats
// travel as hexadecimal bit patterns, f32 in 8 digits.
//   box depth rmin[3] rmax[3] file  -> per record of `file` (raw f32 {px, py, pz,
//         bound}): lo[3] hi[3] (f32 bits): the grown box of that bound in the
//         grid coordinates of a depth-`depth` octree over that root box, with
//         scale = G / (rmax - rmin) in f32 as the host sets it (rt_scene.cpp)
//   keys file_probes file_spheres -> per probe one line: ok (0 | 1), then the
//         key of every sphere (f32 bits)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracingstudy_amd/csrc/rt_closest_math.h"

namespace {
int g_argc;
char** g_argv;
int g_next = 2;

const char* arg() {
    if (g_next >= g_argc) {
        fprintf(stderr, "closest_math_dump: too few arguments\n");
        exit(2);
    }
    return g_argv[g_next++];
}
float f32() {
    const uint32_t b = static_cast<uint32_t>(strtoul(arg(), nullptr, 16));
    float f;
    memcpy(&f, &b, sizeof(f));
    return f;
}
uint32_t bits(float f) {
    uint32_t b;
    memcpy(&b, &f, sizeof(b));
    return b;
}
std::vector<float> records(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "closest_math_dump: cannot open %s\n", path);
        exit(2);
    }
    std::vector<float> v;
    float rec[4];
    while (fread(rec, sizeof(float), 4, f) == 4) v.insert(v.end(), rec, rec + 4);
    fclose(f);
    return v;
}
}  // namespace

int main(int argc, char** argv) {
    g_argc = argc;
    g_argv = argv;
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "box") {
        const uint32_t depth = static_cast<uint32_t>(strtoul(arg(), nullptr, 10));
        if (depth > 16u) {
            fprintf(stderr, "closest_math_dump: depth over 16\n");
            return 2;
        }
        float rmin[3], rmax[3], scale[3];
        for (float& x : rmin) x = f32();
        for (float& x : rmax) x = f32();
        const float G = static_cast<float>(1u << depth);
        for (int i = 0; i < 3; ++i) scale[i] = G / (rmax[i] - rmin[i]);
        const float slack_m = rtamd::closest_slack_m(rmin, rmax);
        const std::vector<float> p = records(arg());
        for (size_t i = 0; i + 3 < p.size(); i += 4) {
            const rtamd::ClosestBox b =
                rtamd::closest_box(p[i], p[i + 1], p[i + 2], p[i + 3], rmin, scale, slack_m);
            printf("%08x %08x %08x %08x %08x %08x\n", bits(b.lo[0]), bits(b.lo[1]), bits(b.lo[2]),
                   bits(b.hi[0]), bits(b.hi[1]), bits(b.hi[2]));
        }
        return 0;
    }
    if (cmd == "keys") {
        const std::vector<float> p = records(arg());
        const std::vector<float> s = records(arg());
        for (size_t i = 0; i + 3 < p.size(); i += 4) {
            printf("%d", rtamd::closest_probe_ok(p[i], p[i + 1], p[i + 2], p[i + 3]) ? 1 : 0);
            for (size_t j = 0; j + 3 < s.size(); j += 4)
                printf(" %08x", bits(rtamd::closest_key(p[i], p[i + 1], p[i + 2], s[j], s[j + 1], s[j + 2],
                                                        s[j + 3])));
            putchar('\n');
        }
        return 0;
    }
    fprintf(stderr, "closest_math_dump: unknown command\n");
    return 2;
}
