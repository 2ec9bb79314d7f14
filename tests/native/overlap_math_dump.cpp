// Prints csrc/rt_overlap_math.h's results (tests/test_overlap_cpu.py).  Floats
// travel as hexadecimal bit patterns, f32 in 8 digits.
//   box depth rmin[3] rmax[3] file  -> per probe of `file` (raw f32 {px, py, pz, R}
//         records): ok(0 | 1) lo[3] hi[3] (f32 bits): the grown box in the grid
//         coordinates of a depth-`depth` octree over that root box, with
//         scale = G / (rmax - rmin) in f32 as the host sets it (rt_scene.cpp)
//   accepts file_probes file_spheres -> per probe one line of 0 | 1, one digit
//         per sphere: the predicate (and the probe's validity)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracingstudy_amd/csrc/rt_overlap_math.h"

namespace {
int g_argc;
char** g_argv;
int g_next = 2;

const char* arg() {
    if (g_next >= g_argc) {
        fprintf(stderr, "overlap_math_dump: too few arguments\n");
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
        fprintf(stderr, "overlap_math_dump: cannot open %s\n", path);
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
            fprintf(stderr, "overlap_math_dump: depth over 16\n");
            return 2;
        }
        float rmin[3], rmax[3], scale[3];
        for (float& x : rmin) x = f32();
        for (float& x : rmax) x = f32();
        const float G = static_cast<float>(1u << depth);
        for (int i = 0; i < 3; ++i) scale[i] = G / (rmax[i] - rmin[i]);
        const float slack_m = rtamd::overlap_slack_m(rmin, rmax);
        const std::vector<float> p = records(arg());
        for (size_t i = 0; i + 3 < p.size(); i += 4) {
            const bool ok = rtamd::overlap_probe_ok(p[i], p[i + 1], p[i + 2], p[i + 3]);
            const rtamd::OverlapBox b =
                rtamd::overlap_box(p[i], p[i + 1], p[i + 2], p[i + 3], rmin, scale, slack_m);
            printf("%d %08x %08x %08x %08x %08x %08x\n", ok ? 1 : 0, bits(b.lo[0]), bits(b.lo[1]),
                   bits(b.lo[2]), bits(b.hi[0]), bits(b.hi[1]), bits(b.hi[2]));
        }
        return 0;
    }
    if (cmd == "accepts") {
        const std::vector<float> p = records(arg());
        const std::vector<float> s = records(arg());
        std::string line;
        for (size_t i = 0; i + 3 < p.size(); i += 4) {
            line.clear();
            const bool ok = rtamd::overlap_probe_ok(p[i], p[i + 1], p[i + 2], p[i + 3]);
            for (size_t j = 0; j + 3 < s.size(); j += 4)
                line.push_back(ok && rtamd::overlap_accepts(p[i], p[i + 1], p[i + 2], p[i + 3], s[j],
                                                            s[j + 1], s[j + 2], s[j + 3])
                                   ? '1'
                                   : '0');
            puts(line.c_str());
        }
        return 0;
    }
    fprintf(stderr, "overlap_math_dump: unknown command\n");
    return 2;
}
