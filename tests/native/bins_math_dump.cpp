// Prints csrc/rt_bins_math.h's results (tests/test_bins_cpu.py).  Floats
// travel as hexadecimal bit patterns, f32 in 8 digits and f64 in 16.
//   rect  W H shrink(f64) K[9] R[9] o[3] file  -> per sphere of `file` (raw f32
//         {cx, cy, cz, r} records): class x0 y0 x1 y1 near(f32 bits)
//   camok K[9] R[9] o[3]                       -> 0 | 1
//   framegate W H K[9] R[9] o[3]               -> 0 | 1: the host's gate of a W x H
//         frame (rt_bins_host.cpp screen_bins: bins_camera_ok and cam8_basis)
//   cadence gen,mframe,mflag ...               -> per plain frame "skip" | "build": the
//         dense-skip step (bin_dense_skip_step) over frames 1, 2, ... of scene
//         generation `gen`, each seeing the pinned frame and flag words mframe and
//         mflag; a frame that builds becomes the last building frame, as in
//         rt_bins_host.cpp screen_bins
//   want captest n mframe mflag mentries lastframe ent_n -> the entries wanted
//         (bin_entries_wanted)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracingstudy_amd/csrc/rt_bins_math.h"
#include "../../raytracingstudy_amd/csrc/rt_frame_math.h"

namespace {
int g_argc;
char** g_argv;
int g_next = 2;

const char* arg() {
    if (g_next >= g_argc) {
        fprintf(stderr, "bins_math_dump: too few arguments\n");
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
double f64() {
    const uint64_t b = strtoull(arg(), nullptr, 16);
    double d;
    memcpy(&d, &b, sizeof(d));
    return d;
}
uint32_t u32() { return static_cast<uint32_t>(strtoul(arg(), nullptr, 10)); }
void vec(float* v, int n) {
    for (int i = 0; i < n; ++i) v[i] = f32();
}
}  // namespace

int main(int argc, char** argv) {
    g_argc = argc;
    g_argv = argv;
    const std::string cmd = argc > 1 ? argv[1] : "";
    float K[9], R[9], o[3];
    if (cmd == "rect") {
        const uint32_t W = u32(), H = u32();
        const double shrink = f64();
        vec(K, 9);
        vec(R, 9);
        vec(o, 3);
        FILE* f = fopen(arg(), "rb");
        if (!f) {
            fprintf(stderr, "bins_math_dump: cannot open the sphere file\n");
            return 2;
        }
        std::vector<float> sp;
        float rec[4];
        while (fread(rec, sizeof(float), 4, f) == 4) sp.insert(sp.end(), rec, rec + 4);
        fclose(f);
        for (size_t i = 0; i + 4 <= sp.size(); i += 4) {
            const rtamd::BinRect rc = rtamd::sphere_screen_rect(&sp[i], K, R, o, W, H, shrink);
            uint32_t nb;
            memcpy(&nb, &rc.near_t, sizeof(nb));
            printf("%u %u %u %u %u %08x\n", rc.cls, rc.x0, rc.y0, rc.x1, rc.y1, nb);
        }
    } else if (cmd == "camok") {
        vec(K, 9);
        vec(R, 9);
        vec(o, 3);
        printf("%d\n", rtamd::bins_camera_ok(K, R, o) ? 1 : 0);
    } else if (cmd == "framegate") {
        const uint32_t W = u32(), H = u32();
        float B[9];
        vec(K, 9);
        vec(R, 9);
        vec(o, 3);
        printf("%d\n", rtamd::bins_camera_ok(K, R, o) && rtamd::cam8_basis(K, R, W, H, B) ? 1 : 0);
    } else if (cmd == "cadence") {
        rtamd::BinCadence c;
        for (uint32_t frame = 1; g_next < g_argc; ++frame) {
            unsigned long long gen;
            unsigned mframe, mflag;
            if (sscanf(arg(), "%llu,%u,%u", &gen, &mframe, &mflag) != 3) {
                fprintf(stderr, "bins_math_dump: cadence takes gen,mframe,mflag\n");
                return 2;
            }
            const bool skip = rtamd::bin_dense_skip_step(c, gen, mframe, mflag);
            if (!skip) c.last_frame = frame;
            printf("%s\n", skip ? "skip" : "build");
        }
    } else if (cmd == "want") {
        const uint32_t captest = u32(), n = u32(), mframe = u32(), mflag = u32(), mentries = u32(),
                       lastframe = u32();
        const size_t ent_n = strtoull(arg(), nullptr, 10);
        printf("%zu\n", rtamd::bin_entries_wanted(captest, n, mframe, mflag, mentries, lastframe, ent_n));
    } else {
        fprintf(stderr, "bins_math_dump: unknown command '%s'\n", cmd.c_str());
        return 2;
    }
    return 0;
}
