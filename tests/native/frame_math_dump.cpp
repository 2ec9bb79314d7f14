// Prints csrc/rt_frame_math.h's results for inputs given on the command line
// (tests/test_frame_math.py).  Floats travel as hexadecimal bit patterns, f32
// in 8 digits and f64 in 16, so a NaN or a last-place difference survives.
//   light   L[3]                       -> e[6]
//   cam8    W H K[9] R[9]              -> ok B[9]
//   reach   mn[3] mx[3]                -> reach (f64)
//   gate    o[3] mn[3] mx[3] gate(f64) -> 0 | 1
//   hilbert nx ny                      -> the order, decimal
//   sig     frame | ts id...           -> the pixel-set signature, decimal
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../raytracingstudy_amd/csrc/rt_frame_math.h"

namespace {
int g_argc;
char** g_argv;
int g_next = 2;

const char* arg() {
    if (g_next >= g_argc) {
        fprintf(stderr, "frame_math_dump: too few arguments\n");
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
void print(const float* v, int n) {
    for (int i = 0; i < n; ++i) {
        uint32_t b;
        memcpy(&b, &v[i], sizeof(b));
        printf("%08x ", b);
    }
}
}  // namespace

int main(int argc, char** argv) {
    g_argc = argc;
    g_argv = argv;
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "light") {
        float L[3], e[6];
        vec(L, 3);
        rtamd::light_plane_basis(L, e);
        print(e, 6);
    } else if (cmd == "cam8") {
        const uint32_t W = u32(), H = u32();
        float K[9], R[9], B[9];
        vec(K, 9);
        vec(R, 9);
        printf("%u ", rtamd::cam8_basis(K, R, W, H, B));
        print(B, 9);
    } else if (cmd == "reach") {
        float mn[3], mx[3];
        vec(mn, 3);
        vec(mx, 3);
        const double m = rtamd::root_reach(mn, mx);
        uint64_t b;
        memcpy(&b, &m, sizeof(b));
        printf("%016llx", static_cast<unsigned long long>(b));
    } else if (cmd == "gate") {
        float o[3], mn[3], mx[3];
        vec(o, 3);
        vec(mn, 3);
        vec(mx, 3);
        printf("%d", rtamd::occ_camera_in_gate(o, mn, mx, f64()) ? 1 : 0);
    } else if (cmd == "hilbert") {
        const uint32_t nx = u32(), ny = u32();
        for (uint32_t i : rtamd::hilbert_order(nx, ny)) printf("%u ", i);
    } else if (cmd == "sig") {
        std::vector<uint32_t> ids;
        if (std::string(argv[argc - 1]) == "frame") {
            printf("%llu", static_cast<unsigned long long>(rtamd::pixel_set_signature(nullptr, 0, 0)));
        } else {
            const uint32_t ts = u32();
            while (g_next < argc) ids.push_back(u32());
            printf("%llu", static_cast<unsigned long long>(rtamd::pixel_set_signature(
                               ids.data(), static_cast<uint32_t>(ids.size()), ts)));
        }
    } else {
        fprintf(stderr, "frame_math_dump: unknown command '%s'\n", cmd.c_str());
        return 2;
    }
    printf("\n");
    return 0;
}
