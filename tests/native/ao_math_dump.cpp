// Prints csrc/rt_ao_math.h's results (tests/test_ao_cpu.py).  Floats travel as
// hexadecimal bit patterns, f32 in 8 digits.
//   valid rays radius -> ao_rays_ok and ao_radius_ok, one digit each
//   dirs seed file -> per record of `file` (raw 24-byte {f32 n[3], u32 pid, u32 i,
//         u32 salt}): the direction's three words and whether it is the fallback,
//         under ao_key(mix32(seed ^ 0x9E3779B9), salt)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../raytracingstudy_amd/csrc/rt_ao_math.h"

namespace {
uint32_t bits(float f) {
    uint32_t b;
    memcpy(&b, &f, sizeof(b));
    return b;
}
float f32(const char* s) {
    const uint32_t b = static_cast<uint32_t>(strtoul(s, nullptr, 16));
    float f;
    memcpy(&f, &b, sizeof(f));
    return f;
}
}  // namespace

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "valid" && argc == 4) {
        printf("%d%d\n", rtamd::ao_rays_ok(static_cast<uint32_t>(strtoul(argv[2], nullptr, 10))) ? 1 : 0,
               rtamd::ao_radius_ok(f32(argv[3])) ? 1 : 0);
        return 0;
    }
    if (cmd != "dirs" || argc != 4) {
        fprintf(stderr, "ao_math_dump: valid RAYS RADIUS | dirs SEED FILE\n");
        return 2;
    }
    const uint32_t seed = static_cast<uint32_t>(strtoul(argv[2], nullptr, 10));
    const uint32_t seedmix = rtamd::ao_mix32(seed ^ 0x9E3779B9u);
    FILE* f = fopen(argv[3], "rb");
    if (!f) {
        fprintf(stderr, "ao_math_dump: cannot open the records\n");
        return 2;
    }
    struct Rec {
        float n[3];
        uint32_t pid, i, salt;
    } r;
    static_assert(sizeof(Rec) == 24, "a packed record");
    while (fread(&r, sizeof(r), 1, f) == 1) {
        float d0, d1, d2;
        const uint32_t hp = rtamd::ao_pixel_word(rtamd::ao_key(seedmix, r.salt), r.pid);
        const bool fb = rtamd::ao_direction(hp, r.i, r.n[0], r.n[1], r.n[2], d0, d1, d2);
        printf("%08x %08x %08x %d\n", bits(d0), bits(d1), bits(d2), fb ? 1 : 0);
    }
    fclose(f);
    return 0;
}
