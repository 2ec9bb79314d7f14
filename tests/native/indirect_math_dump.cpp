// Prints csrc/rt_indirect_math.h's results (tests/test_indirect_cpu.py).  Floats
// travel as hexadecimal bit patterns, f32 in 8 digits; every FILE holds raw packed
// little-endian records.
//   valid rays radius sky_scale flags -> ao_rays_ok, ao_radius_ok, indirect_scale_ok and
//         indirect_params_ok, one digit each
//   sky file  -> per record {f32 dy, f32 dz, f32 sky_scale}: indirect_sky's three words
//   hit file  -> per record {u32 al, f32 ambient, f32 lam}: indirect_hit_color's three words
//   sum rays file -> per record of `rays` f32: the array after indirect_tree_sum, then
//         indirect_mean of element 0
//   open rays hits -> indirect_open's word
//   add file  -> per record {u32 px, f32 layer[3], u32 al, u32 has_albedo, f32 gain}:
//         add_layer_pixel's word
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../raytracingstudy_amd/csrc/rt_indirect_math.h"

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
uint32_t u32(const char* s) { return static_cast<uint32_t>(strtoul(s, nullptr, 10)); }

struct SkyRec {
    float dy, dz, sky;
};
struct HitRec {
    uint32_t al;
    float ambient, lam;
};
struct AddRec {
    uint32_t px;
    float layer[3];
    uint32_t al, has_albedo;
    float gain;
};
static_assert(sizeof(SkyRec) == 12 && sizeof(HitRec) == 12 && sizeof(AddRec) == 28, "packed records");
}  // namespace

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "valid" && argc == 6) {
        const uint32_t rays = u32(argv[2]), flags = u32(argv[5]);
        const float radius = f32(argv[3]), sky = f32(argv[4]);
        printf("%d%d%d%d\n", rtamd::ao_rays_ok(rays) ? 1 : 0, rtamd::ao_radius_ok(radius) ? 1 : 0,
               rtamd::indirect_scale_ok(sky) ? 1 : 0, rtamd::indirect_params_ok(rays, radius, sky, flags) ? 1 : 0);
        return 0;
    }
    if (cmd == "open" && argc == 4) {
        printf("%08x\n", bits(rtamd::indirect_open(u32(argv[2]), u32(argv[3]))));
        return 0;
    }
    const bool sum = cmd == "sum" && argc == 4;
    if (!sum && !((cmd == "sky" || cmd == "hit" || cmd == "add") && argc == 3)) {
        fprintf(stderr, "indirect_math_dump: valid RAYS RADIUS SKY FLAGS | sky FILE | hit FILE | sum RAYS FILE | "
                        "open RAYS HITS | add FILE\n");
        return 2;
    }
    FILE* f = fopen(argv[sum ? 3 : 2], "rb");
    if (!f) {
        fprintf(stderr, "indirect_math_dump: cannot open the records\n");
        return 2;
    }
    if (cmd == "sky") {
        SkyRec r;
        while (fread(&r, sizeof(r), 1, f) == 1) {
            float c[3];
            rtamd::indirect_sky(r.dy, r.dz, r.sky, c);
            printf("%08x %08x %08x\n", bits(c[0]), bits(c[1]), bits(c[2]));
        }
    } else if (cmd == "hit") {
        HitRec r;
        while (fread(&r, sizeof(r), 1, f) == 1) {
            float c[3];
            rtamd::indirect_hit_color(r.al, r.ambient, r.lam, c);
            printf("%08x %08x %08x\n", bits(c[0]), bits(c[1]), bits(c[2]));
        }
    } else if (cmd == "add") {
        AddRec r;
        while (fread(&r, sizeof(r), 1, f) == 1)
            printf("%08x\n", rtamd::add_layer_pixel(r.px, r.layer, r.al, r.has_albedo != 0u, r.gain));
    } else {
        const uint32_t rays = u32(argv[2]);
        if (!rtamd::ao_rays_ok(rays)) {
            fclose(f);
            fprintf(stderr, "indirect_math_dump: rays must be 1, 2, 4, .. 64\n");
            return 2;
        }
        float v[rtamd::kAoMaxRays];
        while (fread(v, sizeof(float), rays, f) == rays) {
            rtamd::indirect_tree_sum(v, rays);
            for (uint32_t i = 0; i < rays; ++i) printf("%08x ", bits(v[i]));
            printf("%08x\n", bits(rtamd::indirect_mean(v[0], rays)));
        }
    }
    fclose(f);
    return 0;
}
