// Walks one slot of the wave queue the way scene_body's ticket loop does and
// prints which wave tiles csrc/rt_sched.h's pair_starts shades together
// (tests/test_pair_rule_cpu.py).
//   gw gh chunk ks  -> the slot at the grid's origin (ks = 12: a superblock of
//                      64x64 wave tiles, ks = 6: one 8x8 block), its tickets of
//                      `chunk` tiles in order; per shaded unit one line:
//                      "S wx wy"  a tile shaded alone
//                      "P wx wy"  the pair (wx, wy), (wx + 1, wy); the second
//                                 may lie off the grid (padding of an edge block)
//   plan spp opt occ bins prog stats -> the Frame<> switches (SceneInstance::flags)
//                      of a 70x44 frame's instance once its occluder lists and
//                      bins are known (0 / 1 each)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../raytracingstudy_amd/csrc/rt_sched.h"

int main(int argc, char** argv) {
    if (argc == 8 && !strcmp(argv[1], "plan")) {
        uint32_t v[6];
        for (int i = 0; i < 6; ++i) v[i] = static_cast<uint32_t>(strtoul(argv[2 + i], nullptr, 10));
        const rtamd::FramePlan p =
            rtamd::plan_scene_frame(0u, v[0], v[4] != 0u, v[5] != 0u, true, 4u, 8u, 70u, 44u, 0u, 0u, v[1]);
        printf("%u\n", p.inst.with(v[2] != 0u, v[3] != 0u).flags());
        return 0;
    }
    if (argc != 5) {
        fprintf(stderr, "pair_rule_dump: gw gh chunk ks\n");
        return 2;
    }
    const uint32_t gw = static_cast<uint32_t>(strtoul(argv[1], nullptr, 10));
    const uint32_t gh = static_cast<uint32_t>(strtoul(argv[2], nullptr, 10));
    const uint32_t chunk = static_cast<uint32_t>(strtoul(argv[3], nullptr, 10));
    const uint32_t ks = static_cast<uint32_t>(strtoul(argv[4], nullptr, 10));
    if (!gw || !gh || !chunk || 32u % chunk || (ks != 6u && ks != 12u)) {
        fprintf(stderr, "pair_rule_dump: bad argument\n");
        return 2;
    }
    const uint32_t sx0 = 0, sy0 = 0;
    for (uint32_t u0 = 0; u0 < (1u << ks); u0 += chunk) {  // the slot's tickets
        const uint32_t w0 = u0 & ((1u << ks) - 1u);
        for (uint32_t cur = w0; cur < w0 + chunk; ++cur) {
            const uint32_t b = cur >> 6, w = cur & 63u;
            const uint32_t wx = sx0 + (b & 7u) * 8u + (w & 7u);
            const uint32_t wy = sy0 + (b >> 3) * 8u + (w >> 3);
            if (wx >= gw || wy >= gh) continue;  // padding of an edge block
            if (rtamd::pair_starts(cur, w0, chunk)) {
                printf("P %u %u\n", wx, wy);
                ++cur;
                continue;
            }
            printf("S %u %u\n", wx, wy);
        }
    }
    return 0;
}
