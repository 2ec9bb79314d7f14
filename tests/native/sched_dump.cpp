// Prints csrc/rt_sched.h's results (tests/test_sched_cpu.py).  The command is
// argv[1]; each line of standard input is one row of decimal arguments, each
// line of output that row's result.
//   pick  variant spp progressive count_work sort_on have_occ have_bins tab_k stack_depth
//         -> valid waveq stats prog sorted occ bin min_waves w8 flags
//   grid  W H spp n_tiles tile_size
//         -> tw th gw gh nbx nby nsx nsy blocks superblocks units slot_shift
//   lds   sorted tab_k stack_depth
//         -> sums stacks sort_waves leaf_buf bytes
//   plan  variant spp progressive count_work sort_on tab_k stack_depth W H n_tiles tile_size opt
//         -> pick's ten (occ = bin = 0), grid's twelve, then
//            spw g ppw rounds slot_shift slot_stride lds_bytes ticket ticket_forced
//   waveq units resident cus per_simd ticket ticket_forced
//         -> grid ticket
//   btiles W H n_tiles tile_size tw th resident force
//         -> side grid
//   btlds lds_bytes spw opt
//         -> lds_bytes
#include <cstdio>
#include <cstring>

#include "../../raytracingstudy_amd/csrc/rt_sched.h"

using namespace rtamd;

// the instance flags name the switches they say they do
static_assert(Frame<kFTiles | kFStats | kFProg>::tiles && Frame<kFStats>::stats && Frame<kFProg>::prog &&
                  !Frame<kFStats | kFProg>::tiles && !Frame<kFStats>::waveq,
              "Frame<> decodes its flags");
static_assert(Frame<kFWaveQ | kFOcc | kFBin>::min_waves == 8 && Frame<kFWaveQ | kFStats>::min_waves == 7 &&
                  Frame<kFOcc>::min_waves == 1,
              "waves per SIMD follow the queue and the counters");
static_assert(Frame<kFWaveQ>::cam8 && !Frame<kFWaveQ | kFSorted>::cam8 && !Frame<0u>::cam8,
              "the image-plane screen: unsorted wave-queue walks");

static void print_instance(const SceneInstance& s, const char* end) {
    printf("%d %d %d %d %d %d %d %u %d %u%s", s.valid, s.waveq, s.stats, s.prog, s.sorted, s.occ, s.bin,
           s.min_waves(), s.w8(), s.flags(), end);
}
static void print_grid(const WaveGrid& g, const char* end) {
    printf("%u %u %u %u %u %u %u %u %u %u %llu %u%s", g.tw, g.th, g.gw, g.gh, g.nbx, g.nby, g.nsx, g.nsy,
           g.blocks(), g.superblocks(), static_cast<unsigned long long>(g.units()), g.slot_shift(), end);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        unsigned v[12] = {};
        unsigned long long units = 0;  // waveq's first argument is 64 bits wide
        const int n = sscanf(line, "%llu %u %u %u %u %u %u %u %u %u %u %u", &units, v + 1, v + 2, v + 3, v + 4,
                             v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11);
        v[0] = static_cast<unsigned>(units);
        if (!strcmp(argv[1], "pick") && n == 9) {
            print_instance(pick_scene_instance(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]), "\n");
        } else if (!strcmp(argv[1], "grid") && n == 5) {
            print_grid(WaveGrid(v[0], v[1], v[2], v[3], v[4]), "\n");
        } else if (!strcmp(argv[1], "plan") && n == 12) {
            const FramePlan p = plan_scene_frame(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9],
                                                 v[10], v[11]);
            print_instance(p.inst, " ");
            print_grid(p.grid, " ");
            printf("%u %u %u %u %u %u %u %u %d\n", p.spw, p.g, p.ppw, p.rounds, p.slot_shift, p.slot_stride,
                   p.lds_bytes, p.ticket, p.ticket_forced);
        } else if (!strcmp(argv[1], "waveq") && n == 6) {
            const WaveQueueLaunch s = size_wave_queue(units, v[1], v[2], v[3], v[4], v[5] != 0u);
            printf("%u %u\n", s.grid, s.ticket);
        } else if (!strcmp(argv[1], "btiles") && n == 8) {
            const BlockTileLaunch s = size_block_tiles(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
            printf("%u %u\n", s.side, s.grid);
        } else if (!strcmp(argv[1], "btlds") && n == 3) {
            printf("%u\n", block_tile_lds(v[0], v[1], v[2]));
        } else if (!strcmp(argv[1], "lds") && n == 3) {
            const FrameLds l(v[0] != 0u, v[1], v[2]);
            printf("%u %u %u %u %u\n", l.sums, l.stacks, l.sort_waves, l.leaf_buf, l.bytes);
        } else {
            fprintf(stderr, "sched_dump: bad command or row: %s %s", argv[1], line);
            return 2;
        }
    }
    return 0;
}
