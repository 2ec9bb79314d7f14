// Prints csrc/rt_bins_math.h's tile-word functions (tests/test_bin_tiles_cpu.py).
//   index tw th      -> tiles per bin, then one line per pixel of a 16x16 block
//                       (two bins a side): x y bin_tile_index bin_tile_index_log2
//   words file       -> per line of `file` ("tw th cnt rect0 rect1 ..", rects in
//                       hexadecimal: x0 | x1 << 4 | y0 << 8 | y1 << 12): the
//                       words of the bin's tiles in index order, 16 hex digits each
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../raytracingstudy_amd/csrc/rt_bins_math.h"

namespace {
uint32_t log2_of(uint32_t v) {
    uint32_t l = 0;
    while ((1u << l) < v) ++l;
    return l;
}
}  // namespace

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "index" && argc == 4) {
        const uint32_t tw = static_cast<uint32_t>(strtoul(argv[2], nullptr, 10));
        const uint32_t th = static_cast<uint32_t>(strtoul(argv[3], nullptr, 10));
        printf("%u\n", rtamd::bin_tiles_per_bin(tw, th));
        for (uint32_t y = 0; y < 16; ++y)
            for (uint32_t x = 0; x < 16; ++x)
                printf("%u %u %u %u\n", x, y, rtamd::bin_tile_index(x, y, tw, th),
                       rtamd::bin_tile_index_log2(x, y, log2_of(tw), log2_of(th)));
    } else if (cmd == "words" && argc == 3) {
        std::ifstream in(argv[2]);
        if (!in) {
            fprintf(stderr, "bin_tiles_dump: cannot open the list file\n");
            return 2;
        }
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            uint32_t tw = 0, th = 0, cnt = 0;
            ls >> tw >> th >> cnt;
            std::vector<uint32_t> rects(cnt);
            for (uint32_t k = 0; k < cnt; ++k) ls >> std::hex >> rects[k];
            if (!ls || !tw || !th) {
                fprintf(stderr, "bin_tiles_dump: bad line\n");
                return 2;
            }
            const uint32_t tpb = rtamd::bin_tiles_per_bin(tw, th);
            for (uint32_t t = 0; t < tpb; ++t)
                printf("%016" PRIx64 "%c", rtamd::bin_tile_word(rects.data(), cnt, t, tw, th),
                       t + 1 == tpb ? '\n' : ' ');
        }
    } else {
        fprintf(stderr, "bin_tiles_dump: unknown command\n");
        return 2;
    }
    return 0;
}
