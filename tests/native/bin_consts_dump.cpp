// bin_consts_dump — the frame-constant word of the screen-space bins
// (csrc/rt_bins_math.h) on the CPU, for
// tests/test_bin_consts_cpu.py.  Built with the address and
// undefined-behaviour sanitizers.
//   bin_consts_dump all
//       every (flag word, wide count, ltw, lth) that fits, one line each:
//       "flag wide ltw lth word flag' wide' ltw' lth'" (flag, word in hex)
//   bin_consts_dump fit <wide> <ltw> <lth>
//       "1" if the three fit the word, else "0"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../raytracingstudy_amd/csrc/rt_bins_math.h"

using namespace rtamd;

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "all")) {
        const uint32_t flags[] = {0u, kBinFlagCapacity, kBinFlagWide, kBinFlagDense,
                                  kBinFlagCapacity | kBinFlagWide | kBinFlagDense, 0x80000000u, 0xFFFFFFFFu};
        for (uint32_t flag : flags)
            for (uint32_t wide = 0; wide <= kBinWideCap + 8u; ++wide)
                for (uint32_t ltw = 0; ltw <= kBinShift + 1u; ++ltw)
                    for (uint32_t lth = 0; lth <= kBinShift + 1u; ++lth) {
                        if (!bin_consts_fit(wide, ltw, lth)) continue;
                        const uint32_t c = bin_consts_pack(flag, wide, ltw, lth);
                        printf("%x %u %u %u %x %u %u %u %u\n", flag, wide, ltw, lth, c,
                               bin_consts_flag(c) ? 1u : 0u, bin_consts_wide(c), bin_consts_ltw(c),
                               bin_consts_lth(c));
                    }
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "fit")) {
        const uint32_t wide = static_cast<uint32_t>(strtoul(argv[2], nullptr, 0));
        const uint32_t ltw = static_cast<uint32_t>(strtoul(argv[3], nullptr, 0));
        const uint32_t lth = static_cast<uint32_t>(strtoul(argv[4], nullptr, 0));
        printf("%d\n", bin_consts_fit(wide, ltw, lth) ? 1 : 0);
        return 0;
    }
    fprintf(stderr, "usage: bin_consts_dump all | fit <wide> <ltw> <lth>\n");
    return 2;
}
