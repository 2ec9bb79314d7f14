// Prints csrc/rt_filter_math.h's results (tests/test_filter_cpu.py).  Floats
// travel as hexadecimal bit patterns, f32 in 8 digits.
//   valid passes channels sigma normal_power flags -> filter_params_ok and the four
//         field checks, one digit each
//   floor f -> apply_floor_ok
//   taps -> filter_tap_k of the offsets -2 .. 2
//   plan passes -> per pass: step, source and destination (0 in, 1 out, 2 scratch),
//         then whether the plan needs the scratch layer
//   weights file -> per record of `file` (raw 44-byte {f32 k, n_p[3], n_q[3], t_p,
//         t_q, sigma, u32 normal_power}): filter_inv_depth and filter_weight
//   layer file -> the whole filter on the host, the specification's loops over the
//         header's functions and plan: `file` holds {u32 w, h, channels, passes,
//         normal_power, f32 sigma}, then w*h u32 sphere, w*h f32 t, w*h*4 f32
//         normals and w*h*channels f32 values; prints the output's words
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracingstudy_amd/csrc/rt_filter_math.h"

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

// one pass of include/rt.h's specification at tap spacing `step`
void pass(const std::vector<uint32_t>& sphere, const std::vector<float>& t, const std::vector<float>& nrm,
          const std::vector<float>& in, std::vector<float>& out, int w, int h, int c, int step, float sigma,
          uint32_t normal_power) {
    using namespace rtamd;
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t p = static_cast<size_t>(y) * w + x;
            if (sphere[p] == 0xFFFFFFFFu) {
                for (int ch = 0; ch < c; ++ch) out[p * c + ch] = in[p * c + ch];
                continue;
            }
            const float iz = filter_inv_depth(sigma, t[p]);
            float sw = 0.0f, sv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int j = -kFilterReach; j <= kFilterReach; ++j)
                for (int i = -kFilterReach; i <= kFilterReach; ++i) {
                    const int qx = x + i * step, qy = y + j * step;
                    if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                    const size_t q = static_cast<size_t>(qy) * w + qx;
                    if (sphere[q] == 0xFFFFFFFFu) continue;
                    const float wq = filter_weight(filter_tap_k(i) * filter_tap_k(j), &nrm[p * 4], &nrm[q * 4], t[p],
                                                   t[q], iz, normal_power);
                    sw += wq;
                    for (int ch = 0; ch < c; ++ch) sv[ch] += wq * in[q * c + ch];
                }
            for (int ch = 0; ch < c; ++ch) out[p * c + ch] = sw > 0.0f ? sv[ch] / sw : in[p * c + ch];
        }
}

int layer(const char* path) {
    using namespace rtamd;
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    uint32_t hd[5];
    float sigma;
    if (fread(hd, sizeof(hd), 1, f) != 1 || fread(&sigma, sizeof(sigma), 1, f) != 1) return 2;
    const int w = static_cast<int>(hd[0]), h = static_cast<int>(hd[1]), c = static_cast<int>(hd[2]);
    const uint32_t passes = hd[3], normal_power = hd[4];
    if (!filter_params_ok(passes, hd[2], sigma, normal_power, 0)) return 3;
    const size_t n = static_cast<size_t>(w) * h;
    std::vector<uint32_t> sphere(n);
    std::vector<float> t(n), nrm(n * 4), in(n * c), outb(n * c), scratch(n * c);
    if (fread(sphere.data(), 4, n, f) != n || fread(t.data(), 4, n, f) != n || fread(nrm.data(), 4, n * 4, f) != n * 4 ||
        fread(in.data(), 4, n * c, f) != n * c)
        return 2;
    fclose(f);
    std::vector<float>* buf[3] = {&in, &outb, &scratch};
    for (uint32_t s = 0; s < passes; ++s)
        pass(sphere, t, nrm, *buf[filter_pass_src(s, passes)], *buf[filter_pass_dst(s, passes)], w, h, c,
             static_cast<int>(filter_pass_step(s)), sigma, normal_power);
    for (float v : outb) printf("%08x\n", bits(v));
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    using namespace rtamd;
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "valid" && argc == 7) {
        const uint32_t passes = u32(argv[2]), channels = u32(argv[3]), np = u32(argv[5]), flags = u32(argv[6]);
        const float sigma = f32(argv[4]);
        printf("%d%d%d%d%d\n", filter_params_ok(passes, channels, sigma, np, flags) ? 1 : 0,
               filter_passes_ok(passes) ? 1 : 0, filter_channels_ok(channels) ? 1 : 0,
               filter_depth_sigma_ok(sigma) ? 1 : 0, filter_normal_power_ok(np) ? 1 : 0);
        return 0;
    }
    if (cmd == "floor" && argc == 3) {
        printf("%d\n", apply_floor_ok(f32(argv[2])) ? 1 : 0);
        return 0;
    }
    if (cmd == "taps" && argc == 2) {
        for (int o = -kFilterReach; o <= kFilterReach; ++o) printf("%08x\n", bits(filter_tap_k(o)));
        return 0;
    }
    if (cmd == "plan" && argc == 3) {
        const uint32_t passes = u32(argv[2]);
        for (uint32_t s = 0; s < passes; ++s)
            printf("%u %u %u\n", filter_pass_step(s), static_cast<uint32_t>(filter_pass_src(s, passes)),
                   static_cast<uint32_t>(filter_pass_dst(s, passes)));
        printf("%d\n", filter_needs_scratch(passes) ? 1 : 0);
        return 0;
    }
    if (cmd == "layer" && argc == 3) return layer(argv[2]);
    if (cmd != "weights" || argc != 3) {
        fprintf(stderr, "filter_math_dump: valid P C SIGMA NP FLAGS | floor F | taps | plan P | weights FILE | layer FILE\n");
        return 2;
    }
    FILE* f = fopen(argv[2], "rb");
    if (!f) {
        fprintf(stderr, "filter_math_dump: cannot open the records\n");
        return 2;
    }
    struct Rec {
        float k, n_p[3], n_q[3], t_p, t_q, sigma;
        uint32_t normal_power;
    } r;
    static_assert(sizeof(Rec) == 44, "a packed record");
    while (fread(&r, sizeof(r), 1, f) == 1) {
        const float iz = filter_inv_depth(r.sigma, r.t_p);
        printf("%08x %08x\n", bits(iz), bits(filter_weight(r.k, r.n_p, r.n_q, r.t_p, r.t_q, iz, r.normal_power)));
    }
    fclose(f);
    return 0;
}
