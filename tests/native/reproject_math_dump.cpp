// Prints csrc/rt_reproject_math.h's results (tests/test_reproject_cpu.py).  Floats
// travel as hexadecimal bit patterns, f32 in 8 digits.
//   valid channels max_count depth_tol flags -> reproject_params_ok and the three
//         field checks, one digit each
//   points file -> per record of `file` (raw 136-byte {f32 pose[16], K[9], o[3], d[3],
//         t, u32 W, H}: the previous camera, the current origin, ray and hit
//         distance, the image size): u0 v0 a b dist, then front, the inside digits
//         of u0, u0 + 1, v0, v0 + 1, then the four taps' weights (j outer, i inner)
//   taps file -> per record (raw 20-byte {u32 s, s_hist, f32 dist, t_hist,
//         depth_tol}): tap_accepted
//   image file -> the whole pass on the host, reproject_pixel over every pixel:
//         `file` holds {u32 w, h, channels, has_history, f32 max_count, depth_tol,
//         o[3]}, w*h*3 f32 rays, w*h u32 sphere, w*h f32 t, w*h*channels f32 values,
//         and with a history {f32 pose[16], K[9]}, w*h u32 sphere, w*h f32 t,
//         w*h*channels f32 layer, w*h f32 count; prints the output's words, then
//         the counts'
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracingstudy_amd/csrc/rt_reproject_math.h"

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

template <typename T>
bool get(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <uint32_t kC>
void image_pixels(const rtamd::PrevCamera& c, const float o[3], uint32_t w, uint32_t h, const std::vector<float>& d,
                  const std::vector<uint32_t>& sphere, const std::vector<float>& t, const std::vector<float>& cur,
                  const uint32_t* hist_hits, const float* hist_layer, const float* hist_count, float max_count,
                  float depth_tol, std::vector<float>& out, std::vector<float>& count) {
    for (size_t p = 0; p < static_cast<size_t>(w) * h; ++p)
        count[p] = rtamd::reproject_pixel<kC>(c, o, &d[3 * p], t[p], sphere[p], &cur[kC * p], w, h, hist_hits,
                                              hist_layer, hist_count, max_count, depth_tol, &out[kC * p]);
}

int image(const char* path) {
    using namespace rtamd;
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    uint32_t hd[4];
    float fl[5];
    if (fread(hd, sizeof(hd), 1, f) != 1 || fread(fl, sizeof(fl), 1, f) != 1) return 2;
    const uint32_t w = hd[0], h = hd[1], c = hd[2];
    if (!reproject_params_ok(c, fl[0], fl[1], 0)) return 3;
    const size_t n = static_cast<size_t>(w) * h;
    std::vector<float> d, t, cur, cam, ht, hl, hc;
    std::vector<uint32_t> sphere, hs, hist_hits;
    if (!get(f, d, 3 * n) || !get(f, sphere, n) || !get(f, t, n) || !get(f, cur, n * c)) return 2;
    PrevCamera prev{};
    if (hd[3]) {
        if (!get(f, cam, 25) || !get(f, hs, n) || !get(f, ht, n) || !get(f, hl, n * c) || !get(f, hc, n)) return 2;
        prev = prev_camera(&cam[0], &cam[16]);
        hist_hits.resize(2 * n);  // rt_hit records: {t bits, sphere}
        for (size_t p = 0; p < n; ++p) hist_hits[2 * p] = bits(ht[p]), hist_hits[2 * p + 1] = hs[p];
    }
    fclose(f);
    std::vector<float> out(n * c), count(n);
    const uint32_t* hh = hd[3] ? hist_hits.data() : nullptr;
    if (c == 4u) image_pixels<4>(prev, &fl[2], w, h, d, sphere, t, cur, hh, hl.data(), hc.data(), fl[0], fl[1], out, count);
    else image_pixels<1>(prev, &fl[2], w, h, d, sphere, t, cur, hh, hl.data(), hc.data(), fl[0], fl[1], out, count);
    for (float v : out) printf("%08x\n", bits(v));
    for (float v : count) printf("%08x\n", bits(v));
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    using namespace rtamd;
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "valid" && argc == 6) {
        const uint32_t channels = u32(argv[2]), flags = u32(argv[5]);
        const float max_count = f32(argv[3]), tol = f32(argv[4]);
        printf("%d%d%d%d\n", reproject_params_ok(channels, max_count, tol, flags) ? 1 : 0,
               reproject_channels_ok(channels) ? 1 : 0, reproject_max_count_ok(max_count) ? 1 : 0,
               reproject_depth_tol_ok(tol) ? 1 : 0);
        return 0;
    }
    if (cmd == "image" && argc == 3) return image(argv[2]);
    if ((cmd != "points" && cmd != "taps") || argc != 3) {
        fprintf(stderr, "reproject_math_dump: valid C MAXCOUNT TOL FLAGS | points FILE | taps FILE | image FILE\n");
        return 2;
    }
    FILE* f = fopen(argv[2], "rb");
    if (!f) {
        fprintf(stderr, "reproject_math_dump: cannot open the records\n");
        return 2;
    }
    if (cmd == "taps") {
        struct Rec {
            uint32_t s, s_hist;
            float dist, t_hist, tol;
        } r;
        static_assert(sizeof(Rec) == 20, "a packed record");
        while (fread(&r, sizeof(r), 1, f) == 1) printf("%d\n", tap_accepted(r.s, r.s_hist, r.dist, r.t_hist, r.tol) ? 1 : 0);
    } else {
        struct Rec {
            float pose[16], K[9], o[3], d[3], t;
            uint32_t W, H;
        } r;
        static_assert(sizeof(Rec) == 136, "a packed record");
        while (fread(&r, sizeof(r), 1, f) == 1) {
            const Reprojection rp = reproject_point(prev_camera(r.pose, r.K), r.o, r.d, r.t);
            printf("%08x %08x %08x %08x %08x %d%d%d%d%d", bits(rp.u0), bits(rp.v0), bits(rp.a), bits(rp.b), bits(rp.dist),
                   rp.front ? 1 : 0, tap_inside(rp.u0, r.W) ? 1 : 0, tap_inside(rp.u0 + 1.0f, r.W) ? 1 : 0,
                   tap_inside(rp.v0, r.H) ? 1 : 0, tap_inside(rp.v0 + 1.0f, r.H) ? 1 : 0);
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 2; ++i) printf(" %08x", bits(tap_weight(i, j, rp.a, rp.b)));
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}
