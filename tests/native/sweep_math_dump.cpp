// Prints csrc/rt_sweep_math.h's results (tests/test_sweep_cpu.py).  Floats
// travel as hexadecimal bit patterns, f32 in 8 digits.
//   best rays radii spheres flags -> per cast one line: ok (0 | 1), then the
//         header's answer over EVERY sphere (sweep_cast_ok, sweep_isect; the
//         smallest (t, index); flags: 1 entry only, 2 skip self): t bits,
//         sphere index; a miss: the cast's tmax bits, ffffffff
//   descend depth rmin[3] rmax[3] root_is_leaf noslack nodes prim_idx rays radii want
//         -> per cast one line: reached (0 | 1), node records read.  The tree
//         (nodes: n x {x, y} u32 in the product's record layout, prim_idx:
//         u32 per leaf reference) is descended as rt_sweep.hip descends it,
//         by the header's grown-cell test (sweep_guide, sweep_slab,
//         sweep_meets) in the grid coordinates of a depth-`depth` octree over
//         that root box, scale = G / (rmax - rmin) in f32 as the host sets it,
//         with the FIXED bound want[i].t: reached = some visited leaf lists
//         want[i].sphere.  want: n x {bound bits, sphere index} u32.
//         noslack = 1: the per-cast and the scene's slack are zero.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../raytracingstudy_amd/csrc/rt_sweep_math.h"

namespace {
int g_argc;
char** g_argv;
int g_next = 2;

const char* arg() {
    if (g_next >= g_argc) {
        fprintf(stderr, "sweep_math_dump: too few arguments\n");
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
uint32_t bits(float f) {
    uint32_t b;
    memcpy(&b, &f, sizeof(b));
    return b;
}
template <typename T>
std::vector<T> words(const char* path, size_t per) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "sweep_math_dump: cannot open %s\n", path);
        exit(2);
    }
    std::vector<T> v;
    std::vector<T> rec(per);
    while (fread(rec.data(), sizeof(T), per, f) == per) v.insert(v.end(), rec.begin(), rec.end());
    fclose(f);
    return v;
}

struct Tree {
    std::vector<uint32_t> nodes, prim_idx;
    uint32_t depth;
};

// rt_sweep.hip's descent with a bound that stays: every child whose grown cell
// the segment meets is read
struct Descent {
    const Tree& tr;
    const rtamd::SweepGuide& sg;
    float tmin, bound;
    uint32_t want;
    bool reached = false;
    unsigned long nodes = 0;
    void leaf(uint32_t off, uint32_t cnt) {
        for (uint32_t j = 0; j < cnt; ++j) reached = reached || tr.prim_idx.at(off + j) == want;
    }
    void node(uint32_t x, uint32_t y, uint32_t l0, uint32_t l1, uint32_t l2, uint32_t size) {
        const uint32_t half = size >> 1, l[3] = {l0, l1, l2}, valid = y & 0xFFu, leafm = (y >> 8) & 0xFFu;
        rtamd::SweepSlab s[3][2];
        for (int i = 0; i < 3; ++i) {
            s[i][0] = rtamd::sweep_slab(sg, i, static_cast<float>(l[i]), static_cast<float>(l[i] + half));
            s[i][1] = rtamd::sweep_slab(sg, i, static_cast<float>(l[i] + half), static_cast<float>(l[i] + size));
        }
        uint32_t slot = x;
        for (uint32_t c = 0; c < 8; ++c) {
            if (!(valid & (1u << c))) continue;
            const uint32_t at = slot++;
            if (!rtamd::sweep_meets(s[0][c & 1], s[1][(c >> 1) & 1], s[2][(c >> 2) & 1], tmin, bound)) continue;
            nodes += 1;
            const uint32_t rx = tr.nodes.at(2 * at), ry = tr.nodes.at(2 * at + 1);
            if (leafm & (1u << c)) leaf(rx, ry);
            else node(rx, ry, l0 + ((c & 1) ? half : 0), l1 + ((c & 2) ? half : 0), l2 + ((c & 4) ? half : 0), half);
        }
    }
};
}  // namespace

int main(int argc, char** argv) {
    g_argc = argc;
    g_argv = argv;
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "best") {
        const std::vector<float> rays = words<float>(arg(), 8);
        const std::vector<float> radii = words<float>(arg(), 1);
        const std::vector<float> s = words<float>(arg(), 4);
        const unsigned long flags = strtoul(arg(), nullptr, 10);
        const size_t n = rays.size() / 8;
        if (radii.size() != n) {
            fprintf(stderr, "sweep_math_dump: one radius per ray\n");
            return 2;
        }
        for (size_t i = 0; i < n; ++i) {
            const float* r = &rays[8 * i];
            const bool ok = rtamd::sweep_cast_ok(r[0], r[1], r[2], r[4], r[5], r[6], radii[i]);
            float best_t = r[7];
            uint32_t best = 0xFFFFFFFFu;
            for (size_t j = 0; ok && 4 * j + 3 < s.size(); ++j) {
                if ((flags & 2) && j == i) continue;
                float t;
                if (rtamd::sweep_isect(r[0], r[1], r[2], r[4], r[5], r[6], s[4 * j], s[4 * j + 1], s[4 * j + 2],
                                       s[4 * j + 3], radii[i], r[3], r[7], (flags & 1) != 0, t) &&
                    (best == 0xFFFFFFFFu || t < best_t)) {
                    best_t = t;
                    best = static_cast<uint32_t>(j);
                }
            }
            printf("%d %08x %08x\n", ok ? 1 : 0, bits(best_t), best);
        }
        return 0;
    }
    if (cmd == "descend") {
        Tree tr;
        tr.depth = static_cast<uint32_t>(strtoul(arg(), nullptr, 10));
        if (tr.depth > 16u) {
            fprintf(stderr, "sweep_math_dump: depth over 16\n");
            return 2;
        }
        float rmin[3], rmax[3], scale[3];
        for (float& x : rmin) x = f32();
        for (float& x : rmax) x = f32();
        const bool root_is_leaf = strtoul(arg(), nullptr, 10) != 0;
        const bool noslack = strtoul(arg(), nullptr, 10) != 0;
        tr.nodes = words<uint32_t>(arg(), 2);
        tr.prim_idx = words<uint32_t>(arg(), 1);
        const std::vector<float> rays = words<float>(arg(), 8);
        const std::vector<float> radii = words<float>(arg(), 1);
        const std::vector<uint32_t> want = words<uint32_t>(arg(), 2);
        const size_t n = rays.size() / 8;
        if (radii.size() != n || want.size() != 2 * n || tr.nodes.size() < 2) {
            fprintf(stderr, "sweep_math_dump: one radius and one {bound, sphere} per ray, a root record\n");
            return 2;
        }
        const float G = static_cast<float>(1u << tr.depth);
        for (int i = 0; i < 3; ++i) scale[i] = G / (rmax[i] - rmin[i]);
        const float slack_m = rtamd::sweep_slack_m(rmin, rmax);
        for (size_t i = 0; i < n; ++i) {
            const float* r = &rays[8 * i];
            float bound;
            memcpy(&bound, &want[2 * i], sizeof(bound));
            const float slack = noslack ? 0.0f : rtamd::sweep_slack_o(r[0], r[1], r[2]) + slack_m;
            const rtamd::SweepGuide sg =
                rtamd::sweep_guide(r[0], r[1], r[2], r[4], r[5], r[6], radii[i], rmin, scale, slack);
            Descent d{tr, sg, r[3], bound, want[2 * i + 1]};
            if (rtamd::sweep_meets(rtamd::sweep_slab(sg, 0, 0.0f, G), rtamd::sweep_slab(sg, 1, 0.0f, G),
                                   rtamd::sweep_slab(sg, 2, 0.0f, G), r[3], bound)) {
                d.nodes += 1;
                if (root_is_leaf) d.leaf(tr.nodes[0], tr.nodes[1]);
                else d.node(tr.nodes[0], tr.nodes[1], 0, 0, 0, 1u << tr.depth);
            }
            printf("%d %lu\n", d.reached ? 1 : 0, d.nodes);
        }
        return 0;
    }
    fprintf(stderr, "sweep_math_dump: unknown command\n");
    return 2;
}
