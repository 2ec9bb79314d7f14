// rt_bins_math.h — the screen-space bins' per-sphere arithmetic (DESIGN.md 5.1
// round 10) and the host's build policy, free of HIP and of the renderer's
// state: plain arrays and integers in and out, f64 operations in a fixed order
// (built with -ffp-contract=off like the rest).  screen_bins.hip runs the
// arithmetic per sphere on the device, rt_bins_host.cpp the policy per frame, and
// tests/native/bins_math_dump.cpp prints both for tests/test_bins_cpu.py on the CPU.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_BINS_HD __host__ __device__
#else
#define RT_BINS_HD
#endif

namespace rtamd {

// Bin side: 2^kBinShift pixels.  Every wave tile (1x1 .. 8x8 pixels, aligned)
// lies in one bin, so a wave reads one list whatever the spp.
constexpr uint32_t kBinShift = 3;
constexpr uint32_t kBinSide = 1u << kBinShift;
// A bin with more entries than this walks (its header count is kBinWalk): one
// wave sorts a list, a lane an entry.
constexpr uint32_t kBinCap = 64;
constexpr uint32_t kBinWalk = 0xFFFFFFFFu;
// The frame-level list of spheres every pixel tests (camera inside, or the
// sphere straddles the camera plane); more of them: the frame walks.
constexpr uint32_t kBinWideCap = 32;
// A frame whose non-empty bins hold more than this many entries on average
// walks (a device-side rule, screen_bins.hip: bins_decide_kernel): past it
// most bins are over kBinCap anyway and the fill is work for nothing.
constexpr uint32_t kBinMeanMax = 48;
// After a frame the rule above sent walking, the next kBinDenseSkip plain
// frames build no bins at all (they run the instances without them), then one
// probes again: a dense scene pays the count pass once in 16 frames (C5: 0.65
// ms a frame otherwise, profiles/r10).  Read from the pinned info words
// without a sync; whatever it decides, a frame's pixels are the same.
constexpr uint32_t kBinDenseSkip = 15;
// Frames of fewer primary samples than this walk: the build is seven short
// launches (75 us on C2's 1,000 spheres), more than such a frame's whole
// kernel (C2, 2.07 M samples: 0.093 ms walking, 0.170 ms with bins).
constexpr uint64_t kBinMinSamples = 1ull << 22;

// Slack of the rectangle and the near bound.  A ray
// isect accepts passes within r (1 + 2.5 u) + 20 u D of the centre, D = |c - o|
// (isect's b, q and h roundings: 8 u D; the f32 ray direction against the
// exact pinhole ray through the sample: 12 u D), and a pose whose rotation is
// orthonormal to 2^-20 (the host's gate, bins_camera_ok) moves the centre's
// camera coordinates by at most 2 * 2^-20 D.  r'' = r (1 + 1e-6) + 2^-17 D
// holds both: 2^-17 = 64 u + 4 * 2^-20.
constexpr double kBinSlackDist = 1.0 / 131072.0;
// the sample's image coordinate x + jitter is rounded to f32: at most
// 2^-24 * 32768 pixels, and (u - K2) / K0 adds 2 u relative; 1/64 pixel and
// 1e-6 relative hold both
constexpr double kBinSlackPix = 1.0 / 64.0;
constexpr double kBinSlackPixRel = 1e-6;
constexpr double kBinOrthoGate = 1.0 / 1048576.0;  // 2^-20

enum BinClass : uint32_t { kBinDropped = 0, kBinBinned = 1, kBinWide = 2 };

struct BinRect {
    uint32_t cls;            // BinClass
    uint32_t x0, y0, x1, y1; // pixels, inclusive, clipped to the image (binned only)
    float near_t;            // a lower bound on every t isect can accept (>= 0)
};

// Whether a frame of this camera may use bins: K's focal terms finite and
// non-zero and R orthonormal to kBinOrthoGate (the slack above assumes it).
RT_BINS_HD inline bool bins_camera_ok(const float K[9], const float R[9], const float o[3]) {
    for (int i = 0; i < 3; ++i)
        if (!isfinite(static_cast<double>(o[i]))) return false;
    const double k0 = K[0], k4 = K[4], k2 = K[2], k5 = K[5];
    if (!isfinite(k0) || !isfinite(k4) || !isfinite(k2) || !isfinite(k5) || k0 == 0.0 || k4 == 0.0) return false;
    for (int a = 0; a < 3; ++a)
        for (int b = a; b < 3; ++b) {
            double s = 0.0;
            for (int i = 0; i < 3; ++i) s += static_cast<double>(R[3 * a + i]) * R[3 * b + i];
            if (!(fabs(s - (a == b ? 1.0 : 0.0)) <= kBinOrthoGate)) return false;
        }
    return true;
}

// The pixels whose samples may meet sphere sp = {cx, cy, cz, r} (radius scaled
// by `shrink`: 1 in the product, 0.9 under the negative-control test hook) for
// the camera getRay uses (K[c*3+r], R = mat3(pose) column-major, origin o) on
// a W x H image, and the near bound.
//  * camera coordinates {X, Y, Z} = R^T (c - o): a sample's ray is along
//    {dx, dy, 1} there, dx = (u - K[2]) / K[0];
//  * wholly behind the camera plane (Z < -r''): dropped, every ray has z > 0;
//  * the camera within r'' (1 + 1e-4) of the centre, or the sphere reaching
//    the camera plane (Z <= r''), or a non-finite term: wide;
//  * else per axis the tangent lines from the origin to the circle of radius
//    r'' about {X, Z} in that axis' plane bound x / z:
//    (X Z -+ r'' sqrt(X^2 + Z^2 - r''^2)) / (Z^2 - r''^2),
//    mapped to pixels, widened by the slack, floored: pixel x holds samples
//    u in [x, x + 1].
RT_BINS_HD inline BinRect sphere_screen_rect(const float sp[4], const float K[9], const float R[9],
                                             const float o[3], uint32_t W, uint32_t H, double shrink) {
    BinRect out;
    out.cls = kBinWide;
    out.x0 = out.y0 = 0u;
    out.x1 = W ? W - 1u : 0u;
    out.y1 = H ? H - 1u : 0u;
    out.near_t = 0.0f;
    const double vx = static_cast<double>(sp[0]) - o[0], vy = static_cast<double>(sp[1]) - o[1],
                 vz = static_cast<double>(sp[2]) - o[2];
    const double X = static_cast<double>(R[0]) * vx + static_cast<double>(R[1]) * vy + static_cast<double>(R[2]) * vz;
    const double Y = static_cast<double>(R[3]) * vx + static_cast<double>(R[4]) * vy + static_cast<double>(R[5]) * vz;
    const double Z = static_cast<double>(R[6]) * vx + static_cast<double>(R[7]) * vy + static_cast<double>(R[8]) * vz;
    const double dist = sqrt(vx * vx + vy * vy + vz * vz);
    const double rp = static_cast<double>(sp[3]) * shrink * (1.0 + 1e-6) + kBinSlackDist * dist;
    if (!isfinite(dist) || !isfinite(rp) || !(rp >= 0.0)) return out;
    if (Z < -rp) {
        out.cls = kBinDropped;
        return out;
    }
    if (!(dist > rp * 1.0001) || !(Z > rp)) return out;
    const double nb = (dist - rp) * (1.0 - kBinOrthoGate);
    out.near_t = nb > 0.0 ? static_cast<float>(nb) : 0.0f;
    double lo[2], hi[2];
    const double C[2] = {X, Y};
    const double kf[2] = {K[0], K[4]}, kc[2] = {K[2], K[5]};
    const double den = Z * Z - rp * rp;
    for (int a = 0; a < 2; ++a) {
        const double s = rp * sqrt(C[a] * C[a] + den);
        const double p0 = kf[a] * ((C[a] * Z - s) / den) + kc[a];
        const double p1 = kf[a] * ((C[a] * Z + s) / den) + kc[a];
        if (!isfinite(p0) || !isfinite(p1)) return out;
        const double mn = p0 < p1 ? p0 : p1, mx = p0 < p1 ? p1 : p0;
        lo[a] = floor(mn - kBinSlackPix - kBinSlackPixRel * fabs(mn));
        hi[a] = floor(mx + kBinSlackPix + kBinSlackPixRel * fabs(mx));
    }
    const double wmax = static_cast<double>(W) - 1.0, hmax = static_cast<double>(H) - 1.0;
    if (hi[0] < 0.0 || hi[1] < 0.0 || lo[0] > wmax || lo[1] > hmax) {
        out.cls = kBinDropped;
        return out;
    }
    out.cls = kBinBinned;
    out.x0 = static_cast<uint32_t>(lo[0] > 0.0 ? lo[0] : 0.0);
    out.y0 = static_cast<uint32_t>(lo[1] > 0.0 ? lo[1] : 0.0);
    out.x1 = static_cast<uint32_t>(hi[0] < wmax ? hi[0] : wmax);
    out.y1 = static_cast<uint32_t>(hi[1] < hmax ? hi[1] : hmax);
    return out;
}

// ---- tile words ----
// A frame's wave tiles are tw x th pixels (1x1 .. 8x8, powers of two, aligned
// to their size), so a bin holds (8 / tw) * (8 / th) of them.  Every wave tile
// of a non-empty bin within the cap gets one 64-bit word: bit k is set iff the
// bin-local rectangle of the bin's sorted entry k overlaps the tile.  The
// frame kernel visits the set bits only (rt_bins.h).

RT_BINS_HD inline uint32_t bin_tiles_per_bin(uint32_t tw, uint32_t th) {
    return (kBinSide / tw) * (kBinSide / th);
}

// The tile of pixel (x, y) within its bin, row-major; the table's index is
// bin * bin_tiles_per_bin + this.
RT_BINS_HD inline uint32_t bin_tile_index(uint32_t x, uint32_t y, uint32_t tw, uint32_t th) {
    return ((y & (kBinSide - 1u)) / th) * (kBinSide / tw) + (x & (kBinSide - 1u)) / tw;
}

// The same from the sides' logarithms (tw = 1 << ltw, th = 1 << lth), as the
// frame kernel computes it: no division.
RT_BINS_HD inline uint32_t bin_tile_index_log2(uint32_t x, uint32_t y, uint32_t ltw, uint32_t lth) {
    return (((y & (kBinSide - 1u)) >> lth) << (kBinShift - ltw)) + ((x & (kBinSide - 1u)) >> ltw);
}

// Whether an entry's rectangle (x0 | x1 << 4 | y0 << 8 | y1 << 12, bin-local,
// inclusive: BinEntry::rect) holds a pixel of tile `tile` of its bin.
RT_BINS_HD inline bool bin_rect_overlaps_tile(uint32_t rect, uint32_t tile, uint32_t tw, uint32_t th) {
    const uint32_t per_row = kBinSide / tw;
    const uint32_t tx0 = (tile % per_row) * tw, ty0 = (tile / per_row) * th;
    const uint32_t tx1 = tx0 + tw - 1u, ty1 = ty0 + th - 1u;
    return !((rect & 15u) > tx1 || ((rect >> 4) & 15u) < tx0 || ((rect >> 8) & 15u) > ty1 ||
             ((rect >> 12) & 15u) < ty0);
}

// The word of tile `tile` over a list's rectangles in list order (cnt <= 64).
RT_BINS_HD inline uint64_t bin_tile_word(const uint32_t* rects, uint32_t cnt, uint32_t tile, uint32_t tw,
                                         uint32_t th) {
    uint64_t w = 0;
    for (uint32_t k = 0; k < cnt && k < 64u; ++k)
        if (bin_rect_overlaps_tile(rects[k], tile, tw, th)) w |= uint64_t(1) << k;
    return w;
}

// ---- the frame's constants as one word ----
// What every wave tile of a frame needs of the build beside its own bin: the
// fallback flag (as one bit), the wide list's length (<= kBinWideCap) and the
// logarithms of the wave tile's sides (<= kBinShift).  The frame kernel reads
// them once per wave and carries them in one scalar register:
// bit 0 flag != 0, bits 1-6 the wide count, bits 7-8 ltw, bits 9-10 lth.
RT_BINS_HD inline bool bin_consts_fit(uint32_t wide, uint32_t ltw, uint32_t lth) {
    return wide <= kBinWideCap && ltw <= kBinShift && lth <= kBinShift;
}
// (of values that fit; the flag word is any value)
RT_BINS_HD inline uint32_t bin_consts_pack(uint32_t flag, uint32_t wide, uint32_t ltw, uint32_t lth) {
    return (flag ? 1u : 0u) | (wide << 1) | (ltw << 7) | (lth << 9);
}
RT_BINS_HD inline bool bin_consts_flag(uint32_t c) { return (c & 1u) != 0u; }
RT_BINS_HD inline uint32_t bin_consts_wide(uint32_t c) { return (c >> 1) & 63u; }
RT_BINS_HD inline uint32_t bin_consts_ltw(uint32_t c) { return (c >> 7) & 3u; }
RT_BINS_HD inline uint32_t bin_consts_lth(uint32_t c) { return (c >> 9) & 3u; }

// ---- the host's policy (rt_bins_host.cpp screen_bins) ----
// What a frame's build reports: the bin_info words on the device, mirrored to
// the renderer's pinned copy, which the next frames read without a sync.
enum BinInfoWord : uint32_t {
    kBinInfoFlag = 0,   // 0: binned; kBinFlag* bits: the frame walks
    kBinInfoWide,       // spheres in the wide list
    kBinInfoEntries,    // total entries the frame's bins need
    kBinInfoNonEmpty,   // bins with at least one entry
    kBinInfoLongest,    // the longest list
    kBinInfoOver,       // bins over the cap (their pixels walk)
    kBinInfoFrame,      // the frame id the words belong to
    kBinInfoWords = 8
};
// The build's zeroed words are one allocation, cleared by one memset: the
// bins' counts [nb + 1] (the scan's last item is 0), their fill cursors [nb],
// the decide kernel's partial results and arrival counter (round 19), the info
// words.
enum BinDecideWord : uint32_t { kBinDecNonEmpty = 0, kBinDecLongest, kBinDecOver, kBinDecArrived, kBinDecWords };
inline size_t bin_cursor_at(uint32_t nb) { return size_t(nb) + 1u; }
inline size_t bin_decide_at(uint32_t nb) { return 2u * size_t(nb) + 1u; }
inline size_t bin_info_at(uint32_t nb) { return bin_decide_at(nb) + kBinDecWords; }
inline size_t bin_zeroed_words(uint32_t nb) { return bin_info_at(nb) + kBinInfoWords; }

constexpr uint32_t kBinFlagCapacity = 1u;  // the entries do not fit the buffer
constexpr uint32_t kBinFlagWide = 2u;      // the wide list overflowed
constexpr uint32_t kBinFlagDense = 4u;     // mean list length over kBinMeanMax

// The dense-skip cadence (kBinDenseSkip) and what it is counted against.
struct BinCadence {
    uint32_t skip = 0;        // plain frames still to run without a build
    uint64_t gen = 0;         // ... counted for this scene generation
    uint32_t last_frame = 0;  // the id of the last frame that built bins (0: none, or used up below)
};

// Whether this frame builds no bins because the last build found the scene
// too dense: it probes once in kBinDenseSkip + 1 frames.  mirror_frame /
// mirror_flag: the pinned kBinInfoFrame / kBinInfoFlag words, which count
// only when they belong to the last building frame.
inline bool bin_dense_skip_step(BinCadence& c, uint64_t scene_gen, uint32_t mirror_frame,
                                uint32_t mirror_flag) {
    if (c.gen != scene_gen) c.skip = 0, c.gen = scene_gen;
    if (!c.skip && c.last_frame && mirror_frame == c.last_frame && mirror_flag == kBinFlagDense) {
        // (this frame is the first of the kBinDenseSkip skipped ones: the block below counts it)
        c.skip = kBinDenseSkip;
        c.last_frame = 0;  // (this observation is used up: the probe makes the next one)
    }
    if (!c.skip) return false;
    --c.skip;
    return true;
}

// The entries the bin buffer should hold (the caller allocates twice that):
// 6 per sphere to start with (C3 needs 3.1, C5 2.0), a quarter over what the
// last frame that built bins reported when it did not fit, never under half
// the buffer's ent_n records now (two an entry: the buffer never shrinks),
// never over what 32-bit entry offsets reach.
// (capacity_test: RT_TEST_BIN_CAPACITY, a tiny first buffer, so the first frame overflows)
inline size_t bin_entries_wanted(uint32_t capacity_test, uint32_t n_spheres, uint32_t mirror_frame,
                                 uint32_t mirror_flag, uint32_t mirror_entries, uint32_t last_frame,
                                 size_t ent_n) {
    size_t want = capacity_test ? capacity_test : 6ull * n_spheres + 65536ull;
    const size_t grown = static_cast<size_t>(mirror_entries) + mirror_entries / 4u;
    if (last_frame && mirror_frame == last_frame && (mirror_flag & kBinFlagCapacity) && grown > want)
        want = grown;
    if (ent_n / 2 > want) want = ent_n / 2;
    const size_t most = 0x7FFFFFFFull / 4u;
    return want < most ? want : most;
}

}  // namespace rtamd
