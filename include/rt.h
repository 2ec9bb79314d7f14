/*
 * rt.h — C-ABI of the MI355X-native render path (drop-in for the reference's
 * KernelRenderer, randomwons/RayTracingStudy).
 *
 * Plain C: opaque handle, plain pointers and sizes, int status (0 = ok,
 * negative = error).  No HIP, GL or torch types appear in any signature; a HIP
 * stream is passed as `void*` (a hipStream_t), device buffers as `void*`.
 *
 * Every entry point names the reference interface it replaces (file:line is
 * relative to the reference repository root):
 *
 *   reference                                            this ABI
 *   ---------------------------------------------------  ---------------------------
 *   KernelRenderer(cudaGraphicsResource_t,w,h)            rt_create
 *     include/renderer.cuh:29, src/renderer.cu:124-141
 *   ~KernelRenderer()  include/renderer.cuh:28,           rt_destroy
 *     src/renderer.cu:189-198 (leaks device objects)
 *   setPosition(glm::mat4)  include/renderer.cuh:32,      rt_set_pose
 *     src/renderer.cu:111-113, 93-97
 *   setIntrinsic(glm::mat3) include/renderer.cuh:33,      rt_set_intrinsic
 *     src/renderer.cu:115-117, 99-103
 *   resize(int,int) include/renderer.cuh:31,              rt_resize
 *     src/renderer.cu:155-187
 *   setOctree(vec3,vec3,float) include/renderer.cuh:35    rt_set_octree
 *     (declared, never defined: src/renderer.cu:119-121)
 *   (none: Octree::traverse is a stub,                    rt_set_scene
 *     include/octree.h:19-21)
 *   render() include/renderer.cuh:30,                     rt_render
 *     src/renderer.cu:143-153 (raytracing<<<>>> :149)
 *   cudaGraphicsResourceGetMappedPointer + unmap          rt_render(dev_rgba8 = mapped ptr)
 *     src/renderer.cu:145-151
 *   (none: single device)                                 rt_render_tiles / rt_unpack_tiles
 *   (none: single device; SURVEY 8b B2 "device ids",      rt_create_multi / rt_get_multi_info /
 *     8e E1 ncclCommInitAll)                                rt_get_multi_timing
 *   (none: Octree::traverse is a stub,                    rt_trace_rays
 *     include/octree.h:19-21; no ray entry point)
 *   (none: Octree::traverse is a stub; the Displayer's    rt_pick
 *     mouse input selects nothing)
 *   (none: as above; one hit was the most a ray           rt_trace_rays_multi / rt_pick_multi
 *     could report)
 *   (none: one colour per pixel,                          rt_render_gbuffer, rt_render_ao
 *     src/renderer.cu:57-82)                              rt_filter_layer, rt_apply_layer
 *   (none: a hit is lit by one light and a constant       rt_render_indirect, rt_add_layer
 *     term, src/renderer.cu:57-82)
 *   (none: nothing is kept between two frames)            rt_reproject_layer
 *   (none: Octree::traverse is a stub; nothing asks       rt_query_overlaps / rt_overlaps_at
 *     the octree which spheres touch a ball)
 *   (none: as above; nothing asks which spheres are       rt_query_closest / rt_closest_at
 *     nearest to a point)
 *   (none: as above; nothing asks what a moving ball      rt_sweep_spheres / rt_sweep_at /
 *     touches first)                                        rt_pick_thick
 *   (none: no error reporting, all void)                  rt_last_error
 *
 * Threading: one handle per host thread / stream; calls on one handle are not
 * re-entrant.  Ownership: the caller owns every buffer it passes in; the
 * renderer owns its internal device buffers (freed by rt_destroy).
 */
#ifndef RT_AMD_RT_H
#define RT_AMD_RT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 4

typedef struct rt_renderer rt_renderer;

/* status codes */
enum {
    RT_OK = 0,
    RT_E_INVALID = -1,  /* bad argument */
    RT_E_HIP = -2,      /* HIP runtime error (message in rt_last_error) */
    RT_E_NOMEM = -3,    /* host or device allocation failed */
    RT_E_NOSCENE = -4,  /* RT_MODE_SCENE render without rt_set_scene */
    RT_E_STATE = -5     /* call not valid in the current state */
};

/* render modes */
enum {
    /* Byte-exact restatement of the reference kernel `raytracing`
     * (src/renderer.cu:57-82): R = Octree::traverse() = 200, root-box slab test
     * `hit_sphere` (src/renderer.cu:3-55), miss colour from the direction. */
    RT_MODE_COMPAT = 0,
    /* Build-defined octree scene: nearest sphere hit, Lambert + one shadow ray,
     * `spp` jittered samples averaged (DESIGN.md "Scene mode"). */
    RT_MODE_SCENE = 1
};

/* rt_config.flags */
enum {
    RT_FLAG_JITTER = 1u << 0,      /* per-sample sub-pixel jitter (default: on iff spp > 1) */
    RT_FLAG_NO_JITTER = 1u << 1,   /* force jitter off */
    RT_FLAG_RADIANCE = 1u << 2,    /* also keep the float4 mean radiance buffer */
    RT_FLAG_NO_SHADOWS = 1u << 3,  /* skip shadow rays (Lambert without visibility) */
    RT_FLAG_HOST_BUILD = 1u << 4,  /* build the octree on the host (default: on the GPU);
                                      both builders produce the identical tree */
    RT_FLAG_PROGRESSIVE = 1u << 5, /* scene mode: accumulate samples across frames while the
                                      camera, size, scene and tile list stay unchanged; every
                                      frame adds spp samples */
    RT_FLAG_COMPAT_FMA = 1u << 6,  /* compat mode: evaluate getRay (include/camera.h:31-34) with
                                      ONE CANDIDATE of the FMA contraction nvcc's default
                                      -fmad=true may apply to the reference binary; which order
                                      that binary really uses is unpinned here (no nvcc).  Off
                                      (default) = the reference's SOURCE semantics, in source
                                      order */
    /* bits 8..9, test-only: what fills the padding after the last leaf list
     * (DESIGN.md §4): 0 zero spheres (default), 1 NaN spheres, 2 spheres
     * covering the root box.  Images and counters are the same for all three. */
    RT_FLAG_PAD_FILL_SHIFT = 8,
    /* Test-only: rt_create / rt_create_multi honour the RT_TEST_* environment
     * variables (RT_TEST_FAULT fault injection, RT_TEST_CLAIM_DELAY, RT_TEST_OCC_CAP, RT_TEST_OCC_MEAN,
     * RT_TEST_BIN_CAP, RT_TEST_BIN_CAPACITY, RT_TEST_BIN_SHRINK, RT_TEST_BIN_MIN_SAMPLES,
     * RT_TEST_BIN_MEAN)
     * and the A/B switches RT_SORT, RT_LDS_STAGE, RT_LEAF_PACK and RT_SB_ORDER
     * (none changes an image); without this flag they are
     * ignored (a set one is named on stderr once). */
    RT_FLAG_TEST_HOOKS = 1u << 10,
    /* Test-only: before every frame, fill the frame's outputs with a sentinel
     * (RGBA8 bytes 0xAB, frame or packed tiles; radiance and a first
     * progressive frame's sums all-ones bits, a NaN), so a pixel the kernels
     * do not write shows in any readback.  Costs a memset per frame. */
    RT_FLAG_TEST_POISON = 1u << 11,
    /* A/B: no occluder lists, every shadow ray walks the octree (DESIGN.md 5.1
     * round 7).  Images and counters are the same either way.  (Its own bit:
     * the eight RT_FLAG_OPT_SHIFT bits are all taken.) */
    RT_FLAG_NO_OCCLUDERS = 1u << 12,
    /* A/B: no screen-space bins, every primary ray walks the octree (DESIGN.md
     * 5.1 round 10).  Images and counters are the same either way. */
    RT_FLAG_NO_BINS = 1u << 13,
    /* A/B: no pixel pairs: a binned 33..64-spp frame shades one pixel a wave
     * pass, as every other frame does.  Images and
     * counters are the same either way. */
    RT_FLAG_NO_PAIRS = 1u << 14,
    /* bits 16..19: scene-kernel variant for A/B runs (0 = default: 13, the
     * per-wave queue, for spp >= 8, else 7; others in DESIGN.md 5.1); images
     * and counters are identical across variants (packets: images only) */
    RT_FLAG_VARIANT_SHIFT = 16,
    /* bits 20..27: A/B toggles that switch single optimisations off or on (0 = defaults) */
    RT_FLAG_OPT_SHIFT = 20,
    /* bits 28..31: depth of the octree's cell table (DESIGN.md 5.1 "Cell table"):
     * 0 = chosen from the tree (default), 1..7 = that depth (clamped to the
     * tree), 15 = no table.  Images and counters are the same either way. */
    RT_FLAG_CELL_TABLE_SHIFT = 28
};

typedef struct rt_config {
    uint32_t width;        /* framebuffer width  (reference: KernelRenderer::width)  */
    uint32_t height;       /* framebuffer height (reference: KernelRenderer::height) */
    uint32_t spp;          /* samples per pixel (scene mode; compat ignores it: 1)   */
    uint32_t seed;         /* sampling seed (scene mode)                              */
    int32_t device;        /* HIP device ordinal, -1 = the calling thread's current   */
    uint32_t mode;         /* RT_MODE_*                                               */
    uint32_t flags;        /* RT_FLAG_*                                               */
    float light_dir[3];    /* direction the directional light TRAVELS (need not be unit) */
    float ambient;         /* ambient term of the Lambert shade, [0,1]                */
} rt_config;

/* Octree parameters.  Defaults (rt_octree_params_default) are the reference's
 * hard-coded root, src/renderer.cu:134-136: min (0,0,0), max (1.28)^3,
 * resolution 0.01 => max_depth = ceil(log2(1.28/0.01)) = 7. */
typedef struct rt_octree_params {
    float min[3];
    float max[3];
    float resolution;       /* smallest cell edge; used when max_depth == 0            */
    uint32_t max_depth;     /* 0 = derive from resolution; else 1..16                  */
    uint32_t leaf_capacity; /* split a cell while it holds more spheres than this (8) */
} rt_octree_params;

typedef struct rt_stats {
    uint64_t primary_rays;   /* camera rays cast (pixels * spp)                         */
    uint64_t shadow_rays;    /* shadow rays cast (lit-facing primary hits)              */
    uint64_t nodes_visited;  /* octree node records read (DESIGN.md counter definition) */
    uint64_t prims_tested;   /* ray-sphere tests                                        */
    float ms;                /* device time of the render launch(es), hipEvent          */
    uint32_t samples_per_pixel; /* samples in the image: spp, or the accumulated total  */
} rt_stats;

typedef struct rt_scene_info {
    uint32_t n_spheres;
    uint32_t n_nodes;        /* node records (internal + leaf)                          */
    uint32_t n_leaves;
    uint32_t n_prim_refs;    /* total length of all leaf sphere lists                   */
    uint32_t max_depth;      /* depth limit the tree was built with                     */
    uint32_t depth_reached;  /* deepest leaf                                            */
    uint32_t node_bytes;     /* sizeof one node record                                  */
    uint32_t prim_bytes;     /* bytes read per sphere test                              */
    float root_min[3];       /* effective root box: the configured box grown to          */
    float root_max[3];       /*   enclose every sphere (equal to it when none protrudes)  */
    double build_ms;         /* time to a device-resident octree (GPU build, or host
                                build + upload with RT_FLAG_HOST_BUILD)                 */
    double upload_ms;        /* time to place the sphere list in device memory          */
    uint32_t builder;        /* RT_BUILDER_* that built the current tree                */
    uint32_t cell_table_depth; /* K of the depth-K cell table the walk uses, 0 = none   */
    /* Occluder lists: made by the first frame after a
     * scene (or light) change, so all three are 0 until then. */
    double occluder_build_ms;  /* device time of that build; filled at the renderer's next
                                  synchronisation after it (a stats frame, rt_synchronize,
                                  rt_readback), 0 until then                            */
    uint32_t occluder_entries; /* total length of the lists                               */
    uint32_t occluder_lists_on; /* 1: plain frames answer shadow rays from the lists; 0:
                                  every shadow ray walks (scene rule, RT_FLAG_NO_OCCLUDERS).
                                  A frame whose camera is far from the scene (its distance
                                  terms over 3x the root box's farthest corner) walks too */
} rt_scene_info;

enum { RT_BUILDER_DEVICE = 0, RT_BUILDER_HOST = 1 };

/* ---- version / discovery -------------------------------------------------- */
int rt_abi_version(void);
/* Number of visible HIP devices (0 when no GPU); never initialises a context. */
int rt_device_count(void);

/* ---- lifecycle ------------------------------------------------------------ */
void rt_config_default(rt_config* cfg);
void rt_octree_params_default(rt_octree_params* p);
/* Reference ctor: camera K0 = mat3(1000,0,640, 0,1000,340, 0,0,1) and identity
 * pose (src/renderer.cu:84-91), octree root from rt_octree_params_default. */
int rt_create(const rt_config* cfg, rt_renderer** out);
int rt_destroy(rt_renderer* r);

/* ---- camera --------------------------------------------------------------- */
/* pose: glm-style column-major mat4; origin = pose[3].xyz, rot = mat3(pose)
 * (include/camera.h:43-46).  K: column-major mat3, K[0][0]=fx, K[1][1]=fy,
 * K[0][2]=cx, K[1][2]=cy, i.e. K[c*3+r] (include/camera.h:24-26). */
int rt_set_pose(rt_renderer* r, const float pose[16]);
int rt_set_intrinsic(rt_renderer* r, const float K[9]);
int rt_get_camera(const rt_renderer* r, float pose_out[16], float K_out[9]);
/* Reference resize (src/renderer.cu:155-170): f = W/(2 tan(radians(80)/2)),
 * cx = W/2, cy = H/2 (integer division); reallocates internal buffers. */
int rt_resize(rt_renderer* r, uint32_t width, uint32_t height);
/* The intrinsic rt_resize would set, without a renderer (for hosts/tests). */
void rt_resize_intrinsic(uint32_t width, uint32_t height, float K_out[9]);

/* ---- scene ---------------------------------------------------------------- */
/* spheres: 4*n floats (cx, cy, cz, radius); albedo: n packed RGBA8 (R in the low
 * byte) or NULL (every sphere 0.8 grey).  oct == NULL keeps the current octree
 * parameters.  Builds the octree on the host and uploads it. */
int rt_set_scene(rt_renderer* r, const float* spheres, const uint32_t* albedo, uint32_t n,
                 const rt_octree_params* oct);
/* Same, from a sphere list already in device memory (e.g. produced by a
 * simulation on the GPU): dev_spheres = 4*n floats, dev_albedo = n RGBA8 words
 * or NULL.  `stream` (or NULL) is the stream that produced them; the call waits
 * for it.  The octree is built on the GPU unless RT_FLAG_HOST_BUILD is set.
 * Invalid spheres (r <= 0, non-finite values) are found on the device and the
 * call fails with RT_E_INVALID, keeping the previous scene.  SURVEY.md 8f F1;
 * the reference's intended entry is setOctree (include/renderer.cuh:35). */
int rt_set_scene_device(rt_renderer* r, const void* dev_spheres, const void* dev_albedo,
                        uint32_t n, const rt_octree_params* oct, void* stream);
/* Mirror of the reference's setOctree(min, max, resolution): rebuilds the
 * octree of the current spheres with a new root box / resolution. */
int rt_set_octree(rt_renderer* r, const float min[3], const float max[3], float resolution);
int rt_get_scene_info(const rt_renderer* r, rt_scene_info* info);
/* Copy the current octree to host memory (sizes from rt_get_scene_info):
 * nodes_out 2*n_nodes words (uint2 records), prim_sp_out
 * 4*n_prim_refs floats, prim_idx_out n_prim_refs words; any may be NULL. */
int rt_export_octree(rt_renderer* r, uint32_t* nodes_out, float* prim_sp_out,
                     uint32_t* prim_idx_out);
/* Copy the occluder lists to host memory (RT_E_STATE when the scene has none,
 * or before the first frame after a scene change): per sphere offsets_out and
 * counts_out (n_spheres words each; a count of 0xFFFFFFFF: that sphere's
 * shadow rays walk the octree and its list is empty), indices_out the lists'
 * sphere indices (occluder_entries words, nearest-first along the light),
 * prim_occ_out 2*n_prim_refs words: the {offset, count} header of every leaf
 * reference.  Any may be NULL. */
int rt_export_occluders(rt_renderer* r, uint32_t* offsets_out, uint32_t* counts_out,
                        uint32_t* indices_out, uint32_t* prim_occ_out);
/* Screen-space bins: every plain scene frame of the
 * wave queue lists, per 8x8-pixel bin, the spheres its primary rays can meet,
 * and answers those rays from the lists; the lists are rebuilt inside every
 * such frame (the camera may move every frame).  rt_get_bin_info reports the
 * handle's last frame (it waits for the handle's queued work). */
enum {
    RT_BINS_ON = 0,           /* the frame's primary rays were answered from the bins       */
    RT_BINS_OFF_FLAG = 1,     /* RT_FLAG_NO_BINS                                             */
    RT_BINS_OFF_KERNEL = 2,   /* a frame that walks by design: a stats frame, a block-tile
                                 variant, a frame below the size at which bins pay, compat   */
    RT_BINS_OFF_CAMERA = 3,   /* a pose that is not a rotation, or a degenerate intrinsic    */
    RT_BINS_OFF_CAPACITY = 4, /* the entries did not fit the buffer: this frame walked, the
                                 next one gets a larger buffer                               */
    RT_BINS_OFF_WIDE = 5,     /* too many spheres around or beside the camera                */
    RT_BINS_OFF_DENSE = 6,    /* mean list length over the rule's: the frame walked          */
    RT_BINS_NO_FRAME = 7      /* nothing rendered yet                                        */
};
typedef struct rt_bin_info {
    uint32_t enabled;         /* 1: reason == RT_BINS_ON                                     */
    uint32_t reason;          /* RT_BINS_*                                                   */
    uint32_t bin_size;        /* bin side in pixels (8)                                      */
    uint32_t bins;            /* bins of the frame: ceil(W / 8) * ceil(H / 8)                */
    uint32_t entries;         /* total length of the lists (what the frame needed)           */
    uint32_t capacity;        /* entries the buffer held for that frame                      */
    uint32_t non_empty_bins;
    uint32_t longest;         /* the longest list                                            */
    uint32_t overflowed_bins; /* bins over the per-bin cap: their pixels walked              */
    uint32_t wide;            /* spheres in the frame-level list every pixel tests           */
    float bin_build_ms;       /* device time of the frame's bin build; its events are
                                 recorded only from the first rt_get_bin_info call on,
                                 so 0 for frames queued before it                            */
} rt_bin_info;
int rt_get_bin_info(rt_renderer* r, rt_bin_info* info);
/* The switches of the scene-kernel instance that the handle's last scene frame
 * launched (tiles 1, stats 2, progressive 4, wave queue 8,
 * sorted rounds 16, occluder lists 32, bins 64, pixel pairs 128); 0 before the
 * first scene frame.  Does not wait. */
uint32_t rt_last_instance(const rt_renderer* r);
/* Copy the last frame's bins to host memory (sizes from rt_get_bin_info;
 * RT_E_STATE unless that frame built lists): headers_out 2*bins words, bin
 * b = by * ceil(W/8) + bx: {first entry, count}, a count of 0xFFFFFFFF: the
 * bin is over the cap and its pixels walk (its entries are still there, up to
 * the next bin's first entry); indices_out `entries` sphere indices;
 * wide_out `wide` sphere indices.  Any may be NULL. */
int rt_export_bins(rt_renderer* r, uint32_t* headers_out, uint32_t* indices_out, uint32_t* wide_out);
/* The last frame's tile words, under rt_export_bins'
 * state rules: that frame's wave tile is *tw x *th pixels (1x1 at 64 spp and
 * more, up to 8x8 at 1 spp), a bin holds *tiles_per_bin = (8 / tw) * (8 / th)
 * of them, and words_out[b * tiles_per_bin + ((y & 7) / th) * (8 / tw) +
 * (x & 7) / tw] is the word of the wave tile that holds pixel (x, y) of bin b:
 * bit k is set iff the bin's entry k (rt_export_bins' order) may be met by a
 * sample of that tile; the frame's kernel tests those entries only.  The
 * words of an empty bin and of a bin over the cap are 0.  words_out: bins *
 * tiles_per_bin words, or NULL for the three sizes alone (any may be NULL). */
int rt_export_bin_tiles(rt_renderer* r, uint32_t* tw, uint32_t* th, uint32_t* tiles_per_bin,
                        uint64_t* words_out);
/* Synthetic scene generator: splitmix64 -> PCG32 from `seed`;
 * centres U[0,1.28)^3, radius 0.02*(1000/n)^(1/3)*U[0.5,1), albedo U[0.2,1). */
int rt_generate_spheres(uint32_t n, uint32_t seed, float* spheres_out, uint32_t* albedo_out);

/* ---- scene files (binary sphere list) --------------------- */
/* Write n spheres (4 floats each) and, if albedo != NULL, their RGBA8 words. */
int rt_save_spheres(const char* path, const float* spheres, const uint32_t* albedo, uint32_t n);
/* Read a sphere file.  *n_out = its sphere count; with spheres_out == NULL only
 * the count is returned.  Otherwise capacity must be >= the count; albedo_out
 * (may be NULL) gets the file's colours or 0.8 grey when it has none. */
int rt_load_spheres(const char* path, float* spheres_out, uint32_t* albedo_out,
                    uint32_t capacity, uint32_t* n_out);

/* ---- render --------------------------------------------------------------- */
/* Render one frame.  dev_rgba8: W*H*4 device bytes (e.g. the pointer a GL PBO
 * maps to), or NULL to render into the renderer's internal framebuffer.
 * stream: a hipStream_t or NULL (the renderer's own stream).  Asynchronous
 * unless stats != NULL (then it waits for the frame and fills the counters).
 * An earlier frame that the kernel found incomplete (its work queue's bounded
 * wait gave up: a broken invariant, never a normal frame) is reported by the
 * first call that sees it, without a sync: this rt_render returns RT_E_HIP
 * naming that frame and renders nothing, so a caller that never reads back
 * (the reference's Displayer, src/window/displayer.cpp:51-53) still learns
 * of it; rt_synchronize, rt_readback and stats frames report it too. */
int rt_render(rt_renderer* r, void* dev_rgba8, void* stream, rt_stats* stats);
/* GL interop.  The Displayer registers its PBO with
 * hipGraphicsGLRegisterBuffer (where it called cudaGraphicsGLRegisterBuffer,
 * src/window/displayer.cpp:13-17, and again after a resize, :61-70) and binds
 * the resource here.  Then rt_render(r, NULL, stream, stats) maps it, renders
 * into the mapped pointer and unmaps it: the reference's render()
 * (src/renderer.cu:145-151).  NULL unbinds (render into the internal
 * framebuffer).  The resource stays owned by the caller. */
int rt_bind_graphics_resource(rt_renderer* r, void* hip_graphics_resource);
/* The same per-frame map -> render -> unmap cycle for a display buffer the
 * caller's toolkit owns (a GL PBO, Vulkan/EGL external memory, a swap-chain
 * image): rt_render(r, NULL, stream, stats) calls ops->map(user, stream, &ptr,
 * &bytes) on the frame's stream, fails with RT_E_INVALID (after unmapping) if
 * bytes < W*H*4, renders into ptr and calls ops->unmap(user, stream) after
 * the launch, also when the render itself failed.  map/unmap return 0 on
 * success; a failing map must leave the buffer unmapped, and rt_render then
 * returns RT_E_HIP.  rt_bind_graphics_resource(r, res) is this call with the
 * built-in HIP graphics-interop ops (hipGraphicsMapResources, ...GetMappedPointer,
 * hipGraphicsUnmapResources) and user = res.  ops == NULL unbinds; *ops is
 * copied.  SURVEY.md 8f F2; replaces src/renderer.cu:145-151. */
typedef struct rt_display_ops {
    int (*map)(void* user, void* stream, void** dev_ptr, size_t* bytes);
    int (*unmap)(void* user, void* stream);
} rt_display_ops;
int rt_bind_display(rt_renderer* r, const rt_display_ops* ops, void* user);
/* Render only the listed image tiles (tile_size x tile_size, row-major tile
 * ids over ceil(W/ts) x ceil(H/ts)) into a packed device buffer of
 * n_tiles*ts*ts*4 bytes: tile k's pixel (lx,ly) at byte 4*(k*ts*ts + ly*ts + lx);
 * pixels outside the image are written as 0.  Used to shard a frame over GPUs. */
int rt_render_tiles(rt_renderer* r, const uint32_t* tile_ids, uint32_t n_tiles,
                    uint32_t tile_size, void* dev_packed_rgba8, void* stream, rt_stats* stats);
/* Scatter a packed tile buffer (layout above) into a W*H*4 device image.
 * A tile id of RT_TILE_SKIP marks a padding slot that is not copied, so the
 * equal-size slabs of all ranks, gathered into one buffer, unpack in one call. */
#define RT_TILE_SKIP 0xFFFFFFFFu
int rt_unpack_tiles(rt_renderer* r, const void* dev_packed_rgba8, const uint32_t* tile_ids,
                    uint32_t n_tiles, uint32_t tile_size, void* dev_rgba8, void* stream);
/* RT_FLAG_PROGRESSIVE: start the next frame from zero samples (any change of
 * pose, intrinsic, size, scene or tile list does this by itself; setting the
 * same pose again, as the reference's Displayer does every frame, does not). */
int rt_reset_accumulation(rt_renderer* r);
/* Wait for all work queued by this renderer, on its own stream or on the
 * caller streams passed to rt_render / rt_render_tiles / rt_unpack_tiles.
 * (Work queued on a stream other than the previous call's is ordered after
 * that previous call's work: the renderer's counters and buffers are shared.) */
int rt_synchronize(rt_renderer* r);
/* Copy the internal framebuffer (and the float4 radiance buffer when
 * RT_FLAG_RADIANCE is set) to host memory; either pointer may be NULL.
 * Waits for the renderer's queued work first, whatever stream it is on. */
int rt_readback(rt_renderer* r, uint8_t* host_rgba8, float* host_rgba32f);
/* Device pointer of the internal framebuffer (W*H*4 bytes). */
void* rt_framebuffer(rt_renderer* r);
/* The renderer's own stream (a hipStream_t made with the handle), the one a
 * NULL stream argument means (a multi-device handle: its output stream on
 * devices[0]).  Extension: the reference launches on the legacy
 * default stream (src/renderer.cu:149).  Renderers made one after another get
 * streams on different hardware queues, so frames in flight on them overlap. */
void* rt_stream(rt_renderer* r);

/* ---- ray queries ---------------------------------------------------------- */
/* Batch ray queries against the scene octree, outside any frame: picking,
 * line-of-sight and collision tests, lidar-style sweeps, a custom integrator's
 * secondary rays.  The reference has no counterpart (Octree::traverse is a
 * stub, include/octree.h:19-21).
 * A ray is origin + t * dir; `dir` is used as given (the caller normalises it
 * if t is to be a distance).  A sphere is hit iff its nearest root t with
 * tmin < t < tmax exists (the frames' own intersection test). */
typedef struct rt_ray {
    float origin[3];
    float tmin;
    float dir[3];
    float tmax;
} rt_ray; /* 32 bytes */
typedef struct rt_hit {
    float t;         /* the hit's t; a miss: the ray's tmax                        */
    uint32_t sphere; /* index into the caller's sphere list; a miss: RT_NO_HIT     */
} rt_hit; /* 8 bytes */
#define RT_NO_HIT 0xFFFFFFFFu
enum {
    RT_QUERY_NEAREST = 0, /* smallest t, then smallest sphere index                */
    RT_QUERY_ANY = 1      /* the first accepted sphere in the walk's cell order and
                             each leaf's list order (an occlusion test)            */
};
/* Trace n rays (dev_rays: n rt_ray in device memory) and write n rt_hit to
 * dev_hits (device memory).  stream: a hipStream_t or NULL (the renderer's
 * own); asynchronous unless stats != NULL, and ordered after the handle's
 * earlier work, like rt_render.  With stats: primary_rays = n (nearest) or
 * shadow_rays = n (any), nodes_visited / prims_tested summed over the rays,
 * ms = device time of the launch.  n == 0: RT_OK, nothing launched.  No scene:
 * RT_E_NOSCENE.  Unknown kind, or a NULL buffer with n > 0: RT_E_INVALID.
 * Rays with a NaN or infinite component miss.  A query reads scene state only:
 * it never changes a frame (progressive accumulation, counters, the next
 * frame's image).  A multi-device handle answers from devices[0]. */
int rt_trace_rays(rt_renderer* r, const void* dev_rays, uint32_t n, uint32_t kind, void* dev_hits,
                  void* stream, rt_stats* stats);
/* The nearest sphere under image coordinates (u, v) of the current camera
 * (pixel (x, y)'s centre ray is u = x, v = y, as the frames cast it):
 * Camera::getRay (include/camera.h:24-41) with tmin = 0, tmax = +inf.  Waits
 * for the answer.  hit_out as above; point_out (may be NULL) = origin + t * dir.
 * The Displayer's mouse position goes here. */
int rt_pick(rt_renderer* r, float u, float v, rt_hit* hit_out, float point_out[3]);

/* Ordered multi-hit queries: the k nearest spheres along each ray (click-through
 * picking, several lidar returns per beam, an integrator's ordered surface
 * list).  For one ray the accepted set is every scene sphere whose t (the
 * intersection test above: the near root, or the far root when the near one is
 * not past tmin) lies in tmin < t < tmax; each sphere counts once.  The answer
 * is the k smallest of the set by (t ascending, then sphere index ascending):
 * RT_QUERY_NEAREST's tie rule extended, and for k = 1 its answer exactly.
 *   dev_hits    n*k rt_hit, ray-major: ray i's hits at [i*k, i*k + k) in that
 *               order; slots past the ray's count hold {the ray's tmax,
 *               RT_NO_HIT}.  Every slot of every ray is written.
 *   dev_counts  n uint32 or NULL: min(k, size of the accepted set).
 * stream, ordering and stats as rt_trace_rays: primary_rays = n, nodes_visited
 * / prims_tested the walk's own counts summed over the rays (for k = 1 the
 * nearest query's; the walk runs with k rounded up to 1, 2, 4, 8 or 16).
 * k == 0 or k > RT_MULTIHIT_MAX: RT_E_INVALID.  n == 0: RT_OK, nothing
 * launched.  A NULL dev_rays / dev_hits with n > 0: RT_E_INVALID.  No scene:
 * RT_E_NOSCENE.  Rays with a NaN or infinite component have an empty set.
 * Reads scene state only; a multi-device handle answers from devices[0]. */
#define RT_MULTIHIT_MAX 16
int rt_trace_rays_multi(rt_renderer* r, const void* dev_rays, uint32_t n, uint32_t k,
                        void* dev_hits, void* dev_counts, void* stream, rt_stats* stats);
/* rt_pick's ray (Camera::getRay, tmin = 0, tmax = +inf) as a 1-ray multi-hit
 * query; waits for the answer.  hits_out has room for k rt_hit, filled as
 * dev_hits above; count_out (may be NULL) as dev_counts.  The Displayer's
 * repeated click on one spot walks down this list. */
int rt_pick_multi(rt_renderer* r, float u, float v, uint32_t k, rt_hit* hits_out, uint32_t* count_out);

/* ---- sphere-overlap queries ------------------------------------------------ */
/* Which scene spheres touch this ball: the contacts of a simulation's spheres
 * after a step, the Displayer's brush selection ("everything within 5 cm of the
 * picked point"), point containment (radius 0).  The reference has no
 * counterpart (Octree::traverse is a stub, include/octree.h:19-21).
 * For one probe (p, R) the accepted set is every scene sphere (c, r) with
 * d2 <= s * s, where dx = p.x - c.x (likewise dy, dz), d2 = (dx*dx + dy*dy) +
 * dz*dz and s = R + r: all f32, in that order, no contraction.  The test is
 * closed (tangent spheres touch); R = 0 is point containment; a probe with a
 * non-finite component or R < 0 has an empty set; each sphere counts once,
 * however many octree leaves list it.
 *   dev_probes   n rt_probe in device memory.
 *   dev_indices  n*k uint32, probe-major: probe i's slots [i*k, i*k + k) hold
 *                the k smallest sphere indices of its set, ascending; slots
 *                past those hold RT_NO_HIT.  Every slot is written.
 *   dev_counts   n uint32 or NULL: min(k, size of the set), with
 *                RT_OVERLAP_MORE OR-ed in iff the set is larger than k (exact).
 * flags: RT_OVERLAP_SKIP_SELF leaves sphere index i out of probe i's set (a
 * probe with i >= n_spheres skips nothing): as rt_probe has a scene sphere's
 * layout, the scene's own device sphere list as the probes with this flag is
 * "all contacts of the scene".
 * stream, ordering and stats as rt_trace_rays: asynchronous unless stats !=
 * NULL, ordered after the handle's earlier work; primary_rays = shadow_rays =
 * 0, nodes_visited = node records the query read, prims_tested = predicate
 * evaluations, ms = device time of the launch.  k == 0, k > RT_OVERLAP_MAX,
 * unknown flag bits, or a NULL dev_probes / dev_indices with n > 0:
 * RT_E_INVALID.  n == 0: RT_OK, nothing launched.  No scene: RT_E_NOSCENE.
 * Reads scene state only: it never changes a frame; a multi-device handle
 * answers from devices[0]. */
typedef struct rt_probe {
    float center[3];
    float radius;
} rt_probe; /* 16 bytes: the layout of a scene sphere */
#define RT_OVERLAP_MAX 16
#define RT_OVERLAP_MORE 0x80000000u /* in a count word: the accepted set is larger than k */
enum { RT_OVERLAP_SKIP_SELF = 1u }; /* probe i does not report sphere index i */
int rt_query_overlaps(rt_renderer* r, const void* dev_probes, uint32_t n, uint32_t k, uint32_t flags,
                      void* dev_indices, void* dev_counts, void* stream, rt_stats* stats);
/* A one-probe query that waits for the answer, like rt_pick.  indices_out has
 * room for k uint32, filled as dev_indices above; count_out (may be NULL) as
 * dev_counts.  The point rt_pick returns goes here for a brush selection
 * (INTEGRATION.md). */
int rt_overlaps_at(rt_renderer* r, const float center[3], float radius, uint32_t k,
                   uint32_t* indices_out, uint32_t* count_out);

/* ---- closest-sphere queries ------------------------------------------------ */
/* Which scene spheres are nearest to this point, and how far away their
 * surfaces are: a click that missed (rt_pick returned RT_NO_HIT) snapping to
 * the nearest sphere, clearances before there is contact, each sphere's k
 * nearest neighbours, the distance to the nearest surface at many points.  The
 * reference has no counterpart (Octree::traverse is a stub,
 * include/octree.h:19-21).
 * A query is an rt_probe: `center` is the point p, `radius` the search radius
 * R, the largest surface distance of interest.  For scene sphere (c, r):
 * dx = p.x - c.x (likewise dy, dz), d2 = (dx*dx + dy*dy) + dz*dz, key =
 * sqrtf(d2) - r: all f32, in that order, no contraction, sqrtf correctly
 * rounded.  key is the signed distance from p to the sphere's surface,
 * negative inside the sphere.  The accepted set is every scene sphere with
 * key <= R (closed).  R = +inf is allowed: the unbounded nearest neighbour.
 * R = -0 is 0.  A probe with a non-finite centre component, a NaN R or R < 0
 * has an empty set.  Each sphere counts once, however many octree leaves list
 * it.  This is not rt_query_overlaps' set: its d2 <= (R + r)^2 rounds
 * differently, so a sphere at the very edge may be in one and not the other.
 * The answer is the k smallest members by (key ascending, then sphere index
 * ascending), 1 <= k <= RT_CLOSEST_MAX.
 *   dev_probes  n rt_probe in device memory.
 *   dev_near    n*k rt_near, probe-major: probe i's slots [i*k, i*k + k) hold
 *               its answer in that order; slots past the probe's count hold
 *               {the probe's radius as given, RT_NO_HIT} (multi-hit's tmax
 *               convention).  Every slot is written.
 *   dev_counts  n uint32 or NULL: min(k, size of the set).  There is no "more"
 *               bit: the search stops looking beyond the k-th distance, and
 *               with it gives up knowing whether the set is larger.
 * flags: RT_CLOSEST_SKIP_SELF leaves sphere index i out of probe i's set (a
 * probe with i >= n_spheres skips nothing): the scene's own device sphere list
 * as the probes with this flag is "each sphere's k nearest neighbours" (the
 * fourth component is then the search radius).
 * stream, ordering, stats and error codes as rt_query_overlaps: asynchronous
 * unless stats != NULL, ordered after the handle's earlier work; primary_rays
 * = shadow_rays = 0, nodes_visited = node records the query read,
 * prims_tested = key evaluations, ms = device time of the launch.  k == 0,
 * k > RT_CLOSEST_MAX, unknown flag bits, or a NULL dev_probes / dev_near with
 * n > 0: RT_E_INVALID.  n == 0: RT_OK, nothing launched.  No scene:
 * RT_E_NOSCENE.  Reads scene state only: it never changes a frame; a
 * multi-device handle answers from devices[0]. */
typedef struct rt_near {
    float dist;      /* the key: signed distance to the sphere's surface          */
    uint32_t sphere; /* index into the caller's sphere list; a free slot: RT_NO_HIT */
} rt_near; /* 8 bytes */
#define RT_CLOSEST_MAX 16
enum { RT_CLOSEST_SKIP_SELF = 1u }; /* probe i leaves sphere index i out */
int rt_query_closest(rt_renderer* r, const void* dev_probes, uint32_t n, uint32_t k, uint32_t flags,
                     void* dev_near, void* dev_counts, void* stream, rt_stats* stats);
/* A one-probe query that waits for the answer, like rt_overlaps_at.  near_out
 * has room for k rt_near, filled as dev_near above (free slots hold max_dist);
 * count_out (may be NULL) as dev_counts.  A point along rt_pick's ray, or the
 * camera's focus, goes here to snap a missed click to the nearest sphere
 * (INTEGRATION.md). */
int rt_closest_at(rt_renderer* r, const float point[3], float max_dist, uint32_t k,
                  rt_near* near_out, uint32_t* count_out);

/* ---- swept-sphere queries --------------------------------------------------- */
/* The first scene sphere a moving ball touches: a simulation's time of impact
 * (continuous collision detection), a character or probe of finite size moved
 * through the scene, a lidar beam with width, a cursor of finite radius that
 * hits the spheres rt_pick's thin ray misses.  The reference has no counterpart
 * (Octree::traverse is a stub, include/octree.h:19-21).
 * A cast is an rt_ray plus a radius R: a ball of radius R has its centre at
 * origin + t * dir.  For scene sphere (c, r), s = r + R is one f32 add, and the
 * test is rt_trace_rays' own intersection test against the sphere (c, s): the
 * same operations in the same order, the same window tmin < t < tmax, the same
 * fall-through to the far root when the near root is not past tmin.  The
 * answer is the smallest t, then the smallest sphere index (RT_QUERY_NEAREST's
 * rule), as an rt_hit; a miss is {the cast's tmax, RT_NO_HIT}.  As r + 0.0f is
 * r, a valid cast with R = 0 answers exactly as rt_trace_rays(...,
 * RT_QUERY_NEAREST), bit for bit.
 * Validity: a cast with a NaN or infinite origin or direction component misses,
 * as in rt_trace_rays; so does one whose R is not finite or is < 0 (R = -0 is
 * 0).  Unlike rt_trace_rays, `dir` has to be of unit length, as R is in world
 * units and t therefore has to be: a cast with
 * |((dx*dx + dy*dy) + dz*dz) - 1| > 2^-18, computed in f32 in that order,
 * misses too.  A direction normalised in f32 (each component divided by the
 * f32 length) passes: it is within 2^-22 of unit length.
 * flags:
 *   RT_SWEEP_ENTRY_ONLY  only the near root counts: a sphere the ball already
 *       touches at tmin (its near root is not past tmin) is not reported; those
 *       spheres are rt_query_overlaps' answer.  Without the flag the ray rule
 *       holds and the far root is reported, like a camera inside a sphere.
 *   RT_SWEEP_SKIP_SELF   cast i leaves sphere index i out (a cast with i >=
 *       n_spheres skips nothing): the scene's centres as origins, its radii as
 *       R and a step's velocities as directions give each sphere's first impact
 *       of that step.
 *   dev_rays   n rt_ray in device memory.
 *   dev_radii  n floats in device memory, cast i's R; NULL: every cast uses
 *              `radius`.
 *   dev_hits   n rt_hit in device memory; every one is written.
 * stream, ordering, stats and error codes as rt_query_closest: asynchronous
 * unless stats != NULL, ordered after the handle's earlier work; primary_rays =
 * n, nodes_visited = node records the query read, prims_tested = intersection
 * tests, ms = device time of the launch.  Unknown flag bits, or a NULL dev_rays
 * / dev_hits with n > 0: RT_E_INVALID.  n == 0: RT_OK, nothing launched.  No
 * scene: RT_E_NOSCENE.  Reads scene state only: it never changes a frame; a
 * multi-device handle answers from devices[0]. */
enum { RT_SWEEP_ENTRY_ONLY = 1u, RT_SWEEP_SKIP_SELF = 2u };
int rt_sweep_spheres(rt_renderer* r, const void* dev_rays, const void* dev_radii, float radius, uint32_t n,
                     uint32_t flags, void* dev_hits, void* stream, rt_stats* stats);
/* A one-cast sweep with tmin = 0 that waits for the answer, like rt_pick.
 * hit_out as dev_hits above; point_out (may be NULL) = origin + t * dir, the
 * ball's centre at contact (at a miss: at tmax).  flags as above. */
int rt_sweep_at(rt_renderer* r, const float origin[3], const float dir[3], float radius, float tmax,
                uint32_t flags, rt_hit* hit_out, float point_out[3]);
/* rt_pick's ray (Camera::getRay, tmin = 0, tmax = +inf) as a one-cast sweep of
 * radius `radius`, no flags: a cursor of finite size.  radius = 0 is rt_pick.
 * Waits for the answer. */
int rt_pick_thick(rt_renderer* r, float u, float v, float radius, rt_hit* hit_out, float point_out[3]);

/* ---- first-hit G-buffer --------------------------------------------------- */
/* The per-pixel geometry of the frame the current size and camera would
 * render: an id buffer (hover highlight, rubber-band selection), a depth
 * buffer (compositing rastered gizmos against the traced scene), normal and
 * albedo guide layers (a denoiser at low sample counts).  The reference has no
 * counterpart (its kernel writes one colour per pixel, src/renderer.cu:57-82).
 * Pixel (x, y)'s ray is rt_pick(x, y)'s and the frames' unjittered sample's:
 * origin pose[3].xyz, direction Camera::getRay(x, y) in source order (never the
 * RT_FLAG_COMPAT_FMA candidate), tmin = 0, tmax = +inf, nearest hit.
 * Three caller-owned device buffers in frame layout (row-major, pixel y*W + x),
 * each optional (NULL: not written); every pixel of a given buffer is written:
 *   dev_hits     rt_hit    {t, sphere} as rt_pick(x, y);   miss {+inf, RT_NO_HIT}
 *   dev_normals  float[4]  n = (o + t*d - c) * (1.0f / r), the frames' shading
 *                          normal, w = 0;                   miss four zeros
 *   dev_albedo   uint32    the sphere's packed RGBA8 as the frames shade it
 *                          (0xFFCCCCCC without albedo);     miss 0
 * A camera inside a sphere reports the far root, like the frames. */
typedef struct rt_gbuffer {
    void* dev_hits;    /* W*H rt_hit, or NULL   */
    void* dev_normals; /* W*H float[4], or NULL */
    void* dev_albedo;  /* W*H uint32, or NULL   */
} rt_gbuffer;
/* stream: a hipStream_t or NULL (the renderer's own); asynchronous unless
 * stats != NULL, and ordered after the handle's earlier work, like
 * rt_trace_rays.  With stats: primary_rays = W*H, nodes_visited / prims_tested
 * summed over the pixels, ms = device time of the launch, the rest 0.  NULL
 * `out` or all three buffers NULL: RT_E_INVALID.  No scene: RT_E_NOSCENE.
 * Reads scene and camera state only: it never changes a frame (progressive
 * accumulation, counters, the framebuffer, the next frame's image).  A
 * multi-device handle answers from devices[0] with the whole frame. */
int rt_render_gbuffer(rt_renderer* r, const rt_gbuffer* out, void* stream, rt_stats* stats);

/* ---- ambient-occlusion layer ---------------------------------------------- */
/* The depth cue of a sphere cloud: from every pixel's first hit (the G-buffer's:
 * rt_pick(x, y)'s ray and hit; a camera inside a sphere reports the far root),
 * `rays` short any-hit rays, cosine-weighted about the hit's shading normal, and
 * the share of them that reach `radius` unoccluded.  A viewer multiplies the
 * layer into its frame.  The reference has no counterpart.
 * Ray i of pixel (x, y), exactly in f32: origin p + n * 1e-5
 * with p = o + t*d and n = (p - c) * (1.0f / r), the frames' shadow-ray origin;
 * direction (n + s) / |n + s|, s a point of the unit sphere hashed from (the
 * renderer's seed, salt, y*W + x, i), or n where that degenerates; tmin = 0,
 * tmax = radius; rt_trace_rays' RT_QUERY_ANY test.  A miss pixel casts nothing.
 * Every pixel of each given buffer is written (row-major, pixel y*W + x). */
typedef struct rt_ao_params {
    uint32_t rays;    /* AO rays per hit pixel: 1, 2, 4, 8, 16, 32 or 64 */
    float    radius;  /* each AO ray's tmax in world units: > 0, +inf allowed */
    uint32_t salt;    /* mixed into the direction hash: successive calls with
                         different salts give independent directions, so a caller
                         can average them while the camera rests */
    uint32_t flags;   /* 0; unknown bits: RT_E_INVALID */
} rt_ao_params;
typedef struct rt_ao_out {
    void* dev_ao;        /* W*H float, or NULL: (rays - occluded) * (1.0f / rays); a miss pixel 1.0f */
    void* dev_occluded;  /* W*H uint32, or NULL: occluded count, 0..rays; a miss pixel 0 */
} rt_ao_out;
/* stream, ordering and asynchrony as rt_render_gbuffer.  With stats:
 * primary_rays = W*H, shadow_rays = the AO rays cast (rays x hit pixels),
 * nodes_visited / prims_tested = the primary walk once per pixel plus every AO
 * ray's any-hit walk, ms = device time of the launch, the rest 0.  No scene:
 * RT_E_NOSCENE.  NULL p or out, both buffers NULL, rays not one of the seven
 * values, radius NaN or <= 0, or unknown flags: RT_E_INVALID.  Reads scene and
 * camera state only: it never changes a frame.  A multi-device handle answers
 * from devices[0] with the whole frame. */
int rt_render_ao(rt_renderer* r, const rt_ao_params* p, const rt_ao_out* out, void* stream, rt_stats* stats);

/* ---- one-bounce diffuse light layer ---------------------------------------- */
/* What the constant ambient term cannot show: the light a hit receives from the
 * lit spheres around it, and its colour.  rt_render_ao's rays with another
 * payload: each returns its NEAREST hit shaded as a frame shades a primary hit,
 * or the frames' miss colour where it escapes, and a pixel stores their mean as
 * a float4 layer {r, g, b, w} that rt_reproject_layer and rt_filter_layer
 * (channels = 4) carry and rt_add_layer adds into the frame.
 * The reference has no counterpart.
 * Exactly in f32, in the stated order, no contraction, IEEE division and square
 * root, no transcendental.  Pixel (x, y): the primary ray and
 * hit are rt_pick(x, y)'s; p = o + t*d, n = (p - c) * (1.0f / r); the bounce
 * origin is o' = p + n * 1e-5 and ray i's direction d_i is rt_render_ao's (with
 * equal rays, radius and salt these are its rays bit for bit).  A miss pixel casts
 * nothing and stores {0, 0, 0, 1.0f} and a count of 0.
 * Ray i: tmin = 0, tmax = radius, RT_QUERY_NEAREST (smallest t, then smallest
 * sphere index).
 *   miss: c_i = {(200.0f/255.0f) * sky_scale, sat(d_i.y) * sky_scale,
 *         sat(d_i.z) * sky_scale}, sat(x) = x > 0 ? (x < 1 ? x : 1) : 0.
 *   hit on sphere (c2, r2) with albedo word al at t2:
 *         q = o' + t2*d_i;  m = (q - c2) * (1.0f / r2);
 *         ndl = (m.x*L.x + m.y*L.y) + m.z*L.z, L the handle's unit vector toward
 *         the light (-light_dir / |light_dir|);  lam = ndl > 0 ? ndl : 0;
 *         if ndl > 0 and the handle has no RT_FLAG_NO_SHADOWS: one RT_QUERY_ANY
 *         ray from q + m * 1e-5 along L, tmin = 0, tmax = +inf; a hit sets lam = 0;
 *         f = ambient + (1.0f - ambient) * lam;
 *         c_i[k] = (float)al_k * (1.0f / 255.0f) * f, al_k the k-th byte of al.
 * Sum: for m = 1, 2, 4, .. < rays every v[i] becomes v[i] + v[i ^ m] (the frames'
 * pairing), per channel; rgb = v[0] * (1.0f / rays); w = (float)(rays - hits) *
 * (1.0f / rays), hits the rays that hit: w has the bits of rt_render_ao's dev_ao
 * and dev_occluded equals its dev_occluded under equal parameters. */
typedef struct rt_indirect_params {
    uint32_t rays;       /* bounce rays per hit pixel: 1, 2, 4, 8, 16, 32 or 64 */
    float    radius;     /* each bounce ray's tmax in world units: > 0, +inf allowed */
    uint32_t salt;       /* as rt_ao_params.salt */
    float    sky_scale;  /* finite, >= 0: what a ray that escapes brings, times the frames' miss colour */
    uint32_t flags;      /* 0; unknown bits RT_E_INVALID */
} rt_indirect_params;
typedef struct rt_indirect_out {
    void* dev_layer;     /* W*H float[4], 16-byte aligned, or NULL: {r, g, b, w}; a miss pixel {0, 0, 0, 1.0f} */
    void* dev_occluded;  /* W*H uint32, or NULL: bounce rays that hit something, 0..rays; a miss pixel 0 */
} rt_indirect_out;
/* stream, ordering and asynchrony as rt_render_ao.  With stats: primary_rays =
 * W*H, shadow_rays = the bounce rays cast (rays x hit pixels) plus the shadow
 * rays cast at their hits, nodes_visited / prims_tested = the primary walk once
 * per pixel plus every bounce ray's nearest walk plus every such shadow ray's
 * any-hit walk, ms = device time of the launch, the rest 0.  NULL p or out, both
 * buffers NULL, rays not one of the seven values, radius NaN or <= 0, sky_scale
 * NaN, infinite or negative, or unknown flags: RT_E_INVALID, and nothing is
 * launched.  No scene: RT_E_NOSCENE.  Reads scene and camera state and the
 * handle's light_dir, ambient and RT_FLAG_NO_SHADOWS only: it never changes a
 * frame.  A multi-device handle answers from devices[0] with the whole frame. */
int rt_render_indirect(rt_renderer* r, const rt_indirect_params* p, const rt_indirect_out* out, void* stream,
                       rt_stats* stats);

/* ---- guide-driven layer filter, and a layer applied to a frame ------------ */
/* What makes a cheap layer displayable: an edge-avoiding a-trous filter over any
 * per-pixel float layer (rt_render_ao's dev_ao at 4 rays; a float4 radiance
 * layer), steered by the G-buffer's depth and normals, and the multiply of a
 * layer into an RGBA8 frame.  The reference has no counterpart.
 * guides: dev_hits and dev_normals as rt_render_gbuffer wrote them for the
 * handle's current size, both required (a hit's t is finite); dev_albedo is
 * ignored.  dev_in and dev_out: W*H*channels floats each (channels 4: 16-byte
 * aligned), distinct; dev_in is never written, every element of dev_out is.
 * Exactly in f32, no contraction, IEEE division: pixel q is a
 * miss iff its rt_hit.sphere == RT_NO_HIT; t_q and n_q are a hit's rt_hit.t and
 * the first three floats of its normal.  Pass s (0-based) reads pass s - 1's
 * output (pass 0: dev_in) with step = 1 << s.  A miss pixel copies its value.  A
 * hit pixel p = (x, y) starts from sw = 0, sv[c] = 0 and visits the 25 taps
 * q = (x + i*step, y + j*step), j = -2..2 outer, i = -2..2 inner, the centre by
 * the same formula; a tap outside the image or a miss tap is skipped; otherwise
 *   k  = K[|i|] * K[|j|], K = {0.375f, 0.25f, 0.0625f}
 *   dn = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
 *   wn = fmaxf(dn, 0.0f), then wn = wn * wn repeated normal_power times
 *   e  = (t_q - t_p) * iz, iz = 1.0f / (depth_sigma * t_p) once per pixel
 *   wz = 1.0f / (1.0f + e*e);  w = (k * wn) * wz
 *   sw += w;  sv[c] += w * v_q[c] in channel order
 * and the output is sw > 0.0f ? sv[c] / sw : v_p[c] (false for a NaN: garbage
 * guides copy the value).  NaN and infinite layer values propagate as the
 * arithmetic says. */
typedef struct rt_filter_params {
    uint32_t passes;        /* 1..5; pass s (0-based) uses tap spacing 2^s */
    uint32_t channels;      /* 1 (e.g. rt_render_ao's dev_ao) or 4 (float4, e.g. radiance) */
    float    depth_sigma;   /* relative depth tolerance, > 0; +inf: depth ignored */
    uint32_t normal_power;  /* 0..7: normal weight = max(n.n', 0)^(2^normal_power) */
    uint32_t flags;         /* 0; unknown bits RT_E_INVALID */
} rt_filter_params;
void rt_filter_params_default(rt_filter_params*);   /* passes 3, channels 1, depth_sigma 0.05f, normal_power 5 */
/* stream, ordering and asynchrony as rt_render_gbuffer.  With stats: ms = device
 * time of the guide packing and all passes, every counter 0.  NULL p, guides,
 * dev_in or dev_out, a missing guide buffer, dev_in == dev_out, passes outside
 * 1..5, channels not 1 or 4, depth_sigma NaN or <= 0, normal_power > 7 or
 * unknown flags: RT_E_INVALID, and nothing is launched.  Needs no scene.  Reads
 * the handle's size only: it never changes a frame, its progressive sums or the
 * counters.  The packed guides and one scratch layer are the handle's own (they
 * grow with the size and are released by rt_destroy).  A multi-device handle
 * runs it on devices[0]. */
int rt_filter_layer(rt_renderer* r, const rt_filter_params* p, const rt_gbuffer* guides,
                    const void* dev_in, void* dev_out, void* stream, rt_stats* stats);
/* Multiplies a W*H float layer into W*H packed RGBA8 pixels in place, one pass:
 * m = floor + (1.0f - floor) * layer (one multiply, then one add); each of R, G
 * and B becomes (uint8_t)fminf((float)c * m, 255.0f), truncated like the frames'
 * own conversion (a negative product stores 0); A is unchanged.  dev_rgba8 NULL:
 * the handle's internal framebuffer.  A bound display is never mapped: pass its
 * mapped pointer.  floor NaN or outside [0, 1], or a NULL layer: RT_E_INVALID.
 * Stream and ordering as above.  Only the given buffer is modified: a
 * progressive handle's sums are not, so the next rt_render overwrites the result. */
int rt_apply_layer(rt_renderer* r, void* dev_rgba8, const void* dev_layer, float floor, void* stream);
/* Adds a W*H float[4] layer (rt_render_indirect's dev_layer, carried and filtered
 * or not) into W*H packed RGBA8 pixels in place, one pass.  For each of R, G and
 * B, with c the frame's byte, a_k the albedo's byte and layer[k] the layer's
 * channel:
 *   k = dev_albedo ? (float)a_k * (1.0f / 255.0f) : 1.0f;
 *   v = (float)c + ((k * gain) * layer[k]) * 255.0f;
 * and the stored byte is (uint8_t)fminf(fmaxf(v, 0.0f), 255.0f): truncated like
 * the frames' own conversion, a NaN stores 0.  A is unchanged and the layer's w
 * is not read.  dev_albedo: W*H RGBA8 as rt_render_gbuffer wrote it (the surface
 * that receives the light reflects it by its own colour), or NULL: white.
 * dev_rgba8 NULL: the handle's internal framebuffer.  A bound display is never
 * mapped: pass its mapped pointer.  gain NaN, infinite or negative, or a NULL
 * layer: RT_E_INVALID.  Stream and ordering as rt_apply_layer; only the given
 * buffer is modified. */
int rt_add_layer(rt_renderer* r, void* dev_rgba8, const void* dev_layer4, const void* dev_albedo, float gain,
                 void* stream);

/* A per-pixel layer carried across camera motion: the running mean of a layer
 * (rt_render_ao's dev_ao at a few rays, salt = the frame number; a float4 radiance
 * layer) reprojected from the previous camera into the handle's current one, the
 * one rt_render_gbuffer just used.  The primitives are spheres, so "the same
 * surface as last frame" is the equality of two sphere indices plus a relative
 * depth tolerance.  The caller keeps two sets of {hits, layer, count} and swaps
 * them each frame; the handle keeps nothing.  While the camera rests the result
 * is the plain mean of the layers (count k + 1 on frame k, up to max_count).
 * Exactly in f32, in the stated order, no contraction, IEEE division and square
 * root.  o = pose[3].xyz and d = Camera::getRay(x, y) of the
 * current camera, exactly rt_render_gbuffer's ray; o', P' = hist->pose and
 * fx = K'[0], fy = K'[4], cx = K'[2], cy = K'[5] of hist->K.  Per pixel (x, y) with
 * its current hit {t, s}:
 *   1. out[c] = cur[c], count = 1.0f for a miss (s == RT_NO_HIT), for hist == NULL
 *      and where no tap below is accepted.
 *   2. p = o + t*d (one multiply, then one add);  q = p - o';
 *      c_x = (P'[0]*q.x + P'[1]*q.y) + P'[2]*q.z, c_y with P'[4..6], c_z with
 *      P'[8..10] (the rotation block's transpose, used as given);
 *      dist = sqrtf((q.x*q.x + q.y*q.y) + q.z*q.z);  taps only if c_z > 0.0f
 *      (false for a NaN).
 *   3. u = (c_x / c_z) * fx + cx, v = (c_y / c_z) * fy + cy;  u0 = floorf(u),
 *      v0 = floorf(v), a = u - u0, b = v - v0.
 *   4. taps (u0 + i, v0 + j), j = 0, 1 outer, i = 0, 1 inner.  A tap is inside iff
 *      0 <= u0 + i <= W - 1 and 0 <= v0 + j <= H - 1, compared in float (a NaN or a
 *      huge coordinate is outside).  An inside tap with history hit {t', s'} is
 *      accepted iff s' == s and fabsf(dist - t') <= depth_tol * t'.  Then
 *      wx = i ? a : 1.0f - a, wy = j ? b : 1.0f - b, w = wx * wy;
 *      sw += w;  sv[c] += w * hist_layer[c];  sc += w * hist_count.
 *   5. if sw > 0.0f: hv[c] = sv[c] / sw, hc = sc / sw, n = fminf(hc + 1.0f,
 *      max_count), alpha = 1.0f / n, out[c] = hv[c] + (cur[c] - hv[c]) * alpha,
 *      count = n;  else rule 1.
 * NaN and infinite layer or count values propagate as the arithmetic says.  The
 * history assumes a static scene between the two frames. */
typedef struct rt_history {          /* the previous frame's, all caller-owned, the handle's current size */
    const void* dev_hits;   /* W*H rt_hit: rt_render_gbuffer's dev_hits under the previous camera */
    const void* dev_layer;  /* W*H*channels floats: the previous call's dev_out */
    const void* dev_count;  /* W*H floats: the previous call's dev_count_out */
    float pose[16];         /* the previous camera, as rt_set_pose / rt_set_intrinsic take them */
    float K[9];
} rt_history;
typedef struct rt_reproject_params {
    uint32_t channels;   /* 1 or 4 (4: 16-byte aligned layers) */
    float    max_count;  /* finite, >= 1: the mean's longest memory; 1/max_count is the smallest blend weight */
    float    depth_tol;  /* > 0, +inf allowed: relative tolerance between the point's distance from the previous camera and the history's t */
    uint32_t flags;      /* 0; unknown bits RT_E_INVALID */
} rt_reproject_params;
void rt_reproject_params_default(rt_reproject_params*);   /* channels 1, max_count 32, depth_tol 0.05f */
/* stream, ordering and asynchrony as rt_filter_layer.  With stats: ms = device
 * time of the pass, every counter 0.  A NULL p, dev_hits, dev_cur, dev_out or
 * dev_count_out, a non-NULL hist with a NULL member buffer, dev_out equal to
 * dev_cur or to hist->dev_layer, dev_count_out equal to hist->dev_count, channels
 * not 1 or 4, max_count NaN, infinite or below 1, depth_tol NaN or <= 0, or unknown
 * flags: RT_E_INVALID, and nothing is launched.  Needs no scene.  Reads the
 * handle's size and camera only: it never changes a frame, its progressive sums
 * or the counters.  A multi-device handle runs it on devices[0]. */
int rt_reproject_layer(rt_renderer* r, const rt_reproject_params* p,
                       const void* dev_hits,        /* W*H rt_hit: the CURRENT camera's G-buffer hits */
                       const rt_history* hist,      /* NULL: no history (first frame, after a resize or a scene change) */
                       const void* dev_cur,         /* W*H*channels: this frame's layer, never written */
                       void* dev_out, void* dev_count_out,   /* W*H*channels and W*H floats; every element written */
                       void* stream, rt_stats* stats);

/* ---- one process, several devices (SURVEY 8b B2 "device ids", 8e E1) ------ */
/* A renderer handle that renders every frame across n_devices GPUs of this
 * process: one renderer per device (same config, same scene: replicated), the
 * frame's 64x64 tiles dealt round-robin (tile t to device t mod n), each
 * device rendering its tiles into a packed slab on its own stream, the slabs
 * moved to devices[0] (RCCL: one ncclCommInitAll communicator over the
 * devices, grouped ncclSend / ncclRecv on per-device comm streams; or peer
 * copies) and unpacked there by ONE launch into the frame.  Two frames are in
 * flight: frame k+1's tiles render while frame k's slabs travel and unpack.
 * Every other entry point works on the handle as on a single-device one
 * (rt_set_pose / rt_set_intrinsic / rt_resize / rt_set_scene / rt_set_octree
 * / rt_reset_accumulation apply to every device; rt_set_scene_device takes a
 * sphere list on devices[0] and broadcasts it (ncclBroadcast); rt_render,
 * rt_bind_graphics_resource / rt_bind_display, rt_readback, rt_framebuffer,
 * rt_stream, rt_get_scene_info and rt_export_octree are devices[0]'s), except
 * rt_render_tiles / rt_unpack_tiles (RT_E_STATE: the handle renders whole
 * frames).  rt_render with stats renders the devices one after another and
 * sums their counters (ms = host wall time of the frame).  The reference's
 * Displayer (src/window/displayer.cpp:28) constructs the renderer this way
 * and calls render() unchanged.
 * devices: HIP ordinals; a repeated ordinal (e.g. {0,0,0,0}) rehearses the
 * n-way plan on fewer GPUs (peer-copy transport only: RCCL refuses a device
 * twice in one communicator).  cfg->device is ignored. */
enum {
    RT_TRANSPORT_AUTO = 0, /* RCCL when the devices are distinct and librccl loads, else peer */
    RT_TRANSPORT_RCCL = 1, /* grouped ncclSend / ncclRecv over one ncclCommInitAll communicator */
    RT_TRANSPORT_PEER = 2  /* hipMemcpyPeerAsync on the comm streams (xGMI, or a local copy) */
};
#define RT_MAX_DEVICES 16
typedef struct rt_multi_info {
    uint32_t n_devices;              /* 1 for a single-device handle                     */
    int32_t devices[RT_MAX_DEVICES]; /* HIP ordinals, devices[0] holds the frame           */
    uint32_t transport;              /* RT_TRANSPORT_RCCL or RT_TRANSPORT_PEER (0: single)  */
    uint32_t tile_size;              /* 64                                                */
    uint32_t slab_tiles;             /* tiles per device slab (ceil(tiles / n_devices))   */
    uint32_t frames_in_flight;       /* 2                                                 */
    uint64_t frames;                 /* frames rendered by the handle                     */
} rt_multi_info;
/* Refuses RT_FLAG_RADIANCE (RT_E_INVALID: the slabs carry RGBA8 only).  The
 * tile plan and its slabs are allocated here for cfg's size (again at the
 * first frame after a resize), so an allocation failure is reported by this
 * call.  A NULL stream argument (rt_render, rt_stream) means the handle's
 * output stream on devices[0], which is not devices[0]'s render stream, so
 * frame j+1's tiles there do not wait for frame j's unpack.  A failure on one
 * device names it in rt_last_error: "(device <ordinal>, peer <k>)".
 * Test-only (with RT_FLAG_TEST_HOOKS): the environment variable RT_TEST_FAULT,
 * read here, injects one failure: "create:k" (peer k's renderer), "comm"
 * (ncclCommInitAll), "slab:k" (peer k's slab allocation) or "queue:k" (peer
 * k's plain frames report themselves incomplete, which the next rt_render,
 * rt_synchronize or rt_readback returns as RT_E_HIP naming the peer); rt_create
 * honours "queue:0" for a single-device renderer. */
int rt_create_multi(const rt_config* cfg, const int32_t* devices, uint32_t n_devices,
                    uint32_t transport, rt_renderer** out);
int rt_get_multi_info(const rt_renderer* r, rt_multi_info* info);
/* Device times of the handle's last frame (waits for the handle's queued
 * work): render_ms[k] = device k rendering its tiles into its slab (HIP
 * events on its render stream); deliver_ms = on devices[0], from the end of
 * its own tiles to the frame unpacked (the other slabs' arrival over the
 * transport, then the one unpack).  Frames record timing events only after
 * the handle's first rt_get_multi_timing call (the frame path's own
 * synchronisation events stay timing-free), so that first call, like one for
 * a single-device handle or an untimed last frame, returns RT_E_STATE. */
typedef struct rt_multi_timing {
    uint32_t n_devices;
    uint64_t frame;                   /* 0-based index of the frame timed           */
    float render_ms[RT_MAX_DEVICES];
    float deliver_ms;
} rt_multi_timing;
int rt_get_multi_timing(rt_renderer* r, rt_multi_timing* t);

/* ---- errors --------------------------------------------------------------- */
/* Last error message for this handle (r may be NULL: last global error). */
const char* rt_last_error(const rt_renderer* r);

#ifdef __cplusplus
}
#endif

#endif /* RT_AMD_RT_H */
