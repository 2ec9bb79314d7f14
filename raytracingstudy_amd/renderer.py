"""Host-side mirror of the reference's ``KernelRenderer`` over the C-ABI.

Reference interface (``include/renderer.cuh:25-50``)::

    KernelRenderer(cudaGraphicsResource_t cudaResource, int width, int height);
    void render();
    void resize(int width, int height);
    void setPosition(glm::mat4 pose);
    void setIntrinsic(glm::mat3 intrinsic);
    void setOctree(glm::vec3 min, glm::vec3 max, float resolution);

This class keeps those method names, argument meanings (glm column-major
matrices, pixel units) and call order, and adds what the reference left as
stubs: a real scene (``set_scene``), tiles for multi-GPU sharding, stats and
error reporting (the reference's methods return ``void`` and check nothing;
here a failing call raises ``RtError`` with the library's message).

Matrices are given in glm indexing: ``pose[c][r]`` is glm's ``m[c][r]`` (column
``c``, row ``r``), so ``pose[3][:3]`` is the camera origin
(``include/camera.h:43-46``) and ``K[0][2]``/``K[1][2]`` are cx/cy
(``include/camera.h:26-27``).  Flattening in C order yields glm's memory layout.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (RT_FLAG_HOST_BUILD, RT_FLAG_JITTER, RT_FLAG_NO_JITTER, RT_FLAG_NO_SHADOWS,
                   RT_FLAG_PROGRESSIVE, RT_FLAG_RADIANCE,
                   RT_MODE_COMPAT, RT_MODE_SCENE, RtConfig, RtOctreeParams, RtSceneInfo,
                   RtStats, check)

__all__ = ["KernelRenderer", "resize_intrinsic", "generate_spheres", "device_count",
           "save_spheres", "load_spheres"]

_MODES = {"compat": RT_MODE_COMPAT, "scene": RT_MODE_SCENE}
_QUERY_KINDS = {"nearest": _lib.RT_QUERY_NEAREST, "any": _lib.RT_QUERY_ANY}


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _vptr(a: Optional[np.ndarray]):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _ptr(x: Optional[int]):
    """A device address or a stream as a pointer argument (None or 0: NULL)."""
    return ctypes.c_void_p(x) if x else None


def _stats_arg(stats: bool):
    """(the RtStats a call fills or None, what to pass for it)."""
    st = RtStats() if stats else None
    return st, (ctypes.byref(st) if stats else None)


def _records(a, cols: int, what: str, layout: str) -> np.ndarray:
    """`a` as the contiguous, writable (n, cols) float32 array a batch query uploads."""
    a = np.ascontiguousarray(a, np.float32)
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError(f"{what} must be an (n, {cols}) float32 array in {layout} layout")
    return a if a.flags.writeable else a.copy()  # torch.from_numpy wants a writable array


def _split_pairs(words: np.ndarray):
    """(..., 2) int32 records {float bits, index} (rt_hit, rt_near) ->
    (float32 (...), uint32 (...)): two arrays of their own, bit for bit."""
    return words[..., 0].copy().view(np.float32), words[..., 1].copy().view(np.uint32)


def _overlap_words(words):
    """rt_query_overlaps' count words -> (count uint32, more bool)."""
    words = np.asarray(words, np.uint32)
    more = np.uint32(_lib.RT_OVERLAP_MORE)
    return words & ~more, (words & more) != 0


def device_count() -> int:
    return int(_lib.load().rt_device_count())


def resize_intrinsic(width: int, height: int) -> np.ndarray:
    """K the reference's resize() sets (src/renderer.cu:162-170), glm [c][r] indexing."""
    K = np.zeros(9, np.float32)
    _lib.load().rt_resize_intrinsic(width, height, _fptr(K))
    return K.reshape(3, 3)


def generate_spheres(n: int, seed: int = 0x2545F491):
    """SURVEY.md 8d synthetic spheres: (n,4) float32 (cx,cy,cz,r) and (n,) uint32 albedo."""
    sp = np.zeros((max(n, 1), 4), np.float32)
    al = np.zeros(max(n, 1), np.uint32)
    check(_lib.load().rt_generate_spheres(n, seed, _vptr(sp), _vptr(al)))
    return sp[:n], al[:n]


def save_spheres(path: str, spheres: np.ndarray, albedo: Optional[np.ndarray] = None) -> None:
    """Write a binary sphere file (rt_save_spheres; format in DESIGN.md §4.1)."""
    sp = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
    al = None if albedo is None else np.ascontiguousarray(albedo, np.uint32).reshape(-1)
    if al is not None and al.shape[0] != sp.shape[0]:
        raise ValueError("albedo must have one entry per sphere")
    check(_lib.load().rt_save_spheres(str(path).encode(), _vptr(sp), _vptr(al), sp.shape[0]))


def load_spheres(path: str):
    """Read a binary sphere file: ((n,4) float32 spheres, (n,) uint32 albedo)."""
    lib = _lib.load()
    n = ctypes.c_uint32(0)
    check(lib.rt_load_spheres(str(path).encode(), None, None, 0, ctypes.byref(n)))
    sp = np.zeros((max(n.value, 1), 4), np.float32)
    al = np.zeros(max(n.value, 1), np.uint32)
    check(lib.rt_load_spheres(str(path).encode(), _vptr(sp), _vptr(al), sp.shape[0],
                              ctypes.byref(n)))
    return sp[:n.value], al[:n.value]


def _octree_params(root_min, root_max, resolution, max_depth, leaf_capacity) -> RtOctreeParams:
    p = RtOctreeParams()
    for i in range(3):
        p.min[i] = float(root_min[i])
        p.max[i] = float(root_max[i])
    p.resolution = float(resolution)
    p.max_depth = int(max_depth)
    p.leaf_capacity = int(leaf_capacity)
    return p


class KernelRenderer:
    """MI355X renderer handle (one per thread / stream)."""

    def __init__(self, width: int, height: int, *, mode: str = "compat", spp: int = 1,
                 seed: int = 0x2545F491, device: int = -1, jitter: Optional[bool] = None,
                 shadows: bool = True, radiance: bool = False,
                 light_dir: Sequence[float] = (1.0, 1.0, -1.0), ambient: float = 0.1,
                 variant: int = 0, opt_off: int = 0, host_build: bool = False,
                 progressive: bool = False, cell_table: Optional[int] = None,
                 compat_fma: bool = False, pad_fill: int = 0, occluders: bool = True,
                 bins: bool = True, pairs: bool = True,
                 devices: Optional[Sequence[int]] = None, transport: str = "auto"):
        """devices: render every frame across these HIP devices of this process
        (rt_create_multi: tiles round-robin, slabs gathered to devices[0] over
        RCCL or peer copies, one unpack); a repeated ordinal rehearses the plan
        on fewer GPUs.  transport: "auto", "rccl" or "peer"."""
        lib = _lib.load()
        cfg = RtConfig()
        lib.rt_config_default(ctypes.byref(cfg))
        cfg.width, cfg.height = int(width), int(height)
        cfg.spp = int(spp)
        cfg.seed = int(seed) & 0xFFFFFFFF
        cfg.device = int(device)
        cfg.mode = _MODES[mode]
        flags = 0
        if jitter is True:
            flags |= RT_FLAG_JITTER
        elif jitter is False:
            flags |= RT_FLAG_NO_JITTER
        if not shadows:
            flags |= RT_FLAG_NO_SHADOWS
        if radiance:
            flags |= RT_FLAG_RADIANCE
        if host_build:
            flags |= RT_FLAG_HOST_BUILD
        if progressive:
            flags |= RT_FLAG_PROGRESSIVE
        if compat_fma:
            flags |= _lib.RT_FLAG_COMPAT_FMA
        if not occluders:  # A/B: every shadow ray walks the octree
            flags |= _lib.RT_FLAG_NO_OCCLUDERS
        if not bins:  # A/B: every primary ray walks the octree
            flags |= _lib.RT_FLAG_NO_BINS
        if not pairs:  # A/B: one pixel a wave pass in every frame
            flags |= _lib.RT_FLAG_NO_PAIRS
        # pad_fill (test-only): 0 zeros, 1 NaN, 2 covering spheres after the last leaf list
        if not 0 <= int(pad_fill) <= 2:
            raise ValueError("pad_fill must be 0, 1 or 2")
        flags |= int(pad_fill) << _lib.RT_FLAG_PAD_FILL_SHIFT
        flags |= (int(variant) & 0xF) << _lib.RT_FLAG_VARIANT_SHIFT
        flags |= (int(opt_off) & 0xFF) << _lib.RT_FLAG_OPT_SHIFT
        # cell_table: None = depth chosen from the tree, 0 = no table, k = depth k
        if cell_table is not None:
            ct = _lib.RT_CELL_TABLE_OFF if int(cell_table) == 0 else int(cell_table)
            if not 1 <= ct <= 15:
                raise ValueError("cell_table must be None, 0 (off) or a depth 1..7")
            flags |= ct << _lib.RT_FLAG_CELL_TABLE_SHIFT
        cfg.flags = flags | _lib.test_flags
        for i in range(3):
            cfg.light_dir[i] = float(light_dir[i])
        cfg.ambient = float(ambient)
        self._lib = lib
        self.config = cfg
        self.mode = mode
        self.radiance = radiance
        h = ctypes.c_void_p()
        if devices is None:
            check(lib.rt_create(ctypes.byref(cfg), ctypes.byref(h)))
        else:
            tr = {"auto": _lib.RT_TRANSPORT_AUTO, "rccl": _lib.RT_TRANSPORT_RCCL,
                  "peer": _lib.RT_TRANSPORT_PEER}[transport]
            devs = (ctypes.c_int32 * len(devices))(*[int(d) for d in devices])
            check(lib.rt_create_multi(ctypes.byref(cfg), devs, len(devices), tr, ctypes.byref(h)))
        self._h = h
        self.width, self.height = int(width), int(height)

    # -- reference method names -------------------------------------------------
    def render(self, dev_ptr: Optional[int] = None, stream: Optional[int] = None,
               stats: bool = False) -> Optional[RtStats]:
        """render() (src/renderer.cu:143-153).  dev_ptr: a device RGBA8 buffer
        (e.g. the mapped GL PBO pointer) or None for the internal framebuffer."""
        st, st_arg = _stats_arg(stats)
        check(self._lib.rt_render(self._h, _ptr(dev_ptr), _ptr(stream), st_arg), self._h)
        return st

    def resize(self, width: int, height: int) -> None:
        """resize() (src/renderer.cu:155-187): new size + the FOV-80 intrinsic."""
        check(self._lib.rt_resize(self._h, int(width), int(height)), self._h)
        self.width, self.height = int(width), int(height)

    def setPosition(self, pose) -> None:
        """setPosition(glm::mat4) (src/renderer.cu:111-113, include/camera.h:43-46)."""
        p = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(16))
        check(self._lib.rt_set_pose(self._h, _fptr(p)), self._h)

    def setIntrinsic(self, K) -> None:
        """setIntrinsic(glm::mat3) (src/renderer.cu:115-117)."""
        k = np.ascontiguousarray(np.asarray(K, np.float32).reshape(9))
        check(self._lib.rt_set_intrinsic(self._h, _fptr(k)), self._h)

    def setOctree(self, mn, mx, resolution: float) -> None:
        """setOctree(min, max, resolution) (include/renderer.cuh:35; undefined in
        the reference).  Rebuilds the octree of the current spheres."""
        a = np.asarray(mn, np.float32).reshape(3).copy()
        b = np.asarray(mx, np.float32).reshape(3).copy()
        check(self._lib.rt_set_octree(self._h, _fptr(a), _fptr(b), float(resolution)), self._h)

    # -- additions ------------------------------------------------------------
    def bind_display(self, map_fn=None, unmap_fn=None) -> None:
        """A display buffer mapped per frame (rt_bind_display): the
        reference's render() maps its PBO, renders into it and unmaps it
        (src/renderer.cu:145-151).  map_fn(stream) -> (device_ptr, nbytes) or
        None (failure); unmap_fn(stream) -> None, or False on failure.  Called
        with no arguments it unbinds (render into the internal framebuffer)."""
        if map_fn is None:
            self._display = None
            check(self._lib.rt_bind_display(self._h, None, None), self._h)
            return

        def _map(_user, stream, ptr, nbytes):
            try:
                got = map_fn(stream or 0)
            except Exception:  # an exception must not unwind through C
                return 1
            if got is None:
                return 1
            ptr[0], nbytes[0] = int(got[0]), int(got[1])
            return 0

        def _unmap(_user, stream):
            try:
                return 1 if unmap_fn(stream or 0) is False else 0
            except Exception:
                return 1

        ops = _lib.RtDisplayOps(_lib.DISPLAY_MAP(_map), _lib.DISPLAY_UNMAP(_unmap))
        self._display = ops  # the C side keeps raw function pointers: keep them alive
        check(self._lib.rt_bind_display(self._h, ctypes.byref(ops), None), self._h)

    def set_scene(self, spheres: np.ndarray, albedo: Optional[np.ndarray] = None, *,
                  root_min=(0.0, 0.0, 0.0), root_max=(1.28, 1.28, 1.28),
                  resolution: float = 0.01, max_depth: int = 0, leaf_capacity: int = 8) -> dict:
        sp = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
        al = None if albedo is None else np.ascontiguousarray(albedo, np.uint32).reshape(-1)
        if al is not None and al.shape[0] != sp.shape[0]:
            raise ValueError("albedo must have one entry per sphere")
        p = _octree_params(root_min, root_max, resolution, max_depth, leaf_capacity)
        check(self._lib.rt_set_scene(self._h, _vptr(sp), _vptr(al), sp.shape[0], ctypes.byref(p)),
              self._h)
        return self.scene_info()

    def set_scene_device(self, spheres_ptr: int, n: int, albedo_ptr: Optional[int] = None, *,
                         stream: Optional[int] = None, root_min=(0.0, 0.0, 0.0),
                         root_max=(1.28, 1.28, 1.28), resolution: float = 0.01,
                         max_depth: int = 0, leaf_capacity: int = 8) -> dict:
        """Scene from a sphere list already in device memory (4*n float32 at
        spheres_ptr, n RGBA8 words at albedo_ptr); the octree is built on the GPU."""
        p = _octree_params(root_min, root_max, resolution, max_depth, leaf_capacity)
        check(self._lib.rt_set_scene_device(self._h, _ptr(spheres_ptr), _ptr(albedo_ptr), int(n),
                                            ctypes.byref(p), _ptr(stream)), self._h)
        return self.scene_info()

    def set_scene_file(self, path: str, **octree) -> dict:
        """Load a binary sphere file (load_spheres) and make it the scene."""
        sp, al = load_spheres(path)
        return self.set_scene(sp, al, **octree)

    def export_octree(self):
        """The device octree as host arrays: nodes (n,2) uint32 records, prim_sp
        (m,4) float32, prim_idx (m,) uint32 (rt_export_octree)."""
        info = self.scene_info()
        nodes = np.zeros((max(info["n_nodes"], 1), 2), np.uint32)
        m = info["n_prim_refs"]
        sp = np.zeros((max(m, 1), 4), np.float32)
        idx = np.zeros(max(m, 1), np.uint32)
        check(self._lib.rt_export_octree(self._h, _vptr(nodes), _vptr(sp), _vptr(idx)), self._h)
        return nodes[:info["n_nodes"]], sp[:m], idx[:m]

    def export_occluders(self):
        """The occluder lists as host arrays (rt_export_occluders): per sphere
        offsets and counts (0xFFFFFFFF: that sphere's shadow rays walk), the
        lists' sphere indices, and the (m, 2) per-reference headers."""
        info = self.scene_info()
        n, m, e = info["n_spheres"], info["n_prim_refs"], info["occluder_entries"]
        off = np.zeros(max(n, 1), np.uint32)
        cnt = np.zeros(max(n, 1), np.uint32)
        idx = np.zeros(max(e, 1), np.uint32)
        refs = np.zeros((max(m, 1), 2), np.uint32)
        check(self._lib.rt_export_occluders(self._h, _vptr(off), _vptr(cnt), _vptr(idx), _vptr(refs)),
              self._h)
        return off[:n], cnt[:n], idx[:e], refs[:m]

    def bin_info(self) -> dict:
        """rt_get_bin_info: the last frame's screen-space bins (waits for it)."""
        info = _lib.RtBinInfo()
        check(self._lib.rt_get_bin_info(self._h, ctypes.byref(info)), self._h)
        return info.as_dict()

    def last_instance(self) -> int:
        """rt_last_instance: the Frame<> switches of the last scene frame's kernel
        (bit 7, 128: pixel pairs)."""
        return int(self._lib.rt_last_instance(self._h))

    def export_bins(self):
        """The last frame's bins as host arrays (rt_export_bins): (bins, 2)
        headers {first entry, count | 0xFFFFFFFF}, the lists' sphere indices,
        and the wide list's sphere indices."""
        bi = self.bin_info()
        hdr = np.zeros((max(bi["bins"], 1), 2), np.uint32)
        idx = np.zeros(max(bi["entries"], 1), np.uint32)
        wide = np.zeros(max(bi["wide"], 1), np.uint32)
        check(self._lib.rt_export_bins(self._h, _vptr(hdr), _vptr(idx), _vptr(wide)), self._h)
        return hdr[:bi["bins"]], idx[:bi["entries"]], wide[:bi["wide"]]

    def export_bin_tiles(self):
        """The last frame's tile words (rt_export_bin_tiles): (tw, th) the
        frame's wave tile in pixels and a (bins, tiles_per_bin) uint64 array,
        bit k of a word: the bin's entry k overlaps that wave tile."""
        bi = self.bin_info()
        tw, th, tpb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(self._lib.rt_export_bin_tiles(self._h, ctypes.byref(tw), ctypes.byref(th), ctypes.byref(tpb),
                                            None), self._h)
        words = np.zeros((max(bi["bins"], 1), tpb.value), np.uint64)
        check(self._lib.rt_export_bin_tiles(self._h, None, None, None, _vptr(words)), self._h)
        return (tw.value, th.value), words[:bi["bins"]]

    def scene_info(self) -> dict:
        info = RtSceneInfo()
        check(self._lib.rt_get_scene_info(self._h, ctypes.byref(info)), self._h)
        return info.as_dict()

    def multi_info(self) -> dict:
        """rt_get_multi_info: the devices, transport and tile plan of the handle
        (n_devices 1 for a single-device renderer)."""
        info = _lib.RtMultiInfo()
        check(self._lib.rt_get_multi_info(self._h, ctypes.byref(info)), self._h)
        return info.as_dict()

    def multi_timing(self) -> dict:
        """rt_get_multi_timing: per-device render ms of the last frame (HIP
        events on each device's render stream) and devices[0]'s delivery ms
        (its own tiles' end -> the frame unpacked).  Waits for the handle."""
        t = _lib.RtMultiTiming()
        check(self._lib.rt_get_multi_timing(self._h, ctypes.byref(t)), self._h)
        return t.as_dict()

    def camera(self):
        pose = np.zeros(16, np.float32)
        K = np.zeros(9, np.float32)
        check(self._lib.rt_get_camera(self._h, _fptr(pose), _fptr(K)), self._h)
        return pose.reshape(4, 4), K.reshape(3, 3)

    def render_tiles(self, tile_ids, tile_size: int, dev_ptr: int, stream: Optional[int] = None,
                     stats: bool = False) -> Optional[RtStats]:
        ids = np.ascontiguousarray(tile_ids, np.uint32)
        st, st_arg = _stats_arg(stats)
        check(self._lib.rt_render_tiles(self._h, _vptr(ids), ids.shape[0], int(tile_size),
                                        _ptr(dev_ptr), _ptr(stream), st_arg), self._h)
        return st

    def unpack_tiles(self, dev_packed: int, tile_ids, tile_size: int,
                     dev_rgba8: Optional[int] = None, stream: Optional[int] = None) -> None:
        ids = np.ascontiguousarray(tile_ids, np.uint32)
        check(self._lib.rt_unpack_tiles(self._h, _ptr(dev_packed), _vptr(ids), ids.shape[0],
                                        int(tile_size), _ptr(dev_rgba8), _ptr(stream)), self._h)

    # -- batch queries on host arrays: what the four wrappers below share ----------
    def _batch(self, records: np.ndarray, out_shapes, call):
        """The host side of a batch query.  Uploads `records` ((n, cols) float32
        from _records) to the handle's first device, allocates one int32 output
        per entry of out_shapes (a record's shape; max(n, 1) records, so that a
        bad k still reaches the library), and runs call(d_records, *d_outputs)
        on device addresses (0 for every one when n == 0) between a torch
        synchronize and self.synchronize().  Returns (call's result, the host
        arrays of the outputs' first n records)."""
        import torch
        n = records.shape[0]
        dev = torch.device("cuda", self.multi_info()["devices"][0])
        d_in = torch.from_numpy(records).to(dev)
        d_out = [torch.empty((max(n, 1), *shape), dtype=torch.int32, device=dev) for shape in out_shapes]
        torch.cuda.synchronize(dev)  # the upload ran on torch's stream
        st = call(*[d.data_ptr() if n else 0 for d in (d_in, *d_out)])
        self.synchronize()
        return st, [d[:n].cpu().numpy() for d in d_out]

    # -- ray queries (rt_trace_rays / rt_pick) -----------------------------------
    def trace_rays_device(self, rays_ptr: int, n: int, hits_ptr: int, kind: str = "nearest",
                          stream: Optional[int] = None, stats: bool = False) -> Optional[RtStats]:
        """rt_trace_rays on buffers already on the GPU: n rt_ray (32 bytes each:
        origin, tmin, dir, tmax) at rays_ptr -> n rt_hit (t, sphere) at hits_ptr.
        Asynchronous on `stream` (None: the renderer's own) unless stats."""
        st, st_arg = _stats_arg(stats)
        check(self._lib.rt_trace_rays(self._h, _ptr(rays_ptr), int(n), _QUERY_KINDS[kind],
                                      _ptr(hits_ptr), _ptr(stream), st_arg), self._h)
        return st

    def trace_rays(self, rays, kind: str = "nearest", stats: bool = False):
        """Trace a host (n, 8) float32 array of rays in rt_ray layout (origin xyz,
        tmin, dir xyz, tmax): uploads, runs rt_trace_rays, and returns
        (t (n,) float32, sphere (n,) uint32[, RtStats]).  A miss has t = the
        ray's tmax and sphere = RT_NO_HIT."""
        ra = _records(rays, 8, "rays", "rt_ray")
        st, (hits,) = self._batch(ra, [(2,)], lambda d_rays, d_hits: self.trace_rays_device(
            d_rays, len(ra), d_hits, kind, None, stats))
        t, sphere = _split_pairs(hits)
        return (t, sphere, st) if stats else (t, sphere)

    def pick(self, u: float, v: float):
        """rt_pick: the nearest sphere under image coordinates (u, v) of the current
        camera -> (hit: bool, t, sphere, point (3,) float32)."""
        h = _lib.RtHit()
        pt = np.zeros(3, np.float32)
        check(self._lib.rt_pick(self._h, float(u), float(v), ctypes.byref(h), _fptr(pt)), self._h)
        return h.sphere != _lib.RT_NO_HIT, float(h.t), int(h.sphere), pt

    # -- ordered multi-hit queries (rt_trace_rays_multi / rt_pick_multi) -----------
    def trace_rays_multi_device(self, rays_ptr: int, n: int, k: int, hits_ptr: int,
                                counts_ptr: Optional[int] = None, stream: Optional[int] = None,
                                stats: bool = False) -> Optional[RtStats]:
        """rt_trace_rays_multi on buffers already on the GPU: n rt_ray at rays_ptr ->
        n*k rt_hit at hits_ptr (ray-major, each ray's k nearest by (t, sphere
        index), then {tmax, RT_NO_HIT} fillers) and n uint32 counts at counts_ptr
        (optional).  Asynchronous on `stream` (None: the renderer's own) unless stats."""
        st, st_arg = _stats_arg(stats)
        check(self._lib.rt_trace_rays_multi(self._h, _ptr(rays_ptr), int(n), int(k), _ptr(hits_ptr),
                                            _ptr(counts_ptr), _ptr(stream), st_arg), self._h)
        return st

    def trace_rays_multi(self, rays, k: int, stats: bool = False):
        """The k nearest spheres along each ray of a host (n, 8) float32 array in
        rt_ray layout: uploads, runs rt_trace_rays_multi, and returns
        (t (n, k) float32, sphere (n, k) uint32, count (n,) uint32[, RtStats]).
        Slots past a ray's count hold t = the ray's tmax and sphere = RT_NO_HIT."""
        ra, k = _records(rays, 8, "rays", "rt_ray"), int(k)
        st, (hits, counts) = self._batch(
            ra, [(max(k, 1), 2), ()], lambda d_rays, d_hits, d_counts: self.trace_rays_multi_device(
                d_rays, len(ra), k, d_hits, d_counts, None, stats))
        t, sphere = _split_pairs(hits)
        count = counts.view(np.uint32)
        return (t, sphere, count, st) if stats else (t, sphere, count)

    def pick_multi(self, u: float, v: float, k: int):
        """rt_pick_multi: the k nearest spheres under image coordinates (u, v) of the
        current camera, front to back -> (count, t (k,) float32, sphere (k,) uint32);
        slots past count hold +inf and RT_NO_HIT."""
        k = int(k)
        hits = (_lib.RtHit * max(k, 1))()
        cnt = ctypes.c_uint32(0)
        check(self._lib.rt_pick_multi(self._h, float(u), float(v), k, hits, ctypes.byref(cnt)), self._h)
        t, sphere = _split_pairs(np.frombuffer(hits, np.int32).reshape(-1, 2)[:k])
        return int(cnt.value), t, sphere

    # -- sphere-overlap queries (rt_query_overlaps / rt_overlaps_at) ----------------
    def query_overlaps_device(self, probes_ptr: int, n: int, k: int, indices_ptr: int,
                              counts_ptr: Optional[int] = None, skip_self: bool = False,
                              stream: Optional[int] = None, stats: bool = False) -> Optional[RtStats]:
        """rt_query_overlaps on buffers already on the GPU: n rt_probe (16 bytes each:
        centre, radius; a scene sphere's layout) at probes_ptr -> n*k uint32 at
        indices_ptr (probe-major, the k smallest sphere indices each probe touches,
        ascending, then RT_NO_HIT fillers) and n count words at counts_ptr
        (optional; RT_OVERLAP_MORE set: the probe touches more than k).
        Asynchronous on `stream` (None: the renderer's own) unless stats."""
        st, st_arg = _stats_arg(stats)
        check(self._lib.rt_query_overlaps(self._h, _ptr(probes_ptr), int(n), int(k),
                                          _lib.RT_OVERLAP_SKIP_SELF if skip_self else 0,
                                          _ptr(indices_ptr), _ptr(counts_ptr), _ptr(stream), st_arg),
              self._h)
        return st

    def query_overlaps(self, probes, k: int, skip_self: bool = False, stats: bool = False):
        """The scene spheres each probe of a host (n, 4) float32 array (centre xyz,
        radius) touches: uploads, runs rt_query_overlaps, and returns
        (indices (n, k) uint32, count (n,) uint32, more (n,) bool[, RtStats]).
        Slots past a probe's count hold RT_NO_HIT; more: it touches more than k."""
        pa, k = _records(probes, 4, "probes", "rt_probe"), int(k)
        st, (indices, words) = self._batch(
            pa, [(max(k, 1),), ()], lambda d_probes, d_idx, d_counts: self.query_overlaps_device(
                d_probes, len(pa), k, d_idx, d_counts, skip_self, None, stats))
        indices = indices.view(np.uint32)
        count, more = _overlap_words(words.view(np.uint32))
        return (indices, count, more, st) if stats else (indices, count, more)

    def overlaps_at(self, center, radius: float, k: int):
        """rt_overlaps_at: the scene spheres within `radius` of a point (a brush
        around pick()'s point; radius 0: the spheres that contain it) ->
        (count, indices (k,) uint32, more: bool); slots past count hold RT_NO_HIT."""
        k = int(k)
        c = np.ascontiguousarray(np.asarray(center, np.float32).reshape(3))
        idx = (ctypes.c_uint32 * max(k, 1))()
        cnt = ctypes.c_uint32(0)
        check(self._lib.rt_overlaps_at(self._h, _fptr(c), float(radius), k, idx, ctypes.byref(cnt)),
              self._h)
        count, more = _overlap_words(cnt.value)
        return int(count), np.frombuffer(idx, np.uint32)[:k].copy(), bool(more)

    # -- closest-sphere queries (rt_query_closest / rt_closest_at) ------------------
    def query_closest_device(self, probes_ptr: int, n: int, k: int, near_ptr: int,
                             counts_ptr: Optional[int] = None, skip_self: bool = False,
                             stream: Optional[int] = None, stats: bool = False) -> Optional[RtStats]:
        """rt_query_closest on buffers already on the GPU: n rt_probe (16 bytes each:
        a point and its search radius; a scene sphere's layout) at probes_ptr ->
        n*k rt_near at near_ptr (probe-major, each probe's k nearest spheres by
        (signed surface distance, sphere index), then {the probe's radius,
        RT_NO_HIT} fillers) and n uint32 counts at counts_ptr (optional).
        Asynchronous on `stream` (None: the renderer's own) unless stats."""
        st, st_arg = _stats_arg(stats)
        check(self._lib.rt_query_closest(self._h, _ptr(probes_ptr), int(n), int(k),
                                         _lib.RT_CLOSEST_SKIP_SELF if skip_self else 0,
                                         _ptr(near_ptr), _ptr(counts_ptr), _ptr(stream), st_arg),
              self._h)
        return st

    def query_closest(self, probes, k: int, skip_self: bool = False, stats: bool = False):
        """The k scene spheres nearest each probe of a host (n, 4) float32 array
        (point xyz, search radius; +inf: unbounded): uploads, runs
        rt_query_closest, and returns (dist (n, k) float32, sphere (n, k) uint32,
        count (n,) uint32[, RtStats]).  dist is the signed distance to the
        sphere's surface; slots past a probe's count hold its radius and RT_NO_HIT."""
        pa, k = _records(probes, 4, "probes", "rt_probe"), int(k)
        st, (near, counts) = self._batch(
            pa, [(max(k, 1), 2), ()], lambda d_probes, d_near, d_counts: self.query_closest_device(
                d_probes, len(pa), k, d_near, d_counts, skip_self, None, stats))
        dist, sphere = _split_pairs(near)
        count = counts.view(np.uint32)
        return (dist, sphere, count, st) if stats else (dist, sphere, count)

    def closest_at(self, point, max_dist: float, k: int):
        """rt_closest_at: the k spheres nearest a point within max_dist (a missed
        click snapping to the nearest sphere; math.inf: unbounded) ->
        (count, dist (k,) float32, sphere (k,) uint32); slots past count hold
        max_dist and RT_NO_HIT."""
        k = int(k)
        c = np.ascontiguousarray(np.asarray(point, np.float32).reshape(3))
        near = (_lib.RtNear * max(k, 1))()
        cnt = ctypes.c_uint32(0)
        check(self._lib.rt_closest_at(self._h, _fptr(c), float(max_dist), k, near, ctypes.byref(cnt)),
              self._h)
        dist, sphere = _split_pairs(np.frombuffer(near, np.int32).reshape(-1, 2)[:k])
        return int(cnt.value), dist, sphere

    # -- swept-sphere queries (rt_sweep_spheres / rt_sweep_at / rt_pick_thick) ------
    def sweep_spheres_device(self, rays_ptr: int, n: int, hits_ptr: int, radius: float = 0.0,
                             radii_ptr: Optional[int] = None, entry_only: bool = False,
                             skip_self: bool = False, stream: Optional[int] = None,
                             stats: bool = False) -> Optional[RtStats]:
        """rt_sweep_spheres on buffers already on the GPU: n rt_ray at rays_ptr, each
        the path of the centre of a ball of radius radii_ptr[i] (n floats; None:
        `radius` for every cast) -> n rt_hit at hits_ptr: the first sphere the
        ball touches by (t, sphere index), or {tmax, RT_NO_HIT}.  Asynchronous on
        `stream` (None: the renderer's own) unless stats."""
        st, st_arg = _stats_arg(stats)
        flags = (_lib.RT_SWEEP_ENTRY_ONLY if entry_only else 0) | (_lib.RT_SWEEP_SKIP_SELF if skip_self else 0)
        check(self._lib.rt_sweep_spheres(self._h, _ptr(rays_ptr), _ptr(radii_ptr), float(radius), int(n),
                                         flags, _ptr(hits_ptr), _ptr(stream), st_arg), self._h)
        return st

    def sweep_spheres(self, rays, radius, entry_only: bool = False, skip_self: bool = False,
                      stats: bool = False):
        """The first scene sphere a ball touches while its centre moves along each
        ray of a host (n, 8) float32 array in rt_ray layout (`dir` of unit
        length); `radius` is a scalar or an (n,) array.  Uploads, runs
        rt_sweep_spheres, and returns (t (n,) float32, sphere (n,) uint32[,
        RtStats]).  A miss has t = the cast's tmax and sphere = RT_NO_HIT."""
        ra = _records(rays, 8, "rays", "rt_ray")
        d_radii = None
        if np.ndim(radius) != 0:
            import torch
            rr = np.array(radius, np.float32)
            if rr.shape != (len(ra),):
                raise ValueError("radius must be a scalar or an (n,) float32 array, one per ray")
            # (on torch's stream, like _batch's upload, whose synchronize covers it)
            d_radii = torch.from_numpy(rr).to(torch.device("cuda", self.multi_info()["devices"][0]))
        st, (hits,) = self._batch(ra, [(2,)], lambda d_rays, d_hits: self.sweep_spheres_device(
            d_rays, len(ra), d_hits, 0.0 if d_radii is not None else float(radius),
            d_radii.data_ptr() if d_radii is not None and len(ra) else None, entry_only, skip_self, None, stats))
        t, sphere = _split_pairs(hits)
        return (t, sphere, st) if stats else (t, sphere)

    def sweep_at(self, origin, direction, radius: float, tmax: float = float("inf"),
                 entry_only: bool = False):
        """rt_sweep_at: one ball of `radius` from `origin` along the unit `direction`
        up to tmax (tmin = 0), e.g. a time of impact -> (hit: bool, t, sphere,
        point (3,) float32: the ball's centre at contact)."""
        o = np.ascontiguousarray(np.asarray(origin, np.float32).reshape(3))
        d = np.ascontiguousarray(np.asarray(direction, np.float32).reshape(3))
        h = _lib.RtHit()
        pt = np.zeros(3, np.float32)
        check(self._lib.rt_sweep_at(self._h, _fptr(o), _fptr(d), float(radius), float(tmax),
                                    _lib.RT_SWEEP_ENTRY_ONLY if entry_only else 0, ctypes.byref(h),
                                    _fptr(pt)), self._h)
        return h.sphere != _lib.RT_NO_HIT, float(h.t), int(h.sphere), pt

    def pick_thick(self, u: float, v: float, radius: float):
        """rt_pick_thick: pick() with a cursor of finite `radius` (world units) ->
        (hit: bool, t, sphere, point (3,) float32: the cursor ball's centre at contact)."""
        h = _lib.RtHit()
        pt = np.zeros(3, np.float32)
        check(self._lib.rt_pick_thick(self._h, float(u), float(v), float(radius), ctypes.byref(h), _fptr(pt)),
              self._h)
        return h.sphere != _lib.RT_NO_HIT, float(h.t), int(h.sphere), pt

    # -- first-hit G-buffer (rt_render_gbuffer) -----------------------------------
    def render_gbuffer_device(self, hits_ptr: Optional[int] = None, normals_ptr: Optional[int] = None,
                              albedo_ptr: Optional[int] = None, stream: Optional[int] = None,
                              stats: bool = False) -> Optional[RtStats]:
        """rt_render_gbuffer into buffers already on the GPU, each optional, in frame
        layout (pixel y*W + x): W*H rt_hit (t, sphere) at hits_ptr, W*H float[4]
        normals at normals_ptr, W*H packed RGBA8 at albedo_ptr.  Asynchronous on
        `stream` (None: the renderer's own) unless stats."""
        g = _lib.RtGBuffer(hits_ptr or None, normals_ptr or None, albedo_ptr or None)
        st, st_arg = _stats_arg(stats)
        check(self._lib.rt_render_gbuffer(self._h, ctypes.byref(g), _ptr(stream), st_arg), self._h)
        return st

    def render_gbuffer(self, normals: bool = True, albedo: bool = True, stats: bool = False) -> dict:
        """The first-hit G-buffer of the current size and camera as host arrays:
        {"t": (H, W) float32, "sphere": (H, W) uint32[, "normal": (H, W, 4) float32]
        [, "albedo": (H, W) uint32][, "stats": RtStats]}.  A miss has t = +inf,
        sphere = RT_NO_HIT, a zero normal and albedo 0."""
        import torch
        w, h = self.width, self.height
        dev = torch.device("cuda", self.multi_info()["devices"][0])
        d_hits = torch.empty((h, w, 2), dtype=torch.int32, device=dev)
        d_nrm = torch.empty((h, w, 4), dtype=torch.float32, device=dev) if normals else None
        d_alb = torch.empty((h, w), dtype=torch.int32, device=dev) if albedo else None
        torch.cuda.synchronize(dev)  # the allocations are torch's
        st = self.render_gbuffer_device(d_hits.data_ptr(), d_nrm.data_ptr() if normals else None,
                                        d_alb.data_ptr() if albedo else None, None, stats)
        self.synchronize()
        t, sphere = _split_pairs(d_hits.cpu().numpy())
        out = {"t": t, "sphere": sphere}
        if normals:
            out["normal"] = d_nrm.cpu().numpy()
        if albedo:
            out["albedo"] = d_alb.cpu().numpy().view(np.uint32)
        if stats:
            out["stats"] = st
        return out

    # -- ambient-occlusion layer (rt_render_ao) -------------------------------------
    def render_ao_device(self, rays: int, radius: float, ao_ptr: Optional[int] = None,
                         occluded_ptr: Optional[int] = None, salt: int = 0, stream: Optional[int] = None,
                         stats: bool = False) -> Optional[RtStats]:
        """rt_render_ao into buffers already on the GPU, each optional, in frame
        layout (pixel y*W + x): W*H float32 at ao_ptr (1 = open, a miss 1), W*H
        uint32 occluded counts at occluded_ptr.  `rays` (1, 2, 4, .. 64) any-hit
        rays of length `radius` from every hit pixel.  Asynchronous on `stream`
        (None: the renderer's own) unless stats."""
        p = _lib.RtAoParams(int(rays), float(radius), int(salt) & 0xFFFFFFFF, 0)
        o = _lib.RtAoOut(ao_ptr or None, occluded_ptr or None)
        st, st_arg = _stats_arg(stats)
        check(self._lib.rt_render_ao(self._h, ctypes.byref(p), ctypes.byref(o), _ptr(stream), st_arg), self._h)
        return st

    def render_ao(self, rays: int, radius: float, salt: int = 0, stats: bool = False, filter_passes: int = 0,
                  depth_sigma: float = 0.05, normal_power: int = 5) -> dict:
        """The ambient-occlusion layer of the current size and camera as host arrays:
        {"ao": (H, W) float32, "occluded": (H, W) uint32[, "stats": RtStats]}.
        A pixel that hits nothing has ao = 1 and occluded = 0.  Different salts
        give independent directions: average the layers while the camera rests.
        filter_passes > 0: the G-buffer, the layer and rt_filter_layer over it run
        on one stream, and "ao_filtered": (H, W) float32 is returned beside the
        raw layer (what a viewer shows of a 4-ray layer while the camera moves)."""
        import torch
        w, h = self.width, self.height
        dev = torch.device("cuda", self.multi_info()["devices"][0])
        d_ao = torch.empty((h, w), dtype=torch.float32, device=dev)
        d_occ = torch.empty((h, w), dtype=torch.int32, device=dev)
        if filter_passes:
            d_hits = torch.empty((h, w, 2), dtype=torch.int32, device=dev)
            d_nrm = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
            d_flt = torch.empty((h, w), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)  # the allocations are torch's
        if filter_passes:
            self.render_gbuffer_device(d_hits.data_ptr(), d_nrm.data_ptr())
        st = self.render_ao_device(rays, radius, d_ao.data_ptr(), d_occ.data_ptr(), salt, None, stats)
        if filter_passes:
            self.filter_layer_device(d_ao.data_ptr(), d_flt.data_ptr(), d_hits.data_ptr(), d_nrm.data_ptr(),
                                     filter_passes, 1, depth_sigma, normal_power)
        self.synchronize()
        out = {"ao": d_ao.cpu().numpy(), "occluded": d_occ.cpu().numpy().view(np.uint32)}
        if filter_passes:
            out["ao_filtered"] = d_flt.cpu().numpy()
        if stats:
            out["stats"] = st
        return out

    # -- one-bounce diffuse light layer (rt_render_indirect, rt_add_layer) -------------------
    def render_indirect_device(self, rays: int, radius: float, layer_ptr: Optional[int] = None,
                               occluded_ptr: Optional[int] = None, salt: int = 0, sky_scale: float = 1.0,
                               stream: Optional[int] = None, stats: bool = False) -> Optional[RtStats]:
        """rt_render_indirect into buffers already on the GPU, each optional, in frame
        layout (pixel y*W + x): W*H float32[4] {r, g, b, open share} at layer_ptr
        (16-byte aligned; a miss {0, 0, 0, 1}), W*H uint32 counts of the bounce rays
        that hit at occluded_ptr.  `rays` (1, 2, 4, .. 64) nearest-hit rays of length
        `radius` from every hit pixel, render_ao_device's rays under the same salt;
        each hit is shaded as a frame shades it, an escaped ray brings sky_scale
        times the frames' miss colour.  Asynchronous on `stream` (None: the
        renderer's own) unless stats."""
        p = _lib.RtIndirectParams(int(rays), float(radius), int(salt) & 0xFFFFFFFF, float(sky_scale), 0)
        o = _lib.RtIndirectOut(layer_ptr or None, occluded_ptr or None)
        st, st_arg = _stats_arg(stats)
        check(self._lib.rt_render_indirect(self._h, ctypes.byref(p), ctypes.byref(o), _ptr(stream), st_arg), self._h)
        return st

    def render_indirect(self, rays: int, radius: float, salt: int = 0, sky_scale: float = 1.0,
                        stats: bool = False) -> dict:
        """The one-bounce diffuse layer of the current size and camera as host arrays:
        {"layer": (H, W, 4) float32, "occluded": (H, W) uint32[, "stats": RtStats]}.
        layer[..., :3] is the mean light the bounce rays bring, layer[..., 3] the
        share of them that escaped (render_ao's "ao" under the same parameters)."""
        import torch
        w, h = self.width, self.height
        dev = torch.device("cuda", self.multi_info()["devices"][0])
        d_layer = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
        d_occ = torch.empty((h, w), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)  # the allocations are torch's
        st = self.render_indirect_device(rays, radius, d_layer.data_ptr(), d_occ.data_ptr(), salt, sky_scale, None,
                                         stats)
        self.synchronize()
        out = {"layer": d_layer.cpu().numpy(), "occluded": d_occ.cpu().numpy().view(np.uint32)}
        if stats:
            out["stats"] = st
        return out

    def add_layer_device(self, layer_ptr: int, gain: float = 1.0, albedo_ptr: Optional[int] = None,
                         rgba8_ptr: Optional[int] = None, stream: Optional[int] = None) -> None:
        """rt_add_layer: the W*H float32[4] layer at layer_ptr added into the W*H RGBA8
        pixels at rgba8_ptr (None: the internal framebuffer) in place, r, g and b
        times gain and, with render_gbuffer_device's albedo at albedo_ptr, times the
        pixel's albedo; alpha is kept, the layer's w is not read.  Asynchronous on
        `stream`."""
        check(self._lib.rt_add_layer(self._h, _ptr(rgba8_ptr), _ptr(layer_ptr), _ptr(albedo_ptr), float(gain),
                                     _ptr(stream)), self._h)

    # -- guide-driven layer filter and layer multiply (rt_filter_layer, rt_apply_layer) ----
    def filter_layer_device(self, in_ptr: int, out_ptr: int, hits_ptr: int, normals_ptr: int, passes: int = 3,
                            channels: int = 1, depth_sigma: float = 0.05, normal_power: int = 5,
                            stream: Optional[int] = None, stats: bool = False) -> Optional[RtStats]:
        """rt_filter_layer on buffers already on the GPU, in frame layout: W*H*channels
        float32 from in_ptr to out_ptr (distinct), steered by render_gbuffer_device's
        W*H rt_hit at hits_ptr and W*H float[4] normals at normals_ptr.  Asynchronous
        on `stream` (None: the renderer's own) unless stats."""
        p = _lib.RtFilterParams(int(passes), int(channels), float(depth_sigma), int(normal_power), 0)
        g = _lib.RtGBuffer(hits_ptr or None, normals_ptr or None, None)
        st, st_arg = _stats_arg(stats)
        check(self._lib.rt_filter_layer(self._h, ctypes.byref(p), ctypes.byref(g), _ptr(in_ptr), _ptr(out_ptr),
                                        _ptr(stream), st_arg), self._h)
        return st

    def filter_layer(self, layer, gbuffer: dict, passes: int = 3, depth_sigma: float = 0.05,
                     normal_power: int = 5) -> np.ndarray:
        """A host layer, (H, W) or (H, W, 4) float32, filtered under the guides of
        `gbuffer` (render_gbuffer's dict: "t", "sphere" and "normal") -> the
        filtered layer, same shape.  Uploads, runs rt_filter_layer on the handle's
        first device and waits."""
        import torch
        w, h = self.width, self.height
        a = np.ascontiguousarray(layer, np.float32)
        if a.shape not in ((h, w), (h, w, 4)):
            raise ValueError(f"layer must be ({h}, {w}) or ({h}, {w}, 4) float32")
        hits = np.empty((h, w, 2), np.uint32)
        hits[..., 0] = np.ascontiguousarray(gbuffer["t"], np.float32).view(np.uint32).reshape(h, w)
        hits[..., 1] = np.asarray(gbuffer["sphere"], np.uint32).reshape(h, w)
        nrm = np.ascontiguousarray(gbuffer["normal"], np.float32).reshape(h, w, 4)
        dev = torch.device("cuda", self.multi_info()["devices"][0])
        d_in = torch.from_numpy(a).to(dev)
        d_hits = torch.from_numpy(hits.view(np.int32)).to(dev)
        d_nrm = torch.from_numpy(nrm).to(dev)
        d_out = torch.empty_like(d_in)
        torch.cuda.synchronize(dev)  # the uploads ran on torch's stream
        self.filter_layer_device(d_in.data_ptr(), d_out.data_ptr(), d_hits.data_ptr(), d_nrm.data_ptr(), passes,
                                 1 if a.ndim == 2 else 4, depth_sigma, normal_power)
        self.synchronize()
        return d_out.cpu().numpy()

    def apply_layer_device(self, layer_ptr: int, floor: float = 0.0, rgba8_ptr: Optional[int] = None,
                           stream: Optional[int] = None) -> None:
        """rt_apply_layer: the W*H float32 layer at layer_ptr multiplied into the W*H
        RGBA8 pixels at rgba8_ptr (None: the internal framebuffer) in place,
        m = floor + (1 - floor) * layer; alpha is kept.  Asynchronous on `stream`."""
        check(self._lib.rt_apply_layer(self._h, _ptr(rgba8_ptr), _ptr(layer_ptr), float(floor), _ptr(stream)),
              self._h)

    # -- a layer carried across camera motion (rt_reproject_layer) ----------------------
    def reproject_layer_device(self, hits_ptr: int, cur_ptr: int, out_ptr: int, count_out_ptr: int,
                               history: Optional[dict] = None, channels: int = 1, max_count: float = 32.0,
                               depth_tol: float = 0.05, stream: Optional[int] = None,
                               stats: bool = False) -> Optional[RtStats]:
        """rt_reproject_layer on buffers already on the GPU, in frame layout: this
        frame's W*H*channels float32 layer at cur_ptr, under the current camera's
        W*H rt_hit at hits_ptr, blended with the previous frame's reprojected mean
        into out_ptr, the counts (W*H float32) into count_out_ptr.  history: None
        (no history) or {"hits", "layer", "count": device pointers of the previous
        frame, "pose": 16 floats, "K": 9 floats: the previous camera}.
        Asynchronous on `stream` (None: the renderer's own) unless stats."""
        p = _lib.RtReprojectParams(int(channels), float(max_count), float(depth_tol), 0)
        h_arg = None
        if history is not None:
            pose = np.ascontiguousarray(history["pose"], np.float32).reshape(16)
            K = np.ascontiguousarray(history["K"], np.float32).reshape(9)
            h = _lib.RtHistory(history["hits"] or None, history["layer"] or None, history["count"] or None,
                               (ctypes.c_float * 16)(*pose.tolist()), (ctypes.c_float * 9)(*K.tolist()))
            h_arg = ctypes.byref(h)
        st, st_arg = _stats_arg(stats)
        check(self._lib.rt_reproject_layer(self._h, ctypes.byref(p), _ptr(hits_ptr), h_arg, _ptr(cur_ptr),
                                           _ptr(out_ptr), _ptr(count_out_ptr), _ptr(stream), st_arg), self._h)
        return st

    def reproject_layer(self, layer, hits, history: Optional[dict] = None, max_count: float = 32.0,
                        depth_tol: float = 0.05):
        """Torch tensors on the handle's first device: `layer` (H, W) or (H, W, 4)
        float32, this frame's; `hits` (H, W, 2) int32, render_gbuffer_device's rt_hit
        records under the current camera; history: None or {"hits", "layer",
        "count": the previous frame's tensors (count (H, W) float32), "pose", "K":
        the previous camera} -> (out, count), new tensors.  Every tensor must be
        contiguous, of the handle's current size (the history's layer of `layer`'s
        shape) and on its first device: ValueError otherwise, before anything runs.
        Runs rt_reproject_layer and waits.  Feed (hits, out, count) and camera() back
        as the next history."""
        import torch
        w, h = self.width, self.height
        dev = torch.device("cuda", self.multi_info()["devices"][0])

        def want(name, a, shapes, dtype):
            """`a` is a contiguous tensor of one of `shapes` and `dtype` on the handle's first device:
            anything else would make the kernel read past a buffer's end or another device's memory."""
            if (not isinstance(a, torch.Tensor) or tuple(a.shape) not in shapes or a.dtype != dtype
                    or a.device != dev or not a.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape "
                                 f"{' or '.join(map(str, shapes))} on {dev}")

        want("layer", layer, ((h, w), (h, w, 4)), torch.float32)
        want("hits", hits, ((h, w, 2),), torch.int32)
        channels = 1 if layer.dim() == 2 else 4
        if history is not None:
            want("history['hits']", history["hits"], ((h, w, 2),), torch.int32)
            want("history['layer']", history["layer"], (tuple(layer.shape),), torch.float32)
            want("history['count']", history["count"], ((h, w),), torch.float32)
            if np.asarray(history["pose"]).size != 16 or np.asarray(history["K"]).size != 9:
                raise ValueError("history['pose'] must hold 16 floats and history['K'] 9")
        out = torch.empty_like(layer)
        count = torch.empty((h, w), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)  # the inputs were made on torch's streams
        hist = None
        if history is not None:
            hist = dict(hits=history["hits"].data_ptr(), layer=history["layer"].data_ptr(),
                        count=history["count"].data_ptr(), pose=history["pose"], K=history["K"])
        self.reproject_layer_device(hits.data_ptr(), layer.data_ptr(), out.data_ptr(), count.data_ptr(), hist,
                                    channels, max_count, depth_tol)
        self.synchronize()
        return out, count

    def reset_accumulation(self) -> None:
        """Progressive mode: the next frame starts from zero samples."""
        check(self._lib.rt_reset_accumulation(self._h), self._h)

    def synchronize(self) -> None:
        check(self._lib.rt_synchronize(self._h), self._h)

    def readback(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), np.uint8)
        check(self._lib.rt_readback(self._h, _vptr(out), None), self._h)
        return out

    def readback_radiance(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), np.float32)
        check(self._lib.rt_readback(self._h, None, _vptr(out)), self._h)
        return out

    def stream_ptr(self) -> int:
        """The renderer's own hipStream_t (what stream=None means)."""
        return int(self._lib.rt_stream(self._h) or 0)

    def framebuffer_ptr(self) -> int:
        return int(self._lib.rt_framebuffer(self._h) or 0)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.rt_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
