"""The host arithmetic the bit-exact images depend on (csrc/rt_frame_math.h),
on the CPU: tests/native/frame_math_dump.cpp, built with the address and
undefined-behaviour sanitizers, prints each function's result for inputs given
as bit patterns, and the results are compared with numpy restatements (the
ones the GPU tests use) and with each function's contract.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import raytracingstudy_amd as rt
from light_basis import kernel_light
from test_cam8_screen import _in_frame
from test_cam_screen import CAMERAS
from test_gpu_occluders import LIGHT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENTRE = (0.64, 0.64, 0.64)
ROOT_MIN, ROOT_MAX = (0.0, 0.0, 0.0), (1.28, 1.28, 1.28)   # rt_octree_params_default
CAM_GATE = 3.0                                             # kOccCamGate


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bin") / "frame_math_dump")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "frame_math_dump.cpp")])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr   # a sanitizer report fails the test
        return r.stdout.split()
    return run


def _f32(values):
    return ["%08x" % b for b in np.asarray(values, np.float32).reshape(-1).view(np.uint32)]


def _f64(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _floats(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


# ---- light-plane basis -------------------------------------------------------

@pytest.mark.parametrize("light", [LIGHT, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 1.0, 1.0)])
def test_light_plane_basis_equals_the_tests_restatement(dump, light):
    """The same IEEE f64 operations in the same order as light_basis.kernel_light:
    equal bit for bit (the GPU occluder tests rely on that restatement)."""
    L, e1, e2 = kernel_light(light)
    got = _floats(dump("light", *_f32(L)))
    want = np.concatenate([e1, e2]).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- image-plane basis -------------------------------------------------------

def _look_at(o):
    """R (column-major, R[c*3+r]; the camera looks along its third column) of a
    camera at o aimed at the scene centre, f32."""
    z = np.asarray(CENTRE, np.float64) - np.asarray(o, np.float64)
    if np.linalg.norm(z) < 1e-9:                      # the camera AT the centre
        z = np.array([0.3, -0.2, 1.0])
    z /= np.linalg.norm(z)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    return np.concatenate([x, np.cross(z, x), z]).astype(np.float32)


def _ray(K, R, u, v):
    """getRay's direction before normalisation, in f64 from the f32 K and R, in
    cam8_basis's order of operations."""
    K, R = K.astype(np.float64), R.astype(np.float64)
    dx, dy = (u - K[2]) / K[0], (v - K[5]) / K[4]
    return np.array([R[i] * dx + R[3 + i] * dy + R[6 + i] for i in range(3)])


def _cam8(dump, w, h, K, R):
    out = dump("cam8", w, h, *_f32(K), *_f32(R))
    return int(out[0]), _floats(out[1:])


@pytest.mark.parametrize("w,h", [(96, 64), (1920, 1080)])
@pytest.mark.parametrize("o", CAMERAS)
def test_image_plane_basis(dump, o, w, h):
    K = rt.resize_intrinsic(w, h).reshape(9)
    R = _look_at(o)
    ok, B = _cam8(dump, w, h, K, R)
    # rows: f64-orthonormal vectors rounded to f32, so each dot product is off
    # by at most 3 * 2^-24 * sqrt(3) = 3.1e-7
    B64 = B.astype(np.float64).reshape(3, 3)
    assert np.abs(B64 @ B64.T - np.eye(3)).max() <= 1e-6
    # the third row: the normalised ray through the image centre
    z = _ray(K, R, 0.5 * w, 0.5 * h)
    z = z / np.sqrt(z[0] * z[0] + z[1] * z[1] + z[2] * z[2])
    assert np.array_equal(B[6:].view(np.uint32), z.astype(np.float32).view(np.uint32))
    # ok: the frame contract at the four image corners
    corners = np.array([_ray(K, R, u, v) for v in (0.0, float(h)) for u in (0.0, float(w))])
    assert ok == int(_in_frame(B, corners).all()) == 1


def test_image_plane_basis_refuses_a_frame_wider_than_its_contract(dump):
    """(B d).z >= 0.1 |B d| means a ray within atan(sqrt(99)) of the centre ray.
    With the principal point in the middle a corner ray's tangent is half the
    frame's diagonal over the focal length: a focal length of half the
    diagonal's bound puts the corners at twice the tangent allowed."""
    w, h = 96, 64
    K = rt.resize_intrinsic(w, h).reshape(9).copy()
    K[0] = K[4] = np.float32(0.5 * np.hypot(0.5 * w, 0.5 * h) / np.sqrt(99.0))
    R = _look_at(CAMERAS[0])
    ok, B = _cam8(dump, w, h, K, R)
    corners = np.array([_ray(K, R, u, v) for v in (0.0, float(h)) for u in (0.0, float(w))])
    assert not _in_frame(B, corners).any()
    assert ok == 0


# ---- superblock order --------------------------------------------------------

@pytest.mark.parametrize("nx,ny", [(1, 1), (4, 4), (8, 8), (5, 3), (30, 17)])
def test_hilbert_order(dump, nx, ny):
    order = [int(t) for t in dump("hilbert", nx, ny)]
    assert sorted(order) == list(range(nx * ny))
    if nx == ny and nx & (nx - 1) == 0:
        xy = np.array([(i % nx, i // nx) for i in order])
        assert (np.abs(np.diff(xy, axis=0)).sum(axis=1) == 1).all()


# ---- root reach and the far-camera gate ---------------------------------------

def _gate(dump, o, reach):
    return int(dump("gate", *_f32(o), *_f32(ROOT_MIN), *_f32(ROOT_MAX), _f64(CAM_GATE * (reach + 1e-4)))[0])


def test_root_reach_and_camera_gate(dump):
    reach = struct.unpack("<d", struct.pack("<Q", int(dump("reach", *_f32(ROOT_MIN), *_f32(ROOT_MAX))[0], 16)))[0]
    far = np.float32(1.28).astype(np.float64)
    assert reach == np.sqrt(far * far + far * far + far * far)
    assert _gate(dump, (0.64, 0.64, 2.2), reach) == 1          # the scene pose
    diag = float(np.linalg.norm(np.subtract(ROOT_MAX, ROOT_MIN)))
    assert _gate(dump, (0.0, 0.0, 10.0 * diag), reach) == 0
    assert _gate(dump, (np.nan, 0.64, 2.2), reach) == 0


# ---- pixel-set signature -------------------------------------------------------

def test_pixel_set_signature(dump):
    """Progressive sums start over when the signature changes: the full frame's
    is 1, a tile list's never is, and it depends on the ids, their order and
    the tile size."""
    sigs = [int(dump("sig", *a)[0]) for a in (("frame",), (64, 0, 1, 2), (64, 0, 2, 1), (128, 0, 1, 2),
                                              (64, 0, 1))]
    assert sigs[0] == 1 and len(set(sigs)) == len(sigs) and all(s & 2 for s in sigs[1:])
