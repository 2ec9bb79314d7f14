"""tests/native/bins_math_dump.cpp compiled and run for the tests that restate
the screen-space bins on the CPU (test_bins_cpu.py, test_plain_fuzz_cpu.py,
test_gpu_plain_fuzz.py): a stand-alone program built with the address and
undefined-behaviour sanitizers that prints csrc/rt_bins_math.h's results.
Floats travel as hexadecimal bit patterns."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPPED, BINNED, WIDE = 0, 1, 2


def build_dump(d):
    """Compile the program into directory `d`; returns run(*args) -> stdout.
    A sanitizer report fails the caller's test."""
    exe = str(d / "bins_math_dump")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "bins_math_dump.cpp")])

    def run(*args):
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr   # a sanitizer report fails the test
        return r.stdout
    run.dir = d
    return run


def f32_args(values):
    return ["%08x" % b for b in np.asarray(values, np.float32).reshape(-1).view(np.uint32)]


def f64_arg(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def cam_args(pose, K):
    P = np.asarray(pose, np.float32).reshape(4, 4)
    R = P[:3, :3].reshape(-1)          # R[c*3+r] = pose[c*4+r]
    return f32_args(np.asarray(K, np.float32).reshape(-1)) + f32_args(R) + f32_args(P[3, :3])


def rects(dump, sp, pose, K, w, h, shrink=1.0):
    """Per sphere: class, rectangle (x0, y0, x1, y1) and near bound (f32)."""
    path = str(dump.dir / "spheres.f32")
    np.ascontiguousarray(sp, np.float32).tofile(path)
    rows = np.array([[int(t, 16) if i == 5 else int(t) for i, t in enumerate(line.split())]
                     for line in dump("rect", w, h, f64_arg(shrink), *cam_args(pose, K), path).splitlines()],
                    np.int64).reshape(-1, 6)
    near = rows[:, 5].astype(np.uint32).view(np.float32)
    return rows[:, 0], rows[:, 1:5], near


def frame_gate(dump, pose, K, w, h):
    """Whether a w x h frame of this camera may use bins: the host's gate
    (bins_camera_ok and cam8_basis, rt_bins_host.cpp screen_bins)."""
    return dump("framegate", w, h, *cam_args(pose, K)).strip() == "1"
