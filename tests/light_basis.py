"""The frame's light direction and light-plane basis restated in numpy: the one
copy the tests share (tests/test_gpu_occluders.py's pair rule, and
tests/test_frame_math.py, which checks it against the C++ bit for bit)."""
import numpy as np


def kernel_light(ld):
    """FrameArgs::L as rt_frame.cpp fill_frame_args makes it, and the light-plane
    basis {e1, e2} of rt_frame_math.h light_plane_basis (f32 values, as f64)."""
    ld = np.asarray(ld, np.float32)
    ll = np.sqrt(ld[0] * ld[0] + ld[1] * ld[1] + ld[2] * ld[2], dtype=np.float32)
    L = (-(ld / ll)).astype(np.float32)
    l = L.astype(np.float64)
    l /= np.linalg.norm(l)
    k = int(np.argmin(np.abs(l)))      # first of the smallest, like the host loop
    e1 = np.zeros(3)
    e1[k] = 1.0
    e1 -= l[k] * l
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(l, e1)
    return L, e1.astype(np.float32).astype(np.float64), e2.astype(np.float32).astype(np.float64)
