"""Helpers to build ShapeRec blobs (box2d-mt_amd/csrc/b2d_collide.h) for the CPU probe of the device math, and the loaders of
the probe libraries."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_SRC = os.path.join(ROOT, "tests", "probe", "host_probe.cpp")
PROBE_CASES = os.path.join(ROOT, "tests", "probe", "probe_cases.h")
PROBE_LIB = os.path.join(ROOT, "tests", "probe", "libhost_probe.so")
DEVICE_PROBE_LIB = os.path.join(ROOT, "tests", "probe", "libdevice_probe.so")
PRIMS_PROBE_LIB = os.path.join(ROOT, "tests", "probe", "libprims_probe.so")

CIRCLE, EDGE, POLYGON = 0, 1, 2


def build_probe():
    hdrs = [os.path.join(ROOT, "box2d-mt_amd", "csrc", h) for h in ("b2d_math.h", "b2d_collide.h", "b2d_solver.h", "b2d_toi.h",
                                                                     "b2d_shape_geom.h", "b2d_shapecast.h")]
    newest = max(os.path.getmtime(p) for p in hdrs + [PROBE_SRC, PROBE_CASES])
    if not os.path.exists(PROBE_LIB) or os.path.getmtime(PROBE_LIB) < newest:
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared",
                               "-I", os.path.join(ROOT, "box2d-mt_amd", "csrc"), "-o", PROBE_LIB, PROBE_SRC])
    return C.CDLL(PROBE_LIB)


def load_prims_probe():
    """tests/probe/prims_probe.hip through ctypes (built by `make -C box2d-mt_amd all`; the caller checks that the file exists
    and has called b2hip.use_torch_hip_runtime()). Every entry returns 0 or a hipError_t, pprobe_scan_run also
    pprobe_scan_aborted_code()."""
    L = C.CDLL(PRIMS_PROBE_LIB)
    ip, up = C.POINTER(C.c_int), C.POINTER(C.c_uint32)
    L.pprobe_scan_aborted_code.restype = C.c_int
    L.pprobe_scan_open.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.pprobe_scan_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.pprobe_scan_epoch.argtypes = [C.c_void_p]
    L.pprobe_scan_epoch.restype = C.c_uint
    L.pprobe_scan_set_epoch.argtypes = [C.c_void_p, C.c_uint]
    L.pprobe_scan_close.argtypes = [C.c_void_p]
    L.pprobe_wave.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, ip, up, ip, up, C.c_int, ip, C.c_int, C.c_int]
    for name in ("pprobe_scan_open", "pprobe_scan_run", "pprobe_scan_set_epoch", "pprobe_scan_close", "pprobe_wave"):
        getattr(L, name).restype = C.c_int
    return L


def shape_rec(kind, count=0, radius=0.0, centroid=(0, 0), verts=(), normals=()):
    buf = np.zeros(38, np.float32)
    iv = buf.view(np.int32)
    iv[0] = kind
    iv[1] = count
    buf[2] = radius
    buf[4:6] = centroid
    v = np.asarray(verts, np.float32).reshape(-1)
    buf[6:6 + v.size] = v
    n = np.asarray(normals, np.float32).reshape(-1)
    buf[22:22 + n.size] = n
    return buf


def polygon_from_ref(ref, verts):
    """Build the polygon record from the reference's own b2PolygonShape::Set output."""
    o = ref.polygon(verts)
    cnt = int(o[0])
    return shape_rec(POLYGON, cnt, 0.01, o[33:35], o[1:1 + 2 * cnt], o[17:17 + 2 * cnt])


def box_rec(hx, hy):
    return shape_rec(POLYGON, 4, 0.01, (0, 0), [-hx, -hy, hx, -hy, hx, hy, -hx, hy], [0, -1, 1, 0, 0, 1, -1, 0])


def circle_rec(px, py, r):
    return shape_rec(CIRCLE, 0, r, (0, 0), [px, py])


def edge_rec(edge10):
    e = np.asarray(edge10, np.float32)
    flags = (1 if e[4] != 0 else 0) | (2 if e[7] != 0 else 0)
    return shape_rec(EDGE, flags, 0.01, (0, 0), [e[0], e[1], e[2], e[3], e[5], e[6], e[8], e[9]])


def proxy_of(rec):
    """(count, verts as 16 floats, radius) of a shape record, as b2dProxy (b2d_toi.h) takes them"""
    iv = rec.view(np.int32)
    n = 1 if iv[0] == CIRCLE else (2 if iv[0] in (EDGE, 3) else int(iv[1]))
    return n, np.ascontiguousarray(rec[6:22]), float(rec[2])


def cast_fields(want7):
    """Which of b2h_probe_shape_cast's 7 outputs a recorded cast defines: a miss only its flag; a hit everything - but for a hit
    without an iteration (the skins touch at the start) the reference's point is uninitialised memory (see
    tests/golden/make_golden_geom.py), so flag, normal, lambda and iterations."""
    if want7[0] == 0:
        return [0]
    return [0, 3, 4, 5, 6] if want7[6] == 0 else list(range(7))
