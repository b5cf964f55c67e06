"""CPU: deterministic mode's partial-sum slots (obvi-slam_amd/csrc/ba_device.h).  Workgroup b of a kernel that leaves partial sums stores at
scal[SC_COUNT + slot * stride + b] without a bounds check, so the stride the handle gives the slots (det_slots_needed, rounded up by
ensure_det_slots) must cover the grid of every such launch.  Both come from the same grid functions; tests/detslots_shim.cpp exposes them
and this test holds the slot size against every grid over problem shapes of every kind, at every lane count of the back-substitution."""
import ctypes as C
import os
import subprocess

import pytest

import helpers

LIB = os.path.join(helpers.ROOT, "tests", "libdetslots.so")
LANES = (1, 2, 4, 8, 16, 32)   # what launch_backsub_apply may take per feature (Knobs::backsub_lanes, or its own choice)


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(helpers.ROOT, "tests", "detslots_shim.cpp")
    hdrs = [os.path.join(helpers.ROOT, "obvi-slam_amd", "csrc", h) for h in ("ba_device.h", "ba_math.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-w", "-o", LIB, src])
    lib = C.CDLL(LIB)
    lib.detslots_needed.restype = C.c_int64
    return lib


def counts(P=0, L=0, O=0, od=7, n_rp=0, n_point_waves=0, n_long_points=0, n_bb=0, n_sp=0, n_lt=0, n_rl=0):
    return (C.c_int64 * 11)(P, L, O, od, n_rp, n_point_waves, n_long_points, n_bb, n_sp, n_lt, n_rl)


# (P, L, O, n_rp, n_point_waves, n_long_points, n_bb, n_sp, n_lt, n_rl)
SHAPES = {
    "pose_heavy": (40000, 5000, 20, 60000, 1200, 0, 300, 20, 0, 39999),
    "object_heavy_ltm_only": (1000, 10000, 200000, 100000, 1600, 0, 0, 0, 200000, 999),
    "box_heavy": (2000, 20000, 5000, 300000, 5000, 0, 600000, 5000, 5000, 1999),
    "long_track_points": (3000, 300000, 50, 9000000, 0, 300000, 0, 0, 0, 2999),
    "sliding_window": (10, 400, 6, 3000, 60, 0, 40, 6, 6, 9),
    "config3_like": (1200, 250000, 1500, 3000000, 50000, 2000, 30000, 1500, 1500, 1199),
    "points_only": (0, 70000, 0, 0, 0, 0, 0, 0, 0, 0),
    "objects_only": (0, 0, 300000, 0, 0, 0, 0, 300000, 0, 0),
    "poses_only": (500000, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    "empty": (0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
}


@pytest.mark.parametrize("od", [7, 9])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_slots_cover_every_reducing_grid(shim, shape, od):
    P, L, O, n_rp, n_waves, n_long, n_bb, n_sp, n_lt, n_rl = SHAPES[shape]
    c = counts(P, L, O, od, n_rp, n_waves, n_long, n_bb, n_sp, n_lt, n_rl)
    need = shim.detslots_needed(c)
    grids = (C.c_int64 * 8)()
    for lanes in LANES:
        shim.detslots_grids(c, lanes, grids)
        assert max(grids) <= need, (lanes, list(grids), need)
    assert need >= 1                                  # (an empty problem too: the stride is also deterministic mode's flag)


def test_nine_parameter_objects_get_sixteen_threads_per_diagonal_block(shim):
    # 1 000 poses, 200 000 9-parameter objects with LTM priors and no boxes: k_reduced_diag runs 16 threads per block, 16 * 201 000 / 256
    # = 12 563 workgroups (at 8 per block, the count the slots once took for every od, 6 282 -- and a stride of 8 192 they overran)
    P, L, O, n_rp, n_waves, n_long, n_bb, n_sp, n_lt, n_rl = SHAPES["object_heavy_ltm_only"]
    grids = (C.c_int64 * 8)()
    for od, diag in ((7, 6282), (9, 12563)):
        c = counts(P, L, O, od, n_rp, n_waves, n_long, n_bb, n_sp, n_lt, n_rl)
        shim.detslots_grids(c, 1, grids)
        assert grids[3] == diag
        assert shim.detslots_needed(c) >= diag
