"""CPU: the host's table of factor families (obvi-slam_amd/csrc/ba_handle.h: families(), its evaluate layout, reduce_small_families()) against an independent
numpy statement of the same bookkeeping.  The table decides where every kernel of obvi_ba_evaluate writes its residuals and norms, and the reduced-program
routine decides which blocks are variables of a solve and how many residuals it reports; a slip in either is silent on the device.  tests/factor_families_shim.cpp
runs both on a default-constructed handle whose host mirrors it fills: no device, no HIP call.  The reprojection factors appear in the layout only: their share of the
reduced program is a loop of its own in each of the routine's two callers, next to uploads that need a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers

LIB = os.path.join(helpers.ROOT, "tests", "libfactorfamilies.so")
TYPES = (0, 2, 3, 4, 5, 9, 10)   # evaluate order: reprojection, bbox, shape prior, LTM prior, relative pose, map pair prior, map group prior
U8, U32, I64 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def shim():
    src = os.path.join(helpers.ROOT, "tests", "factor_families_shim.cpp")
    csrc = os.path.join(helpers.ROOT, "obvi-slam_amd", "csrc")
    hdrs = [os.path.join(csrc, h) for h in ("ba_handle.h", "ba_device.h", "ba_math.h", "host_util.h")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-w", "-o", LIB, src])
    lib = C.CDLL(LIB)
    lib.ff_create.restype = C.c_void_p
    lib.ff_reduce.restype = C.c_int64
    return lib


def u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def problem(P=0, L=0, O=0, pose_const=(), object_const=(), rp=((), ()), bb=((), ()), sp=(), lt=(), rl=((), ()), mp=((), ()), mg=(), shared=None, inactive=None):
    """A problem as the host mirrors hold it.  rp: (pose, point); bb: (object, pose); sp, lt: objects; rl: (pose a, pose b); mp: (object a, object b); mg: member lists.
    pose_const / object_const: indices of the constant blocks; inactive: {type: indices of masked factors}; shared: per-object flags or None."""
    inactive = inactive or {}
    n = {0: len(rp[0]), 2: len(bb[0]), 3: len(sp), 4: len(lt), 5: len(rl[0]), 9: len(mp[0]), 10: len(mg)}
    active = {t: np.ones(n[t], np.uint8) for t in TYPES}
    for t, idx in inactive.items():
        active[t][list(idx)] = 0
    pc, oc = np.zeros(P, np.uint8), np.zeros(O, np.uint8)
    pc[list(pose_const)] = 1; oc[list(object_const)] = 1
    return dict(P=P, L=L, O=O, pose_const=pc, object_const=oc, rp=rp, bb=bb, sp=sp, lt=lt, rl=rl, mp=mp, mg=[list(g) for g in mg], shared=shared, n=n, active=active)


def fill(shim, h, q):
    shim.ff_set_blocks(C.c_void_p(h), C.c_int64(q["P"]), C.c_int64(q["L"]), C.c_int64(q["O"]), u8(q["pose_const"]).ctypes.data_as(U8), u8(np.zeros(q["L"])).ctypes.data_as(U8),
                       u8(q["object_const"]).ctypes.data_as(U8))

    def two(fn, t, a, b):
        a, b = u32(a), u32(b)
        fn(C.c_void_p(h), C.c_int64(len(a)), a.ctypes.data_as(U32), b.ctypes.data_as(U32), q["active"][t].ctypes.data_as(U8))

    def one(fn, t, a):
        a = u32(a)
        fn(C.c_void_p(h), C.c_int64(len(a)), a.ctypes.data_as(U32), q["active"][t].ctypes.data_as(U8))
    two(shim.ff_set_reproj, 0, *q["rp"]); two(shim.ff_set_bbox, 2, *q["bb"]); one(shim.ff_set_shape, 3, q["sp"]); one(shim.ff_set_ltm, 4, q["lt"])
    two(shim.ff_set_relpose, 5, *q["rl"]); two(shim.ff_set_pairs, 9, *q["mp"])
    ptr = np.concatenate([[0], np.cumsum([len(g) for g in q["mg"]])]).astype(np.int64)
    members = u32([o for g in q["mg"] for o in g])
    shim.ff_set_groups(C.c_void_p(h), C.c_int64(len(q["mg"])), ptr.ctypes.data_as(I64), members.ctypes.data_as(U32), q["active"][10].ctypes.data_as(U8))
    shim.ff_set_shared(C.c_void_p(h), None if q["shared"] is None else u8(q["shared"]).ctypes.data_as(U8))


# ---- the numpy statement ---------------------------------------------------------------------------------------------------------------------
def want_families(q, od):
    """Per type: count, residual rows, rows per factor (0: per group), block widths of debug_linearize, largest pose / point / object / camera index (-1: none)."""
    def top(*arrays):
        return max([int(np.max(a)) for a in arrays if len(a)], default=-1)
    n = q["n"]
    return {0: (n[0], 2 * n[0], 2, 6, 3, top(q["rp"][0]), top(q["rp"][1]), -1, 0 if n[0] else -1),
            2: (n[2], 4 * n[2], 4, od, 6, top(q["bb"][1]), -1, top(q["bb"][0]), 1 if n[2] else -1),
            3: (n[3], 3 * n[3], 3, od, 0, -1, -1, top(q["sp"]), -1),
            4: (n[4], od * n[4], od, od, 0, -1, -1, top(q["lt"]), -1),
            5: (n[5], 6 * n[5], 6, 6, 6, top(*q["rl"]), -1, -1, -1),
            9: (n[9], 2 * od * n[9], 2 * od, od, od, -1, -1, top(*q["mp"]), -1),
            10: (n[10], od * sum(len(g) for g in q["mg"]), 0, 0, 0, -1, -1, top(*q["mg"]) if q["mg"] else -1, -1)}


def want_reduced(q, od):
    """Residual rows of the reduced program and the blocks in use, every family but the reprojection factors: a factor counts unless all its blocks are constant
    (Ceres: Program::RemoveFixedBlocks), its variable blocks are in use; a group counts whole as soon as one member varies; shared objects are in use."""
    pose_used, obj_used, nres = set(), set(), 0
    pc, oc, act = q["pose_const"], q["object_const"], q["active"]
    factors = [(t, i, rows, blocks) for t, rows, lists in ((2, 4, [("o", q["bb"][0]), ("p", q["bb"][1])]), (3, 3, [("o", q["sp"])]), (4, od, [("o", q["lt"])]),
                                                            (5, 6, [("p", q["rl"][0]), ("p", q["rl"][1])]), (9, 2 * od, [("o", q["mp"][0]), ("o", q["mp"][1])]))
               for i in range(q["n"][t]) for blocks in [[(kind, int(idx[i])) for kind, idx in lists]]]
    factors += [(10, g, od * len(members), [("o", o) for o in members]) for g, members in enumerate(q["mg"])]
    for t, i, rows, blocks in factors:
        variable = [(kind, j) for kind, j in blocks if not (pc[j] if kind == "p" else oc[j])]
        if not act[t][i] or not variable:
            continue
        nres += rows
        pose_used |= {j for kind, j in variable if kind == "p"}
        obj_used |= {j for kind, j in variable if kind == "o"}
    if q["shared"] is not None:
        obj_used |= set(np.flatnonzero(q["shared"]).tolist())
    return nres, sorted(pose_used), sorted(obj_used)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
RNG = np.random.default_rng(3)
FULL = dict(P=6, L=40, O=6, rp=(RNG.integers(0, 6, 37), RNG.integers(0, 40, 37)), bb=([0, 1, 2, 4, 4], [0, 2, 3, 3, 5]), sp=[1, 3, 4], lt=[5, 2],
            rl=([0, 1, 2, 3, 4], [1, 2, 3, 4, 5]), mp=([0, 2], [1, 3]), mg=([0, 2, 4], [5]))
CASES = {
    "empty": problem(),
    "blocks_without_factors": problem(P=3, L=5, O=2),
    "every_family": problem(**FULL),
    "inactive_in_every_family": problem(**FULL, inactive={0: [0, 36], 2: [1, 4], 3: [0], 4: [1], 5: [0, 2], 9: [0], 10: [0]}),
    # bbox 0 = (object 0, pose 0), relative pose 0 = (pose 0, pose 1), shape prior of object 1, pair (0, 1): every block constant -- no residuals, nothing marked
    "all_blocks_constant": problem(**FULL, pose_const=[0, 1], object_const=[0, 1]),
    # ... bbox 1 = (object 1, pose 2): constant object, variable pose
    "box_constant_object_variable_pose": problem(**dict(FULL, mp=((), ()), mg=()), object_const=[1]),
    "pair_with_one_constant_object": problem(**dict(FULL, bb=((), ()), sp=(), lt=(), mg=()), object_const=[3]),            # pair (2, 3)
    "group_all_members_constant": problem(**dict(FULL, bb=((), ()), sp=(), lt=(), mp=((), ())), object_const=[0, 2, 4]),   # group {0, 2, 4}: 0 rows
    "group_one_variable_member": problem(**dict(FULL, bb=((), ()), sp=(), lt=(), mp=((), ())), object_const=[0, 4]),       # ... all 3 od rows, only object 2 marked
    # objects 3 and 5 are touched by no factor here; 5 is constant as well (the flag marks it in use all the same: constness is applied behind the routine)
    "shared_objects_nothing_touches": problem(**dict(FULL, sp=[1], lt=[2], mp=((), ()), mg=()), object_const=[5], shared=[0, 0, 0, 1, 0, 1]),
    "everything_constant": problem(**FULL, pose_const=range(6), object_const=range(6)),
}


@pytest.mark.parametrize("od", [7, 9])
@pytest.mark.parametrize("case", sorted(CASES))
def test_table_layout_and_reduced_program(shim, case, od):
    q = CASES[case]
    h = shim.ff_create(C.c_int32(od))
    try:
        fill(shim, h, q)
        want = want_families(q, od)
        out = (C.c_int64 * 10)()
        for place, t in enumerate(TYPES):
            assert shim.ff_family(C.c_void_p(h), C.c_int32(t), out) == place
            assert tuple(out) == (t,) + want[t], (t, tuple(out), want[t])
        for t in (-1, 1, 6, 7, 8, 11):
            assert shim.ff_family(C.c_void_p(h), C.c_int32(t), out) == -1
        slot, row = (C.c_int64 * 8)(), (C.c_int64 * 8)()
        shim.ff_layout(C.c_void_p(h), slot, row)
        assert list(slot) == [0] + list(np.cumsum([want[t][0] for t in TYPES])) and list(row) == [0] + list(np.cumsum([want[t][1] for t in TYPES]))
        nres, pose_used, obj_used = want_reduced(q, od)
        for as_replan in (0, 1, 1, 0):       # the full plan's way and the mask-only re-plan's (twice: its scratch survives a call), same inputs: one answer
            pu, ou = np.full(q["P"], 9, np.uint8), np.full(q["O"], 9, np.uint8)
            got = shim.ff_reduce(C.c_void_p(h), C.c_int32(as_replan), pu.ctypes.data_as(U8), ou.ctypes.data_as(U8))
            assert got == nres and set(pu) <= {0, 1} and set(ou) <= {0, 1}
            assert list(np.flatnonzero(pu)) == pose_used and list(np.flatnonzero(ou)) == obj_used, (as_replan, pu, ou)
    finally:
        shim.ff_destroy(C.c_void_p(h))


def test_the_cases_say_what_their_names_say():
    """The numpy statement on the cases that were picked for one property each: the property, spelled out."""
    od = 7
    every = want_reduced(CASES["every_family"], od)
    assert every == (4 * 5 + 3 * 3 + od * 2 + 6 * 5 + 2 * od * 2 + od * 4, [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5])
    assert want_reduced(CASES["inactive_in_every_family"], od)[0] == 4 * 3 + 3 * 2 + od + 6 * 3 + 2 * od + od
    assert want_reduced(CASES["all_blocks_constant"], od)[0] == every[0] - 4 - 6 - 3 - 2 * od
    assert want_reduced(CASES["box_constant_object_variable_pose"], od) == (4 * 5 + 3 * 2 + od * 2 + 6 * 5, [0, 1, 2, 3, 4, 5], [0, 2, 3, 4, 5])
    assert want_reduced(CASES["pair_with_one_constant_object"], od) == (6 * 5 + 2 * od * 2, [0, 1, 2, 3, 4, 5], [0, 1, 2])
    assert want_reduced(CASES["group_all_members_constant"], od) == (6 * 5 + od, [0, 1, 2, 3, 4, 5], [5])
    assert want_reduced(CASES["group_one_variable_member"], od) == (6 * 5 + od * 4, [0, 1, 2, 3, 4, 5], [2, 5])
    assert want_reduced(CASES["shared_objects_nothing_touches"], od)[2] == [0, 1, 2, 3, 4, 5]
    assert want_reduced(CASES["everything_constant"], od) == (0, [], []) and want_reduced(CASES["empty"], od) == (0, [], [])
