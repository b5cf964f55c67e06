"""Designed cases for the object side of the reduced system, with the extended-precision reference of tests/schur_cases.py carried over to every family.

tests/schur_cases.py pins the reprojection half of an LM step (point pass, Schur strip, far blocks).  Here is the other half: what the side stream adds for
bounding boxes (type 2), shape priors (3), LTM priors (4) and relative-pose factors (5), and the rows and columns of the objects themselves.  The kernels cut
that work in many places -- four factors per wavefront with 13 (15) of 16 lanes carrying a direction (bbox_lin_lanes, relpose_lin_lanes), sixteen factors per
workgroup (k_bbox_lin_dense), 64 priors per workgroup with the switch from shape to LTM priors inside a wavefront (object_priors_lin), an object's factor list
in 7 (4) strided slices (k_bbox_gather), every scratch slot of a target's list (k_small_gather), blocks of 6 / 7 / 9 rows that straddle a 64-row tile edge
(S_at per entry) -- and the cases FIX which object is seen from which frame by which camera, and which priors and relative-pose factors exist, so that every
cut has a factor on both of its sides.

Scene: the slab of schur_cases (camera looking sideways, 0.1 m per frame), ellipsoids 8 to 20 m in front of it, boxes from synth.project_ellipsoids at the
ground truth plus 3 px noise (every 7th box 40 px off), filler points so that every variable pose is held by reprojection factors.

  lanes   20 poses, stereo, one dissection leaf; leaf_rows() restates the row layout of a single leaf (plan.cpp, place_node: 6 rows per pose, then `od` per
          object in order of first observing frame) and the case is aimed so that a pose block, an object block and an object x pose block with a
          bounding-box factor straddle a multiple of 64 rows.  Variant "d": the long object is seen by both cameras from 14 frames (the atomic route of the
          off-diagonal block, bb_pairs_unique false, and a list of 29); variant "u": no (object, pose) pair twice (the plain-store route) -- with 20 poses that
          object's list is then 18 long, the one thing in which the variants differ beside the tail of the factor count.
  tree    44 poses under OBVI_ND_LEAF=8 / OBVI_ND_G=4: objects inside a leaf, across a separator, from the first and the last frame; relative-pose factors
          inside a leaf, into a separator and in reverse order.  (An object's rows follow those of every pose that sees it, whatever the tree: place_node puts
          a node's objects behind its poses and an object into a node at or above its poses' nodes, so obj_low of bbox_lin_lanes is true by construction.)

Every case carries two masks per family: masks0 (set before the first plan) and masks1 (set after the step on the kept plan), a subset that leaves one pose
and one object without any active factor.

Tolerances: TABLE holds, per case, e(oracle) -- the fp64 oracle against the reference fed with the oracle's own residuals and Jacobians -- and e(second), the
reference fed with the PRODUCT's factor arithmetic compiled for the host (tests/libhostmath.so; the priors are linear) against the oracle-fed one: the bounding-box
and relative-pose Jacobians go through dual arithmetic with a square root of a difference, and the device differs from the reference in that too.  The device's
bound is schur_cases.bound(): max(8 max(e(oracle), e(second)), n_terms 2^-53).  tests/test_object_reference.py measures and prints both."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
from scipy.spatial.transform import Rotation as Rot

import helpers
import schur_cases as sc
import synth
from schur_cases import LD, RADII, _Builder, _lm_lambda, entry_error, exact_zeros  # noqa: F401  (shared with the tests)

FAMILIES = (2, 3, 4, 5)
TILE = 64
SLICES = {7: 7, 9: 4}                # k_bbox_gather: strided slices of an object's list
TILT = 0.1

# name: e(oracle) and e(second) ("second_*") per quantity, and n_terms (tests/test_object_reference.py prints them; it fails if they drift by more than a factor 2)
TABLE = {
    "lanes7d": dict(S=1.2e-14, b=7e-16, second_S=4.9e-15, second_b=8.7e-17, n_terms=350, step_pose=1e-14, step_point=6.5e-15, step_object=6.1e-15, cost=3.4e-16, gradient_max_norm=3.4e-17, gradient_norm=3.8e-17, step_norm=2.2e-15, second_step_pose=4.1e-15, second_step_point=6.2e-15, second_step_object=1.6e-16, second_cost=4.9e-17, second_gradient_max_norm=9.7e-17, second_gradient_norm=2.6e-17, second_step_norm=1.1e-15),
    "lanes7u": dict(S=1.2e-14, b=7.2e-16, second_S=2.3e-15, second_b=7.6e-17, n_terms=342, step_pose=1.1e-14, step_point=4.6e-15, step_object=2.1e-15, cost=1.8e-16, gradient_max_norm=1.5e-16, gradient_norm=3.8e-16, step_norm=2e-15, second_step_pose=4.3e-15, second_step_point=6.2e-15, second_step_object=5.3e-17, second_cost=5e-17, second_gradient_max_norm=9.7e-17, second_gradient_norm=2.5e-17, second_step_norm=1e-15),
    "lanes9d": dict(S=1.2e-14, b=6.9e-16, second_S=5.3e-15, second_b=7e-17, n_terms=350, step_pose=1.5e-14, step_point=5.4e-15, step_object=2.4e-15, cost=3.7e-16, gradient_max_norm=3.5e-16, gradient_norm=4.1e-16, step_norm=9.3e-16, second_step_pose=4.2e-15, second_step_point=6.2e-15, second_step_object=5.8e-17, second_cost=5e-17, second_gradient_max_norm=9.7e-17, second_gradient_norm=2.9e-17, second_step_norm=9e-16),
    "lanes9u": dict(S=1.2e-14, b=7e-16, second_S=2.2e-15, second_b=1.1e-16, n_terms=346, step_pose=2.3e-14, step_point=8.3e-15, step_object=1.5e-15, cost=3.9e-16, gradient_max_norm=4e-17, gradient_norm=3.2e-17, step_norm=1.9e-16, second_step_pose=4.3e-15, second_step_point=6.1e-15, second_step_object=4.8e-17, second_cost=4.9e-17, second_gradient_max_norm=9.7e-17, second_gradient_norm=2.4e-17, second_step_norm=9.5e-16),
    "tree7": dict(S=2e-14, b=2.5e-16, second_S=1.1e-14, second_b=7.7e-17, n_terms=273, step_pose=5.9e-14, step_point=2.1e-14, step_object=3e-15, cost=8e-19, gradient_max_norm=2.3e-16, gradient_norm=6e-16, step_norm=3.3e-15, second_step_pose=1.3e-14, second_step_point=3.8e-15, second_step_object=8.6e-17, second_cost=1.5e-16, second_gradient_max_norm=3.8e-16, second_gradient_norm=3.1e-16, second_step_norm=1e-16),
    "tree9": dict(S=2e-14, b=3.4e-16, second_S=2.4e-14, second_b=7.7e-17, n_terms=273, step_pose=6.6e-14, step_point=1.8e-14, step_object=1.2e-14, cost=1.1e-15, gradient_max_norm=6.3e-16, gradient_norm=5.3e-16, step_norm=9.2e-15, second_step_pose=1.4e-14, second_step_point=3.9e-15, second_step_object=7.6e-17, second_cost=1.5e-16, second_gradient_max_norm=3.9e-16, second_gradient_norm=3.2e-16, second_step_norm=3.8e-17),
}


def bound(case, what):
    return sc.bound(case, what, TABLE)


# ------------------------------------------------------------------------------------------
# the case builder
# ------------------------------------------------------------------------------------------
class _Side:
    """objects and the factors of types 2 to 5 on top of a schur_cases._Builder; tags: "m0" = inactive from the start (and after), "m1" = inactive after the step"""

    def __init__(self):
        self.objs, self.bb, self.sp, self.lt, self.rl = [], [], [], [], []

    def obj(self, name, const=False, inside=None):
        """inside: a pose index -- the ellipsoid is put around that pose's camera (the invalid-ellipse branch for every frame near it)"""
        self.objs.append((name, const, inside))
        return len(self.objs) - 1

    def see(self, o, poses, cams=(0,), tag=""):
        for p in poses:
            for c in cams:
                self.bb.append((o, int(p), int(c), tag))

    def shape(self, o, far=False, tag=""):
        self.sp.append((o, far, tag))

    def ltm(self, o, far=False, tag=""):
        self.lt.append((o, far, tag))

    def rel(self, a, b, tight=False, tag=""):
        assert a != b
        self.rl.append((int(a), int(b), tight, tag))

    def finish(self, base, name, od, seed, drop_pose, drop_obj):
        rng = np.random.Generator(np.random.MT19937(seed))
        prob = dict(base["prob"])
        P, O = len(prob["poses"]), len(self.objs)
        # three distinctly different axes (0.6, 1.0, 1.4 m in a random order, +- 8 cm): a near-symmetric ellipsoid has rotation columns that are small differences
        # of large terms, and an entry of J^T J built from them is then ill-conditioned on the scale of its own terms
        dims = np.stack([rng.permutation([0.6, 1.0, 1.4]) for _ in range(O)]) + rng.uniform(-0.08, 0.08, (O, 3))
        gt = np.concatenate([np.stack([rng.uniform(0.2, 0.1 * P - 0.2, O), rng.uniform(8.0, 20.0, O), rng.uniform(-0.5, 0.5, O), rng.uniform(-np.pi, np.pi, O)], axis=1), dims], axis=1)
        start = gt.copy()
        start[:, 0:3] += rng.normal(size=(O, 3)) * 0.05; start[:, 3] += rng.normal(size=O) * 0.05; start[:, 4:7] *= 1.0 + rng.normal(size=(O, 3)) * 0.03
        inside = np.zeros(O, bool)
        for o, (_, _, at) in enumerate(self.objs):
            if at is not None:
                gt[o, 0:3] = prob["poses"][at, 0:3] + np.array([0.02, 0.03, -0.01]); gt[o, 4:7] = 6.0
                start[o], inside[o] = gt[o], True
        # bounding boxes, sorted by (object, pose, camera) as synth does
        bb = sorted(self.bb, key=lambda x: (x[0], x[1], x[2]))
        bb_obj = np.array([x[0] for x in bb], np.uint32); bb_pose = np.array([x[1] for x in bb], np.uint32); bb_cam = np.array([x[2] for x in bb], np.uint16)
        n_bb = len(bb)
        corners = np.zeros((n_bb, 4))
        for c in range(len(prob["K"])):
            m = bb_cam == c
            px, valid, depth = synth.project_ellipsoids(gt[bb_obj[m]], prob["gt_poses"][bb_pose[m]], prob["K"][c], prob["ext"][c])
            assert (valid == ~inside[bb_obj[m]]).all() and (depth[valid] > 5.0).all()
            px = np.where(valid[:, None], px, np.array([200.0, 300.0, 150.0, 250.0]))
            corners[m] = np.stack([px[:, 0:2].min(axis=1), px[:, 0:2].max(axis=1), px[:, 2:4].min(axis=1), px[:, 2:4].max(axis=1)], axis=1)
        corners += rng.normal(size=corners.shape) * 3.0
        corners[np.arange(n_bb) % 7 == 3] += np.array([40.0, 40.0, -40.0, -40.0])
        bb_cov = np.zeros((n_bb, 4, 4))
        bb_cov[:, np.arange(4), np.arange(4)] = np.array([400.0, 900.0, 1600.0])[np.arange(n_bb) % 3][:, None]
        # shape priors: |r| = 14 (far: past the Huber threshold of 10) or 0.7
        n_sp = len(self.sp)
        sp_obj = np.array([x[0] for x in self.sp], np.uint32)
        sd = np.array([0.1, 0.1, 0.2])[None, :] * (1.0 + 0.5 * (np.arange(n_sp) % 3))[:, None]
        u = rng.normal(size=(n_sp, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        sp_mean = start[sp_obj, 4:7] + sd * u * np.where([x[1] for x in self.sp], 14.0, 0.7)[:, None]
        sp_cov = np.zeros((n_sp, 3, 3)); sp_cov[:, np.arange(3), np.arange(3)] = sd ** 2
        # LTM priors (7-parameter form; synth.nine_dof converts): cov = M M^T, mean = start + s M z with |z| = 1, so |r| = s: 2.5 (far) or 0.3, threshold 1
        n_lt = len(self.lt)
        lt_obj = np.array([x[0] for x in self.lt], np.uint32)
        lt_mean, lt_cov = np.zeros((n_lt, 7)), np.zeros((n_lt, 7, 7))
        for i, (o, far, _) in enumerate(self.lt):
            M = np.diag([0.3, 0.3, 0.3, 0.2, 0.1, 0.1, 0.1]) @ (np.eye(7) + 0.3 * np.tril(rng.normal(size=(7, 7)), -1))
            z = rng.normal(size=7); z /= np.linalg.norm(z)
            lt_mean[i], lt_cov[i] = start[o] + (2.5 if far else 0.3) * (M @ z), M @ M.T
        # relative poses: the ground truth's, with a little noise; loose (0.1 m, 0.05 rad: mostly under the threshold) or tight (4 mm, 2 mrad: far over it)
        n_rl = len(self.rl)
        rl_a = np.array([x[0] for x in self.rl], np.uint32); rl_b = np.array([x[1] for x in self.rl], np.uint32)
        Ra = Rot.from_rotvec(prob["gt_poses"][rl_a, 3:6])
        rl_t = Ra.inv().apply(prob["gt_poses"][rl_b, 0:3] - prob["gt_poses"][rl_a, 0:3]) + rng.normal(size=(n_rl, 3)) * 0.002
        rl_aa = (Ra.inv() * Rot.from_rotvec(prob["gt_poses"][rl_b, 3:6])).as_rotvec() + rng.normal(size=(n_rl, 3)) * 0.001
        sig = np.where(np.array([x[2] for x in self.rl])[:, None], np.array([0.004] * 3 + [0.002] * 3)[None, :], np.array([0.1] * 3 + [0.05] * 3)[None, :])
        rl_cov = np.zeros((n_rl, 6, 6)); rl_cov[:, np.arange(6), np.arange(6)] = sig ** 2
        prob.update(objects=start, gt_objects=gt, object_const=np.array([1 if x[1] else 0 for x in self.objs], np.uint8),
                    bb_obj=bb_obj, bb_pose=bb_pose, bb_cam=bb_cam, bb_corners=corners, bb_cov=bb_cov.reshape(-1, 16), bb_huber=0.5, bb_invalid=1000.0,
                    sp_obj=sp_obj, sp_mean=sp_mean, sp_cov=sp_cov.reshape(-1, 9), sp_huber=10.0,
                    lt_obj=lt_obj, lt_mean=lt_mean, lt_cov=lt_cov.reshape(-1, 49), lt_huber=1.0,
                    rl_a=rl_a, rl_b=rl_b, rl_t=rl_t, rl_aa=rl_aa, rl_cov=rl_cov.reshape(-1, 36), rl_huber=1.0, obj_class=[x[0] for x in self.objs])
        if od == 9:
            prob = synth.nine_dof(prob, tilt=TILT, seed=seed + 1)
        tags = {2: [x[3] for x in bb], 3: [x[2] for x in self.sp], 4: [x[2] for x in self.lt], 5: [x[3] for x in self.rl]}
        masks0 = {0: base["mask0"].copy()}; masks1 = {0: base["mask1"].copy()}
        for t in FAMILIES:
            masks0[t] = np.array([0 if g == "m0" else 1 for g in tags[t]], np.uint8)
            masks1[t] = np.array([0 if g in ("m0", "m1") else 1 for g in tags[t]], np.uint8)
        # after the step: one pose and one object lose every factor
        masks1[0][prob["rp_pose"] == drop_pose] = 0
        masks1[2][(bb_pose == drop_pose) | (bb_obj == drop_obj)] = 0
        masks1[3][sp_obj == drop_obj] = 0; masks1[4][lt_obj == drop_obj] = 0
        masks1[5][(rl_a == drop_pose) | (rl_b == drop_pose)] = 0
        for t in masks0:
            assert (masks1[t] <= masks0[t]).all()
        names = {x[0]: o for o, x in enumerate(self.objs)}
        return dict(name=name, od=od, prob=prob, masks0=masks0, masks1=masks1, names=names, inside=inside, drop_pose=drop_pose, drop_obj=drop_obj)


def block_tables(prob):
    """per family: [(kind, index array)] of its blocks (kind "p" pose / "o" object) and its Huber threshold"""
    return {2: ([("o", prob["bb_obj"]), ("p", prob["bb_pose"])], prob["bb_huber"]), 3: ([("o", prob["sp_obj"])], prob["sp_huber"]),
            4: ([("o", prob.get("lt_obj", np.zeros(0, np.uint32)))], prob.get("lt_huber", 1.0)),
            5: ([("p", prob.get("rl_a", np.zeros(0, np.uint32))), ("p", prob.get("rl_b", np.zeros(0, np.uint32)))], prob.get("rl_huber", 1.0))}


def variable_blocks(prob, masks):
    """the reduced program's rule (Ceres, Program::RemoveFixedBlocks): a block is variable iff it is not constant and an active factor with at least one
    non-constant block touches it"""
    P, O = len(prob["poses"]), len(prob["objects"])
    pose, point = prob["rp_pose"].astype(np.int64), prob["rp_point"].astype(np.int64)
    live = (np.asarray(masks[0]) != 0) & ~((prob["pose_const"][pose] != 0) & (prob["point_const"][point] != 0))
    pose_used = np.bincount(pose[live], minlength=P) > 0
    side = SideTerms(prob, None, masks)
    return (prob["pose_const"] == 0) & (pose_used | side.pose_used), (prob["object_const"] == 0) & side.obj_used


def leaf_rows(prob, masks, od):
    """the row layout of a plan with ONE dissection leaf (plan.cpp, place_node): 6 rows per variable pose in upload order, then `od` per variable object in order
    of its first observing frame (over the active boxes from variable poses; none: last), ties by index.  Returns ({pose: row}, {object: row}, rows in all)."""
    var_pose, var_obj = variable_blocks(prob, masks)
    rank = np.cumsum(var_pose) - 1
    pose_row = {int(p): 6 * int(rank[p]) for p in np.flatnonzero(var_pose)}
    first = {int(o): 1 << 30 for o in np.flatnonzero(var_obj)}
    for i in np.flatnonzero(np.asarray(masks[2]) != 0):
        o, p = int(prob["bb_obj"][i]), int(prob["bb_pose"][i])
        if o in first and var_pose[p]:
            first[o] = min(first[o], int(rank[p]))
    order = sorted(first, key=lambda o: (first[o], o))
    obj_row = {o: 6 * len(pose_row) + od * k for k, o in enumerate(order)}
    return pose_row, obj_row, 6 * len(pose_row) + od * len(order)


def straddles(row, size):
    """the block [row, row + size) lies on both sides of a multiple of 64"""
    return row // TILE != (row + size - 1) // TILE


def list_positions(prob, mask, od):
    """of every inactive bounding-box factor: (position in its object's list, list length, is the last entry of its slice of k_bbox_gather)"""
    out = []
    for o in range(len(prob["objects"])):
        idx = np.flatnonzero(prob["bb_obj"] == o)
        for q, i in enumerate(idx):
            if not mask[i]:
                out.append((q, len(idx), q + SLICES[od] >= len(idx)))
    return out


def aim(case):
    """what the case is aimed at, from its own arrays: list lengths, tails, kinds"""
    prob, m0, od = case["prob"], case["masks0"], case["od"]
    var_pose, var_obj = variable_blocks(prob, m0)
    obj, pose = prob["bb_obj"].astype(int), prob["bb_pose"].astype(int)
    pc, oc = prob["pose_const"][pose] != 0, prob["object_const"][obj] != 0
    pairs = list(zip(obj, pose))
    pos = list_positions(prob, m0[2], od)
    ca, cb = prob["pose_const"][prob["rl_a"]] != 0, prob["pose_const"][prob["rl_b"]] != 0
    rl_pairs = [tuple(sorted(x)) for x in zip(prob["rl_a"].astype(int), prob["rl_b"].astype(int))]
    return dict(n_bb=len(obj), n_sp=len(prob["sp_obj"]), n_lt=len(prob["lt_obj"]), n_rl=len(prob["rl_a"]),
                object_lists=sorted(set(np.bincount(obj, minlength=len(prob["objects"]))[prob["object_const"] == 0])),
                pose_lists=sorted(set(np.bincount(pose, minlength=len(prob["poses"]))[var_pose])),
                bbox=dict(inactive_middle=any(0 < q < n - 1 for q, n, last in pos), inactive_slice_end=any(last and q >= SLICES[od] for q, n, last in pos),
                          const_pose=bool((pc & ~oc).any()), const_object=bool((oc & ~pc).any()), both_const=bool((pc & oc).any()),
                          twice=any(pairs.count(x) > 1 for x in set(pairs)), invalid=bool(case["inside"][obj].any())),
                priors=dict(repeated=bool((np.bincount(prob["sp_obj"]) > 1).any() and (np.bincount(prob["lt_obj"]) > 1).any()), inactive=bool((m0[3] == 0).any() and (m0[4] == 0).any()),
                            const_object=bool((prob["object_const"][prob["sp_obj"]] != 0).any() and (prob["object_const"][prob["lt_obj"]] != 0).any())),
                relpose=dict(consecutive=bool((np.abs(prob["rl_a"].astype(int) - prob["rl_b"].astype(int)) == 1).any()), far=bool((np.abs(prob["rl_a"].astype(int) - prob["rl_b"].astype(int)) > 4).any()),
                             reverse=bool((prob["rl_a"] > prob["rl_b"]).any()), const_first=bool((ca & ~cb).any()), const_second=bool((cb & ~ca).any()), both_const=bool((ca & cb).any()),
                             inactive=bool((m0[5] == 0).any()), same_pair_twice=any(rl_pairs.count(x) > 1 for x in set(rl_pairs))))


# ---- lanes -------------------------------------------------------------------------------------
LANES_CONST = (0, 10, 19)
# extra boxes of the last object: the factor count modulo 4 (the last wavefront) differs across od and variant
LANES_TAIL = {(7, "d"): 3, (9, "d"): 2, (7, "u"): 0, (9, "u"): 2}


@functools.lru_cache(maxsize=None)
def lanes(od, variant):
    P = 20
    b = _Builder("lanes", P, True, 7201, const_poses=LANES_CONST)
    b.fillers(40)
    base = b.finish()
    s = _Side()
    var = [p for p in range(P) if p not in LANES_CONST]                     # 17 variable poses: 102 pose rows; pose 12 is the 11th: rows 60 .. 65
    # objects in the order of their first frame, so that index = place in the leaf: the 3rd starts at row 102 + 2 od, the 4th at 102 + 3 od
    o = s.obj("len1"); s.see(o, [1])
    o = s.obj("len3"); s.see(o, [1, 2, 3])
    o = s.obj("len4"); s.see(o, [1, 5, 12, 13])                              # od = 9: rows 120 .. 128, seen from pose 12
    o = s.obj("len5"); s.see(o, [1, 4, 12, 14, 15])                          # od = 7: rows 123 .. 129, seen from pose 12
    o = s.obj("len6"); s.see(o, [2, 3, 4, 5, 6, 7])
    o = s.obj("len7"); s.see(o, [2, 3, 4, 5, 6, 7, 8])
    o = s.obj("len8"); s.see(o, [2, 3, 4, 6, 7, 8, 9]); s.see(o, [5], tag="m0")       # an inactive factor in the middle of a list
    o = s.obj("len9"); s.see(o, [3, 4, 5, 6, 7, 8, 9, 10, 11])                       # pose 10 is constant
    o = s.obj("len14"); s.see(o, [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15]); s.see(o, [14], tag="m0")   # entry 12: the last of slice 5 (of 7) and of slice 0 (of 4)
    o = s.obj("len15"); s.see(o, [2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17])
    o = s.obj("long")
    if variant == "d":
        s.see(o, [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15], cams=(0, 1)); s.see(o, [16])            # 29, fourteen (object, pose) pairs twice
    else:
        for p in [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 19]:
            s.see(o, [p], cams=(p % 2,))
    o = s.obj("const_object", const=True); s.see(o, [3, 5, 10])                       # constant object; with pose 10: both constant
    o = s.obj("inside", inside=6); s.see(o, [6, 7])                                   # the camera inside the ellipsoid: invalid, zero Jacobians
    s.obj("prior_only")
    o = s.obj("later"); s.see(o, [4, 5, 6, 7, 8][:2 + LANES_TAIL[(od, variant)]])
    O = len(s.objs)
    # priors: 40 shape + 30 LTM: the first workgroup of 64 switches family at lane 40, the second holds 6
    for i in range(40):
        s.shape(i % O, far=i % 3 == 1, tag="m0" if i in (7, 39) else "")
    for i in range(30):
        s.ltm((2 * i + 1) % O, far=i % 4 == 2, tag="m0" if i in (0, 23) else "")
    # relative poses: 25 = 6 groups of four and one factor
    for p in range(P - 1):
        s.rel(p, p + 1, tight=p % 3 == 0)
    s.rel(0, 10); s.rel(2, 15, tight=True); s.rel(5, 12); s.rel(14, 3); s.rel(3, 4, tight=True); s.rel(8, 7)
    s.rl[6] = s.rl[6][:3] + ("m0",)
    case = s.finish(base, "lanes%d%s" % (od, variant), od, 7300 + od, drop_pose=5, drop_obj=s.objs.index(("later", False, None)))
    case["var_poses"] = var
    return case


# ---- tree --------------------------------------------------------------------------------------
TREE_CONST = (0, 1, 42, 43)
TREE_KNOBS = {"OBVI_ND_LEAF": "8", "OBVI_ND_G": "4"}


@functools.lru_cache(maxsize=None)
def tree(od):
    P = 44
    b = _Builder("tree", P, True, 7202, const_poses=TREE_CONST)
    nF = b.n_frames                                                              # 40 frames: pose = frame + 2
    for rep in range(2):                                                         # short tracks: a frame couples to the next two, so the dissection goes deep
        for f in range(nF - 2):
            b.frames("filler", [f, f + 1, f + 2], cams=(0, 1))
    base = b.finish()
    s = _Side()
    q = lambda frames: [f + 2 for f in frames]                                   # noqa: E731
    o = s.obj("leaf_a"); s.see(o, q([0, 1, 2, 3]))
    o = s.obj("leaf_b"); s.see(o, q([9, 10, 11, 13]), cams=(0, 1))
    o = s.obj("leaf_c"); s.see(o, q([22, 23, 25, 26]))
    o = s.obj("leaf_d"); s.see(o, q([34, 35, 36, 38, 39]))
    o = s.obj("across_low"); s.see(o, q([2, 3, 5, 6, 9]))                         # across a low separator
    o = s.obj("across_mid"); s.see(o, q([13, 15, 17, 19, 22])); s.see(o, q([18]), tag="m0")
    o = s.obj("across_high"); s.see(o, q([26, 29, 30, 33]))
    o = s.obj("root"); s.see(o, q([0, 39])); s.see(o, [1, 42])                   # the first and the last frame (and two constant poses)
    o = s.obj("const_object", const=True); s.see(o, q([7, 20])); s.see(o, [0])
    s.obj("prior_only")
    o = s.obj("later"); s.see(o, q([30, 31]))
    O = len(s.objs)
    for i in range(2 * O):
        s.shape(i % O, far=i % 3 == 1)
    for i in range(O):
        s.ltm((3 * i + 1) % O, far=i % 4 == 2, tag="m0" if i == 4 else "")
    for p in range(P - 1):
        s.rel(p, p + 1, tight=p % 3 == 0)
    # inside a leaf, reversed inside a leaf, over a few frames (into or over a separator), the later frame first
    s.rel(q([1])[0], q([3])[0]); s.rel(q([11])[0], q([9])[0]); s.rel(q([3])[0], q([8])[0], tight=True); s.rel(q([26])[0], q([21])[0]); s.rel(q([17])[0], q([16])[0], tight=True)
    s.rel(q([14])[0], q([18])[0], tag="m0")
    case = s.finish(base, "tree%d" % od, od, 7400 + od, drop_pose=q([31])[0], drop_obj=s.objs.index(("later", False, None)))
    return case


CASES = {"lanes7d": lambda: lanes(7, "d"), "lanes7u": lambda: lanes(7, "u"), "lanes9d": lambda: lanes(9, "d"), "lanes9u": lambda: lanes(9, "u"),
         "tree7": lambda: tree(7), "tree9": lambda: tree(9)}
KNOBS = {"tree7": TREE_KNOBS, "tree9": TREE_KNOBS}


def upload(ba, case, prob=None):
    """the problem (or the same problem at another state) with the masks of the first kind"""
    synth.upload(ba, case["prob"] if prob is None else prob)
    for t, m in case["masks0"].items():
        ba.set_active_mask(t, m)


# ------------------------------------------------------------------------------------------
# the reference: the other families' terms for schur_cases.reference
# ------------------------------------------------------------------------------------------
class SideTerms:
    """J^T J and J^T r of the factors of types 2 to 5 in long double, from raw residuals and Jacobians lin = {type: (r [n,m], J0 [n,m,d0], J1 [n,m,d1] or None)}
    (debug_linearize's shapes; lin None: the bookkeeping alone), the Huber rule per block (rho = s or 2 h sqrt(s) - h^2, weight rho'), and the reduced
    program's rule for what is variable."""

    def __init__(self, prob, lin, masks):
        self.prob, self.od = prob, int(prob.get("object_block_size", 7))
        P, O = len(prob["poses"]), len(prob["objects"])
        self.pose_used, self.obj_used = np.zeros(P, bool), np.zeros(O, bool)
        self.factors, self.cost, self.branches = [], LD(0), {}
        const = {"p": prob["pose_const"] != 0, "o": prob["object_const"] != 0}
        for t, (blocks, huber) in block_tables(prob).items():
            n = len(blocks[0][1])
            act = np.ones(n, bool) if masks is None or masks.get(t) is None else np.asarray(masks[t]) != 0
            over_any = under_any = False
            for i in np.flatnonzero(act):
                idx = [(k, int(a[i])) for k, a in blocks]
                live = not all(const[k][j] for k, j in idx)
                if live:
                    for k, j in idx:
                        if not const[k][j]:
                            (self.pose_used if k == "p" else self.obj_used)[j] = True
                if lin is None:
                    continue
                r = lin[t][0][i].astype(LD)
                ss, h = (r * r).sum(), LD(huber)
                over = bool(ss > h * h)
                over_any |= over; under_any |= not over
                self.cost += (2 * h * np.sqrt(ss) - h * h if over else ss) / 2
                if live:
                    J = [lin[t][1 + b][i].astype(LD) for b in range(len(blocks))]
                    self.factors.append((idx, r, J, h / np.sqrt(ss) if over else LD(1)))
            self.branches[t] = (over_any, under_any)

    def assemble(self, var_pose, frame):
        prob, od = self.prob, self.od
        obj_var = (prob["object_const"] == 0) & self.obj_used
        ovid = np.where(obj_var, np.cumsum(obj_var) - 1, -1)
        mp = 6 * int(var_pose.sum())
        m = mp + od * int(obj_var.sum())
        H, A, T = np.zeros((m, m), LD), np.zeros((m, m), LD), np.zeros((m, m), np.int64)
        g, Ag, Tg = np.zeros(m, LD), np.zeros(m, LD), np.zeros(m, np.int64)
        for idx, r, J, w in self.factors:
            rows = []
            for (k, j), Jb in zip(idx, J):
                if k == "p" and var_pose[j]:
                    rows.append((6 * int(frame[j]), 6, Jb))
                elif k == "o" and obj_var[j]:
                    rows.append((mp + od * int(ovid[j]), od, Jb))
            for ra, da, Ja in rows:
                g[ra:ra + da] += w * (Ja.T @ r); Ag[ra:ra + da] += w * (np.abs(Ja).T @ np.abs(r)); Tg[ra:ra + da] += len(r)
                for rb, db, Jb in rows:
                    H[ra:ra + da, rb:rb + db] += w * (Ja.T @ Jb); A[ra:ra + da, rb:rb + db] += w * (np.abs(Ja).T @ np.abs(Jb)); T[ra:ra + da, rb:rb + db] += len(r)
        return dict(H=H, A=A, T=T, g=g, Ag=Ag, Tg=Tg, cost=self.cost, object_var=obj_var, od=od, branches=self.branches)


def oracle_lin(o):
    """raw residuals and Jacobians of every family from an oracle handle"""
    return {t: o.debug_linearize(t) for t in (0,) + FAMILIES}


def reference(case, lin, radius, masks, want_step=True, prob=None):
    """schur_cases.reference over all families: lin from oracle_lin() or second_lin()"""
    prob = case["prob"] if prob is None else prob
    return sc.reference(prob, None, radius, masks[0], want_step=want_step, side=SideTerms(prob, lin, masks), lin0=lin[0])


# ------------------------------------------------------------------------------------------
# the product's own factor arithmetic, compiled for the host
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hostmath():
    so = os.path.join(helpers.ROOT, "tests", "libhostmath.so")
    src = os.path.join(helpers.ROOT, "tests", "hostmath_shim.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = C.CDLL(so)
    lib.hostmath_bbox.restype = lib.hostmath_bbox9.restype = C.c_int
    return lib


def _inv_sqrt(S):
    w, V = np.linalg.eigh(S)
    return (V / np.sqrt(w)) @ V.T


def second_lin(prob, lin):
    """lin with the residuals and Jacobians of types 0, 2 and 5 from tests/libhostmath.so (ba_math.h on the host) at the state of `prob`; the measurements are
    prepared as the upload does (rectified corners, the square-root information scaled by the focal lengths, the measured rotation as a matrix)"""
    lib, od = hostmath(), int(prob.get("object_block_size", 7))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731
    f8 = lambda a: np.ascontiguousarray(a, dtype=np.float64)    # noqa: E731
    out = dict(lin)
    n = len(prob["rp_pose"])
    r, Jp, Jl = np.zeros((n, 2)), np.zeros((n, 2, 6)), np.zeros((n, 2, 3))
    K, ext = [f8(k) for k in prob["K"]], [f8(e) for e in prob["ext"]]
    poses, points, objects = f8(prob["poses"]), f8(prob["points"]), f8(prob["objects"])
    pix = f8(prob["rp_pixel"])
    for i in range(n):
        c = int(prob["rp_cam"][i])
        lib.hostmath_reproj(dp(poses[prob["rp_pose"][i]]), dp(points[prob["rp_point"][i]]), dp(K[c]), dp(ext[c]), dp(pix[i]), C.c_double(prob["rp_sigma"]), dp(r[i]), dp(Jp[i]), dp(Jl[i]))
    out[0] = (r, Jp, Jl)
    n = len(prob["bb_obj"])
    r, Jo, Jp = np.zeros((n, 4)), np.zeros((n, 4, od)), np.zeros((n, 4, 6))
    fn = lib.hostmath_bbox9 if od == 9 else lib.hostmath_bbox
    valid = np.zeros(n, bool)
    for i in range(n):
        c = int(prob["bb_cam"][i])
        fx, fy, cx, cy = K[c]
        si = f8(_inv_sqrt(prob["bb_cov"][i].reshape(4, 4)) * np.array([fx, fx, fy, fy])[None, :])
        rect = f8((prob["bb_corners"][i] - np.array([cx, cx, cy, cy])) / np.array([fx, fx, fy, fy]))
        ok = fn(dp(objects[prob["bb_obj"][i]]), dp(poses[prob["bb_pose"][i]]), dp(K[c]), dp(ext[c]), dp(rect), dp(si), C.c_double(prob["bb_invalid"]), dp(r[i]), dp(Jo[i]), dp(Jp[i]))
        assert ok in (0, 1), "hostmath_bbox9: the one-direction form disagrees with the full one"
        valid[i] = ok == 1
    out[2] = (r, Jo, Jp)
    n = len(prob["rl_a"])
    r, Ja, Jb = np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    for i in range(n):
        R = f8(Rot.from_rotvec(prob["rl_aa"][i]).as_matrix())
        si = f8(_inv_sqrt(prob["rl_cov"][i].reshape(6, 6)))
        lib.hostmath_relpose(dp(poses[prob["rl_a"][i]]), dp(poses[prob["rl_b"][i]]), dp(f8(prob["rl_t"][i])), dp(R), dp(si), dp(r[i]), dp(Ja[i]), dp(Jb[i]))
    out[5] = (r, Ja, Jb)
    return out, valid


# ------------------------------------------------------------------------------------------
# errors against the reference
# ------------------------------------------------------------------------------------------
def step_errors(prob, poses, points, objects, ref):
    """as schur_cases.step_errors, with the objects"""
    ep, el = sc.step_errors(prob, poses, points, ref)
    eo = np.abs(objects.astype(LD) - (prob["objects"].astype(LD) + ref["step_object"])).max() / np.abs(ref["step_object"]).max()
    return ep, el, float(eo)


def robust_cost(sq, prob, n):
    """sum of rho / 2 in long double from the block norms of evaluate(apply_loss=False) (inactive factors are 0 there), n = factors per type 0, 2, 3, 4, 5"""
    hub = (prob["rp_huber"], prob["bb_huber"], prob["sp_huber"], prob["lt_huber"], prob["rl_huber"])
    total, at = LD(0), 0
    for k, h in zip(n, hub):
        s, h = sq[at:at + k].astype(LD), LD(h)
        total += np.where(s > h * h, 2 * h * np.sqrt(s) - h * h, s).sum() / 2
        at += k
    assert at == len(sq)
    return total
