"""Designed incidence structures for the two strip geometries of k_schur_window (ba_device.h: SchurWide, five tile columns per column group; SchurNarrow, three),
built with the case builder and checked with the extended-precision reference of tests/schur_cases.py.

The narrow geometry cuts the 40 strip frames of a row chunk into five groups of 8 frames (3 tile columns = 48 columns), so its group edges lie on multiples of
8 frames -- at 8, 16 and 32 frames back from the chunk the wide geometry (edges every 13 1/3 frames) has none.  The cases put tracks on both sides of every such
edge:

  edge        tracks that start, and tracks that end, on a multiple of 8 frames and one frame to either side; two-sighting points on the same frames
  all_groups  a 40-frame track ending with a chunk: that chunk visits all five groups; a 41-frame track: its longest pairs go to k_schur_blocks
  chunk0      tracks inside the first chunks, whose strips start before frame 0
  const       tracks across the constant poses inside the window (poses 20, 21 and 45)
  big_list    48 points on the frames (16, 23) back and (0, 7) of one chunk: one (chunk, group) work list of 17 slots a visit (34 for a stereo point), 816
              (1632) slots -- a workgroup of a default handle (up to 64 visits) streams five (ten) 24 KB batches of 170 slots, both LDS buffers turn over
  filler      short tracks over all frames: two thousand features and more, so that the other work lists are cut into several workgroups

65 variable frames of 70 poses (8 k + 1: the last chunk holds one frame).  `geom_stereo` is a stereo rig (every designed point seen by both cameras: the TWIN
instantiation of the kernel), `geom_mono` the same incidence with one camera.

TABLE: e(oracle) per case as measured by tests/test_schur_geometry_reference.py; the bound for the device is schur_cases.bound(name, what, TABLE)."""
import functools
from collections import defaultdict

import numpy as np
from scipy.spatial.transform import Rotation as Rot

import schur_cases as sc
import synth

# name: e(oracle) per quantity (tests/test_schur_geometry_reference.py prints them; it fails if they drift by more than a factor 2) and n_terms
TABLE = {
    "geom_mono": dict(S=9.6e-15, b=1.1e-16, n_terms=3103),
    "geom_stereo": dict(S=1.2e-14, b=9.4e-17, n_terms=4756),
}

P, CONST_POSES = 70, (0, 20, 21, 45, 69)
NARROW_TILES, NARROW_BATCH_SLOTS = 3, 24576 // 144
BIG_CHUNK, BIG_GROUP, BIG_POINTS = 6, 2, 48
FILLERS = 2100


def narrow_lists(prob, mask=None):
    """{(chunk, group): [slots of each visit]} of the narrow geometry: schur_cases.strip_routing's walk with groups of NARROW_TILES tile columns"""
    n = len(prob["rp_pose"])
    act = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    pose, point = prob["rp_pose"].astype(np.int64), prob["rp_point"].astype(np.int64)
    live = act & ~((prob["pose_const"][pose] != 0) & (prob["point_const"][point] != 0))
    var_pose = (prob["pose_const"] == 0) & (np.bincount(pose[live], minlength=len(prob["poses"])) > 0)
    frame = np.where(var_pose, np.cumsum(var_pose) - 1, -1)
    ntiles, row0 = sc.STRIP * 6 // sc.TILE, sc.BACK * 6 // sc.TILE
    frames_of = defaultdict(list)
    for a in np.flatnonzero(act):
        if frame[pose[a]] >= 0 and not prob["point_const"][point[a]]:
            frames_of[int(point[a])].append(int(frame[pose[a]]))
    lists = defaultdict(list)
    for l in sorted(frames_of):
        F = sorted(frames_of[l])
        mult = max(F.count(f) for f in F)
        if mult > 2:
            continue
        for c in sorted({f // sc.ROWS for f in F}):
            base = sc.ROWS * c - sc.BACK
            offs = {f - base for f in F if base <= f < sc.ROWS * (c + 1)}
            touched = [any(f in offs for f in sc._frames_of_tile(t)) for t in range(ntiles)]
            for g in range(ntiles // NARROW_TILES):
                cols = {tc for tc in range(NARROW_TILES * g, NARROW_TILES * (g + 1)) for tr in range(3) if touched[tc] and touched[row0 + tr] and tc <= row0 + tr}
                rows = {tr for tc in cols for tr in range(3) if touched[row0 + tr] and tc <= row0 + tr}
                if cols:
                    lists[(c, g)].append(sc._visit_slots(cols, rows, mult == 2)[0])
    return dict(lists)


def narrow_batches(lists, schur_wgs=1536):
    """{(chunk, group): [batches of each workgroup]} on a DEFAULT handle (plan.cpp, schur_batches_of): a work list is cut into slices of at most
    max(64, all visits / OBVI_SCHUR_WGS) visits, equal parts, one workgroup each; a workgroup's visits, in point order, fill batches of at most
    sc.BATCH_VISITS visits and NARROW_BATCH_SLOTS slots"""
    slice_ = max(64, sum(len(v) for v in lists.values()) // schur_wgs)
    out = {}
    for key, slots in lists.items():
        parts = -(-len(slots) // slice_)
        per = -(-len(slots) // parts)
        out[key] = []
        for w in range(0, len(slots), per):
            nb, used, cnt = 1, 0, 0
            for n in slots[w:w + per]:
                if cnt == sc.BATCH_VISITS or used + n > NARROW_BATCH_SLOTS:
                    nb, used, cnt = nb + 1, 0, 0
                used += n; cnt += 1
            out[key].append(nb)
    return out


def _finish(b):
    """schur_cases._Builder.finish -- its scene, its noise, its outliers -- without the size cap of the hand-sized cases there, and with the work lists of the
    narrow geometry beside the wide geometry's predictions"""
    L = b.n_points
    rng = b.rng
    i = np.arange(b.P)
    pos = np.stack([0.1 * i, 0.02 * np.sin(0.7 * i), 0.01 * np.cos(0.9 * i)], axis=1)
    R = Rot.from_euler("ZYX", np.stack([np.pi / 2 + 0.03 * np.sin(0.5 * i), 0.02 * np.sin(0.3 * i + 0.3), 0.015 * np.cos(0.4 * i)], axis=1))
    gt_poses = np.concatenate([pos, R.as_rotvec()], axis=1)
    gt_points = np.stack([rng.uniform(-3.0, 0.1 * b.P + 3.0, L), rng.uniform(8.0, 20.0, L), rng.uniform(-2.0, 2.0, L)], axis=1)
    s = sorted(b.sightings, key=lambda x: (x[0], x[1], x[2]))
    rp_point = np.array([x[0] for x in s], np.uint32); rp_pose = np.array([x[1] for x in s], np.uint32); rp_cam = np.array([x[2] for x in s], np.uint16)
    mask0 = np.ones(len(s), np.uint8)
    ext2 = synth.EXT_DEFAULT.copy(); ext2[5] = -0.12
    K = np.stack([synth.K_DEFAULT] * (2 if b.stereo else 1)); ext = np.stack([synth.EXT_DEFAULT, ext2][:2 if b.stereo else 1])
    pix = np.zeros((len(s), 2))
    for c in range(len(K)):
        m = rp_cam == c
        px, z = synth.project_points(gt_poses[rp_pose[m]], gt_points[rp_point[m]], K[c], ext[c])
        assert (z > 5.0).all()
        pix[m] = px
    pix += rng.normal(size=pix.shape)
    is_out = np.arange(len(s)) % 37 == 5
    pix[is_out] += np.array([40.0, -40.0])
    poses = gt_poses + rng.normal(size=gt_poses.shape) * np.array([0.02, 0.02, 0.02, 0.004, 0.004, 0.004])
    points = gt_points + rng.normal(size=gt_points.shape) * 0.05
    prob = dict(K=K, ext=ext, poses=poses, gt_poses=gt_poses, pose_const=b.pose_const.copy(), points=points, gt_points=gt_points,
                point_const=np.array(b.point_const, np.uint8), rp_pose=rp_pose, rp_point=rp_point, rp_cam=rp_cam, rp_pixel=pix,
                rp_sigma=synth.RESIDUAL_PARAMS["reproj_sigma"], rp_huber=synth.RESIDUAL_PARAMS["reproj_huber"], rp_is_outlier=is_out,
                objects=np.zeros((0, 7)), gt_objects=np.zeros((0, 7)), object_const=np.zeros(0, np.uint8),
                bb_obj=np.zeros(0, np.uint32), bb_pose=np.zeros(0, np.uint32), bb_cam=np.zeros(0, np.uint16), bb_corners=np.zeros((0, 4)), bb_cov=np.zeros((0, 16)),
                bb_huber=0.5, bb_invalid=1000.0, sp_obj=np.zeros(0, np.uint32), sp_mean=np.zeros((0, 3)), sp_cov=np.zeros((0, 9)), sp_huber=10.0, obj_class=[])
    for c in range(len(K)):
        m = rp_cam == c
        assert (synth.project_points(poses[rp_pose[m]], points[rp_point[m]], K[c], ext[c])[1] > 5.0).all()
    predict = sc.strip_routing(prob, mask0)
    predict["narrow_lists"] = narrow_lists(prob, mask0)
    predict["narrow_batches"] = narrow_batches(predict["narrow_lists"])
    assert predict["n_frames"] == b.n_frames, "a variable pose without a sighting"
    return dict(name=b.name, prob=prob, mask0=mask0, groups=dict(b.groups), predict=predict, pose_of_frame=b.pose_of_frame)


def _case(name, stereo, seed):
    b = sc._Builder(name, P, stereo, seed, const_poses=CONST_POSES)
    cams = (0, 1) if stereo else (0,)
    nF = b.n_frames
    assert nF == 65
    # the group edges of the narrow geometry: tracks that start / end on a multiple of 8 frames and one frame to either side
    for edge in (8, 16, 24, 32):
        for d in (-1, 0, 1):
            b.frames("edge", range(edge + d, edge + d + 11), cams)          # starts on the edge: its first frame is the first / last / second of a group
            b.frames("edge", range(max(0, edge + d - 10), edge + d + 1), cams)   # ends on it
            b.frames("edge", [edge + d, min(nF - 1, edge + d + 31)], cams)  # two sightings as far apart as the strip reaches from there
            b.frames("edge", [edge + d, edge + d + 16])
    # one row chunk that visits all five groups (40 frames ending with chunk 5), and a track one frame longer (far pairs)
    b.frames("all_groups", range(8, 48), cams)
    b.frames("all_groups", range(7, 48))
    b.frames("all_groups", range(16, 57))
    # the first chunks: strips that start before frame 0
    b.frames("chunk0", [0, 3, 7], cams); b.frames("chunk0", [1, 2]); b.frames("chunk0", [5]); b.frames("chunk0", range(0, 12), cams); b.frames("chunk0", [0, 31])
    # across the constant poses inside the window (poses 20, 21 and 45), and ending on the last frame (a chunk of one frame)
    b.track("const", 17, 8, cams); b.track("const", 40, 10); b.point("const", [(19, 0), (20, 0), (22, 0)]); b.point("const", [(44, 0), (45, 0), (46, 0), (60, 0)])
    b.frames("last", range(nF - 9, nF), cams); b.frames("last", [nF - 1 - 32, nF - 1]); b.frames("last", [nF - 1])
    # one long work list: (chunk 6, group 2) -- frames 16 and 23 of the strip, frames 0 and 7 of the chunk
    base = sc.ROWS * BIG_CHUNK - sc.BACK
    for _ in range(BIG_POINTS):
        b.frames("big_list", [base + 8 * BIG_GROUP, base + 8 * BIG_GROUP + 7, sc.ROWS * BIG_CHUNK, sc.ROWS * BIG_CHUNK + 7], cams)
    b.fillers(FILLERS)
    case = _finish(b)
    pr = case["predict"]
    big = pr["narrow_lists"][(BIG_CHUNK, BIG_GROUP)]
    per = 34 if stereo else 17
    assert big.count(per) >= BIG_POINTS and BIG_POINTS <= 64 and BIG_POINTS * per > 3 * NARROW_BATCH_SLOTS, "one workgroup, more than three batches"
    assert len(pr["narrow_batches"][(BIG_CHUNK, BIG_GROUP)]) == 1 and pr["narrow_batches"][(BIG_CHUNK, BIG_GROUP)][0] >= (9 if stereo else 5), "the long list: one workgroup"
    assert {g for (c, g) in pr["narrow_lists"] if c == 5} == {0, 1, 2, 3, 4}, "a chunk that visits all five groups"
    assert pr["schur_pairs_blocks"] > 0, "the 41-frame tracks leave pairs to k_schur_blocks"
    assert 2000 <= b.n_points <= 4000
    return case


@functools.lru_cache(maxsize=None)
def geom_stereo():
    return _case("geom_stereo", True, 9201)


@functools.lru_cache(maxsize=None)
def geom_mono():
    return _case("geom_mono", False, 9202)


CASES = {"geom_stereo": geom_stereo, "geom_mono": geom_mono}


def measure(name):
    """e(oracle) of a case, as a dict with the keys of TABLE (tests/test_schur_reference.py: measure, on the cases of this module)"""
    import helpers
    case = CASES[name]()
    prob = case["prob"]
    o = helpers.oracle_ba()
    synth.upload(o, prob)
    out = dict(S=0.0, b=0.0, n_terms=0)
    for radius in sc.RADII:
        ref = sc.reference(prob, o, radius, case["mask0"], want_step=False)
        assert ref["pivots_ok"] and ref["both_huber_branches"]
        S, b = o.debug_reduced_system(radius)
        assert S.shape == ref["S"].shape and sc.exact_zeros(S, ref["S"]) and sc.exact_zeros(b, ref["b"])
        out["S"] = max(out["S"], sc.entry_error(S, ref["S"], ref["A_S"]))
        out["b"] = max(out["b"], sc.entry_error(b, ref["b"], ref["A_b"]))
        out["n_terms"] = max(out["n_terms"], ref["n_terms"])
    return out
