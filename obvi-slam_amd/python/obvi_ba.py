"""ctypes binding of the C ABI declared in include/obvi_ba.h.

Plumbing only: tests and bench.py drive libobvi_ba.so (the HIP product) through this class.
The same class can bind any library exporting the ABI under another symbol prefix -- the
tests use that to drive the CPU oracle (oracle/libobvi_oracle.so, prefix "oracle_") with the
very same arrays.  Nothing here computes anything; a missing library raises.
"""
import collections
import ctypes as C
import os

import numpy as np

FACTOR_REPROJECTION = 0
FACTOR_BBOX = 2
FACTOR_SHAPE_PRIOR = 3
FACTOR_LTM_PRIOR = 4
FACTOR_REL_POSE = 5
FACTOR_MAP_PAIR_PRIOR = 9    # include/obvi_map_prior.h: not in FACTOR_TYPES (the oracle does not know it)
MAP_PAIR_JOINT, MAP_PAIR_CONDITIONAL = 0, 1
FACTOR_MAP_GROUP_PRIOR = 10  # include/obvi_map_group_prior.h: a Gaussian on a group of objects (not in FACTOR_TYPES either)
MAP_GROUP_MAX_ROWS = 2048
FACTOR_TYPES = (FACTOR_REPROJECTION, FACTOR_BBOX, FACTOR_SHAPE_PRIOR, FACTOR_LTM_PRIOR, FACTOR_REL_POSE)
RESIDUAL_DIM = {0: 2, 2: 4, 3: 3, 4: 7, 5: 6, 9: 14}
BLOCK_DIMS = {0: (6, 3), 2: (7, 6), 3: (7, 0), 4: (7, 0), 5: (6, 6), 9: (7, 7)}

CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2


class Options(C.Structure):
    _fields_ = [("device_id", C.c_int32), ("object_block_size", C.c_int32), ("reprojection_variant", C.c_int32), ("deterministic", C.c_int32), ("reserved", C.c_int32 * 4)]


class SolverParams(C.Structure):
    """pose_graph_optimization::OptimizationSolverParams (optimization_solver_params.h:10-30)."""
    _fields_ = [("max_num_iterations", C.c_int32), ("allow_non_monotonic_steps", C.c_int32),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double),
                ("max_trust_region_radius", C.c_double)]

    def __init__(self, max_num_iterations=100, allow_non_monotonic_steps=False, function_tolerance=1e-6,
                 gradient_tolerance=1e-10, parameter_tolerance=1e-8, initial_trust_region_radius=1e4,
                 max_trust_region_radius=1e16):
        super().__init__(max_num_iterations, int(allow_non_monotonic_steps), function_tolerance,
                         gradient_tolerance, parameter_tolerance, initial_trust_region_radius,
                         max_trust_region_radius)


class IterationSummary(C.Structure):
    _fields_ = [("iteration", C.c_int32), ("step_is_valid", C.c_int32), ("step_is_successful", C.c_int32),
                ("reserved", C.c_int32), ("cost", C.c_double), ("cost_change", C.c_double),
                ("gradient_max_norm", C.c_double), ("gradient_norm", C.c_double), ("step_norm", C.c_double),
                ("relative_decrease", C.c_double), ("trust_region_radius", C.c_double),
                ("iteration_time_in_seconds", C.c_double)]


class Summary(C.Structure):
    _fields_ = [("termination_type", C.c_int32), ("is_solution_usable", C.c_int32),
                ("num_iterations", C.c_int32), ("num_successful_steps", C.c_int32),
                ("num_unsuccessful_steps", C.c_int32), ("num_parameters_reduced", C.c_int32),
                ("num_residuals_reduced", C.c_int32), ("reduced_system_size", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("fixed_cost", C.c_double),
                ("total_time_in_seconds", C.c_double), ("linear_solver_time_in_seconds", C.c_double),
                ("jacobian_evaluation_time_in_seconds", C.c_double),
                ("residual_evaluation_time_in_seconds", C.c_double), ("message", C.c_char * 160)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p)


class EpipolarParams(C.Structure):
    """obvi_epipolar_params (include/obvi_frontend.h)."""
    _fields_ = [("inlier_epipolar_err_thresh", C.c_double), ("inlier_majority_percentage", C.c_double), ("early_votes_return", C.c_int32), ("reserved", C.c_int32)]

    def __init__(self, thresh=8.0, majority=0.5, early_return=True):
        super().__init__(thresh, majority, int(early_return), 0)


class ParallaxParams(C.Structure):
    """obvi_parallax_params (include/obvi_frontend.h); defaults: config/base7a_2_fallback.json visual_feature_params."""
    _fields_ = [("min_pixel", C.c_double), ("min_transl", C.c_double), ("min_orient", C.c_double), ("enforce_pixel", C.c_int32), ("enforce_pose", C.c_int32)]

    def __init__(self, min_pixel=5.0, min_transl=0.1, min_orient=0.05, enforce_pixel=True, enforce_pose=False):
        super().__init__(min_pixel, min_transl, min_orient, int(enforce_pixel), int(enforce_pose))


class BboxFrontendParams(C.Structure):
    """obvi_bbox_frontend_params (include/obvi_bbox_frontend.h); defaults: FeatureBasedBbAssociationParams."""
    _fields_ = [("bounding_box_inflation_size", C.c_double), ("min_overlapping_features_for_match", C.c_double)]

    def __init__(self, inflation=0.0, min_overlap=2.0):
        super().__init__(inflation, min_overlap)


class LocateParams(C.Structure):
    """obvi_map_locate_params (include/obvi_map_locate.h)."""
    _fields_ = [("pair_min_distance", C.c_double), ("pair_tolerance", C.c_double), ("inlier_gate", C.c_double), ("min_inliers", C.c_int32), ("refine_iterations", C.c_int32)]


Located = collections.namedtuple("Located", "seed transform transform_cov inliers cost partner counts move")


class ObviError(RuntimeError):
    pass


def default_library_path():
    """csrc/libobvi_ba.so; OBVI_BA_LIBRARY names another build of the same product (A/B runs of compile-time variants: scripts/ab_env.sh)."""
    here = os.path.dirname(os.path.abspath(__file__))
    return os.environ.get("OBVI_BA_LIBRARY") or os.path.join(os.path.dirname(here), "csrc", "libobvi_ba.so")


def _f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ptr(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _library_path(library=None):
    """`library`, or the default build; a build that is not there raises: nothing computes in its place."""
    path = library or default_library_path()
    if not os.path.exists(path):
        raise ObviError("%s not found: build it with __graft_entry__.build() -- there is no CPU fallback" % path)
    return path


def _entry(lib, prefix, name, header="obvi_ba.h", restype=C.c_int):
    """lib's function prefix + name, its restype set.  A library that lacks it (the oracle mirrors include/obvi_ba.h alone) raises, naming the entry and its header."""
    try:
        f = getattr(lib, prefix + name)
    except AttributeError:
        raise ObviError("%s%s: this library does not have the entry (include/%s is served by libobvi_ba.so only)" % (prefix, name, header))
    f.restype = restype
    return f


def _count_then_fill(capacity, counts, found_at, call, alloc):
    """The capacity protocol of the two report entries (Map.match, Map.locate).  call(cap, arrays) runs the entry -- arrays None: NULL pointers -- and fills
    counts; alloc(cap) makes the output arrays.  capacity None: a call with capacity 0, then one of the exact size counts[found_at]; a negative one is passed
    through to be refused; 0: the count-only call alone.  Returns (arrays, k), k the entries that were reported."""
    counted = capacity is None
    if counted:
        call(0, None)
        capacity = counts[found_at]
    capacity = int(capacity)
    if capacity < 0:
        call(capacity, None)                                           # refused: raises
    arrays = alloc(capacity)
    if capacity > 0:
        call(capacity, arrays)
    elif not counted:
        call(0, None)
    return arrays, min(capacity, int(counts[found_at]))


class Map:
    """A long-term map on the device (include/obvi_map_resident.h): means [n][od] and the joint covariance [n od][n od] of its n objects, uploaded once and
    immutable; any BundleAdjuster on the same device cuts its group priors from it (set_map_group_priors_from_map)."""

    def __init__(self, mean, cov, device_id=0, object_block_size=7, library=None, prefix="obvi_"):
        path = _library_path(library)
        self._lib = C.CDLL(path)
        self._pre = prefix
        self._m = C.c_void_p()
        f = _entry(self._lib, prefix, "map_create", "obvi_map_resident.h")
        self.od = int(object_block_size) or 7
        mu = _f64(mean, (-1, self.od))
        cv = _f64(cov, (len(mu) * self.od, len(mu) * self.od))
        rc = f(C.c_int32(device_id), C.c_int32(int(object_block_size)), C.c_int64(len(mu)), _ptr(mu, C.c_double), _ptr(cv, C.c_double), C.byref(self._m))
        if rc != 0:
            raise ObviError("%smap_create failed: status %d" % (prefix, rc))

    @classmethod
    def create(cls, mean, cov, **kw):
        return cls(mean, cov, **kw)

    @property
    def n_objects(self):
        f = getattr(self._lib, self._pre + "map_num_objects")
        f.restype = C.c_int64
        return int(f(self._m))

    def _entry(self, name, header):
        return _entry(self._lib, self._pre, name, header)

    # ---- the way back (include/obvi_map_update.h) ----
    def _conditioned(self, ba, rc, new, what):
        ba._check(rc, what)
        m = Map.__new__(Map)
        m._lib, m._pre, m._m, m.od = self._lib, self._pre, new, self.od
        return m

    def get(self):
        """(mean [n][od], cov [n od][n od]) as the device holds them."""
        n = self.n_objects
        mean, cov = np.zeros((n, self.od)), np.zeros((n * self.od, n * self.od))
        rc = self._entry("map_get", "obvi_map_update.h")(self._m, _ptr(mean, C.c_double), _ptr(cov, C.c_double))
        if rc != 0:
            raise ObviError("%smap_get failed: status %d" % (self._pre, rc))
        return mean, cov

    def condition(self, ba, map_idx, post_mean, post_cov):
        """A new Map: this one conditioned on the posterior N(post_mean [k][od], post_cov [k od][k od]) of its objects map_idx; `ba` lends its stream and workspaces."""
        mid = np.ascontiguousarray(map_idx, dtype=np.uint32)
        mu = _f64(post_mean, (len(mid), self.od))
        cv = _f64(post_cov, (len(mid) * self.od, len(mid) * self.od))
        new = C.c_void_p()
        rc = self._entry("map_condition", "obvi_map_update.h")(ba._h, self._m, C.c_int64(len(mid)), _ptr(mid, C.c_uint32), _ptr(mu, C.c_double), _ptr(cv, C.c_double), C.byref(new))
        return self._conditioned(ba, rc, new, "map_condition")

    def condition_on(self, ba, obj_idx, map_idx):
        """A new Map: this one conditioned on the current estimates and joint covariance of `ba`'s objects obj_idx, which are the map objects map_idx."""
        oid, mid = np.ascontiguousarray(obj_idx, dtype=np.uint32), np.ascontiguousarray(map_idx, dtype=np.uint32)
        if len(oid) != len(mid):
            raise ObviError("map_condition_on_handle: obj_idx and map_idx differ in length")
        new = C.c_void_p()
        rc = self._entry("map_condition_on_handle", "obvi_map_update.h")(ba._h, self._m, C.c_int64(len(mid)), _ptr(oid, C.c_uint32), _ptr(mid, C.c_uint32), C.byref(new))
        return self._conditioned(ba, rc, new, "map_condition_on_handle")

    # ---- a map that grows (include/obvi_map_extend.h) ----
    @classmethod
    def _unborn(cls, ba):
        """No map yet: what from_posterior / from_handle extend.  It takes the library, prefix and block size of `ba`."""
        m = cls.__new__(cls)
        m._lib, m._pre, m._m, m.od = ba._lib, ba._pre, C.c_void_p(), ba.od or 7
        return m

    def extend(self, ba, map_idx, post_mean, post_cov, n_new):
        """A new Map of n + n_new objects: this one conditioned on the joint posterior N(post_mean [k + n_new][od], post_cov) of its objects map_idx (k >= 0 of
        them) followed by n_new objects it does not hold, which are appended in that order."""
        mid = np.ascontiguousarray(map_idx, dtype=np.uint32).ravel()
        k = len(mid) + int(n_new)
        mu = _f64(post_mean, (k, self.od))
        cv = _f64(post_cov, (k * self.od, k * self.od))
        new = C.c_void_p()
        rc = self._entry("map_extend", "obvi_map_extend.h")(ba._h, self._m, C.c_int64(len(mid)), _ptr(mid, C.c_uint32) if len(mid) else None, C.c_int64(int(n_new)),
                                           _ptr(mu, C.c_double), _ptr(cv, C.c_double), C.byref(new))
        return self._conditioned(ba, rc, new, "map_extend")

    def extend_on(self, ba, obj_old, map_idx, obj_new):
        """A new Map: this one grown by `ba`'s objects obj_new, from the current estimates and joint covariance of obj_old (the map objects map_idx) and obj_new."""
        old, mid = np.ascontiguousarray(obj_old, dtype=np.uint32).ravel(), np.ascontiguousarray(map_idx, dtype=np.uint32).ravel()
        fresh = np.ascontiguousarray(obj_new, dtype=np.uint32).ravel()
        if len(old) != len(mid):
            raise ObviError("map_extend_on_handle: obj_old and map_idx differ in length")
        new = C.c_void_p()
        rc = self._entry("map_extend_on_handle", "obvi_map_extend.h")(ba._h, self._m, C.c_int64(len(mid)), _ptr(old, C.c_uint32) if len(old) else None,
                                                     _ptr(mid, C.c_uint32) if len(mid) else None, C.c_int64(len(fresh)), _ptr(fresh, C.c_uint32), C.byref(new))
        return self._conditioned(ba, rc, new, "map_extend_on_handle")

    def select(self, ba, map_idx):
        """A new Map of this one's objects map_idx, in that order, copied as the device holds them: a subset is the marginal, all of them a permutation."""
        mid = np.ascontiguousarray(map_idx, dtype=np.uint32).ravel()
        new = C.c_void_p()
        rc = self._entry("map_select", "obvi_map_extend.h")(ba._h, self._m, C.c_int64(len(mid)), _ptr(mid, C.c_uint32), C.byref(new))
        return self._conditioned(ba, rc, new, "map_select")

    @classmethod
    def from_posterior(cls, ba, post_mean, post_cov):
        """A first Map, born on `ba`'s device from the posterior N(post_mean [k][od], post_cov [k od][k od]) of k objects: there is no map yet."""
        return cls._unborn(ba).extend(ba, [], post_mean, post_cov, len(_f64(post_mean, (-1, ba.od or 7))))

    @classmethod
    def from_handle(cls, ba, obj_idx):
        """A first Map, born from the current estimates and joint covariance of `ba`'s objects obj_idx."""
        return cls._unborn(ba).extend_on(ba, [], [], obj_idx)

    # ---- a map that shrinks (include/obvi_map_merge.h) ----
    def merge(self, ba, drop_idx, keep_idx, offset=None, noise=None):
        """(Map, new_index [n]): a new Map of n - q objects in which each object drop_idx[r] is fused into keep_idx[r], x_drop - x_keep = offset[r] ([q][od];
        None: zeros) up to the covariance noise[r] ([q][od][od]; None: exactly); new_index[o] is the new number of old object o."""
        drop, keep = np.ascontiguousarray(drop_idx, dtype=np.uint32).ravel(), np.ascontiguousarray(keep_idx, dtype=np.uint32).ravel()
        if len(drop) != len(keep):
            raise ObviError("map_merge: drop_idx and keep_idx differ in length")
        f = self._entry("map_merge", "obvi_map_merge.h")
        d = None if offset is None else _f64(offset, (len(drop), self.od))
        r = None if noise is None else _f64(noise, (len(drop), self.od, self.od))
        where = np.zeros(self.n_objects, np.uint32)
        new = C.c_void_p()
        rc = f(ba._h, self._m, C.c_int64(len(drop)), _ptr(drop, C.c_uint32), _ptr(keep, C.c_uint32), _ptr(d, C.c_double), _ptr(r, C.c_double),
               _ptr(where, C.c_uint32), C.byref(new))
        return self._conditioned(ba, rc, new, "map_merge"), where

    # ---- which objects are duplicates (include/obvi_map_match.h) ----
    def match(self, ba, gate, labels=None, row_mask=0, max_centre_distance=float("inf"), yaw_period=0.0, capacity=None):
        """(a, b, stat, yaw_offset, counts): the pairs a < b of this map's objects whose difference, on the rows of row_mask, is within `gate` in units of its own
        covariance, in (a, b) order; counts = (found, tested, singular).  capacity None: a count-only call, then one of the exact size."""
        f = self._entry("map_match", "obvi_map_match.h")
        lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32).ravel()
        if lab is not None and len(lab) != self.n_objects:
            raise ObviError("map_match: labels must name every object of the map")
        counts = np.zeros(3, np.int64)

        def call(cap, arrays):
            a, b, s, w = arrays or (None,) * 4
            ba._check(f(ba._h, self._m, _ptr(lab, C.c_int32), C.c_uint32(int(row_mask)), C.c_double(gate), C.c_double(max_centre_distance), C.c_double(yaw_period),
                        C.c_int64(cap), _ptr(a, C.c_uint32), _ptr(b, C.c_uint32), _ptr(s, C.c_double), _ptr(w, C.c_double), _ptr(counts, C.c_int64)), "map_match")

        (a, b, s, w), k = _count_then_fill(capacity, counts, 0, call, lambda cap: (np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap), np.zeros(cap)))
        return a[:k], b[:k], s[:k], w[:k], tuple(int(c) for c in counts)

    # ---- another frame, and two maps in one (include/obvi_map_frame.h) ----
    def transform(self, ba, transform, cov=None):
        """A new Map: this one moved into another frame by T_new<-old = transform ([4] tx ty tz psi for od 7, [6] translation and axis-angle for od 9), whose
        covariance is cov ([dT][dT]; None: the transform is exact).  Same objects, same numbers."""
        dT = 4 if self.od == 7 else 6
        t = _f64(transform, (dT,))
        s = None if cov is None else _f64(cov, (dT, dT))
        new = C.c_void_p()
        rc = self._entry("map_transform", "obvi_map_frame.h")(ba._h, self._m, _ptr(t, C.c_double), _ptr(s, C.c_double), C.byref(new))
        return self._conditioned(ba, rc, new, "map_transform")

    def join(self, ba, other):
        """A new Map of this one's objects followed by `other`'s, the two uncorrelated: blockdiag of the covariances, copied as the device holds them."""
        new = C.c_void_p()
        rc = self._entry("map_join", "obvi_map_frame.h")(ba._h, self._m, other._m, C.byref(new))
        return self._conditioned(ba, rc, new, "map_join")

    # ---- where another map lies in this one (include/obvi_map_locate.h) ----
    def locate(self, ba, other, pair_min_distance, pair_tolerance, inlier_gate, min_inliers=3, refine_iterations=3, labels=None, other_labels=None, capacity=None):
        """Located(seed [k][4], transform [k][4], transform_cov [k][4][4], inliers [k], cost [k], partner [k][n_other], counts, move [k][dT]): the transforms
        T_self<-other = (tx ty tz psi) that lay `other`'s object centres onto this map's, best first; counts = (seeds tested, seeds compatible, hypotheses with
        >= min_inliers).  move is what Map.transform of `other` takes: transform itself for od 7, (t, 0, 0, psi) for od 9.  capacity None: a count-only
        call, then one of the exact size."""
        f = self._entry("map_locate", "obvi_map_locate.h")
        na, nb = self.n_objects, other.n_objects
        la = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32).ravel()
        lb = None if other_labels is None else np.ascontiguousarray(other_labels, dtype=np.int32).ravel()
        if (la is not None and len(la) != na) or (lb is not None and len(lb) != nb):
            raise ObviError("map_locate: labels must name every object of their map")
        params = LocateParams(float(pair_min_distance), float(pair_tolerance), float(inlier_gate), int(min_inliers), int(refine_iterations))
        counts = np.zeros(3, np.int64)

        def call(cap, arrays):
            seed, t, cov, inl, cost, partner = arrays or (None,) * 6
            ba._check(f(ba._h, self._m, other._m, _ptr(la, C.c_int32), _ptr(lb, C.c_int32), C.byref(params), C.c_int64(cap), _ptr(seed, C.c_uint32), _ptr(t, C.c_double),
                        _ptr(cov, C.c_double), _ptr(inl, C.c_int32), _ptr(cost, C.c_double), _ptr(partner, C.c_int32), _ptr(counts, C.c_int64)), "map_locate")

        def alloc(cap):
            return (np.zeros((cap, 4), np.uint32), np.zeros((cap, 4)), np.zeros((cap, 4, 4)), np.zeros(cap, np.int32), np.zeros(cap), np.full((cap, nb), -1, np.int32))

        (seed, t, cov, inl, cost, partner), k = _count_then_fill(capacity, counts, 2, call, alloc)
        move = t[:k].copy() if self.od == 7 else np.concatenate([t[:k, :3], np.zeros((k, 2)), t[:k, 3:]], axis=1)
        return Located(seed[:k], t[:k], cov[:k], inl[:k], cost[:k], partner[:k], tuple(int(c) for c in counts), move)

    def close(self):
        if self._m:
            f = getattr(self._lib, self._pre + "map_destroy")
            f.restype = None
            f(self._m)
            self._m = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def map_match_resolve(od, a, b, stat, max_pairs=None, library=None, prefix="obvi_"):
    """(drop, keep, sel): candidate pairs a < b with their statistics (Map.match) resolved, greedily in ascending (stat, a, b) order, into lists Map.merge accepts
    as they are -- no object dropped twice, no dropped object kept; sel[i] is the position of selected pair i in the input.  Host only: no handle, no device."""
    path = _library_path(library)
    f = _entry(C.CDLL(path), prefix, "map_match_resolve", "obvi_map_match.h")
    ia, ib = np.ascontiguousarray(a, dtype=np.uint32).ravel(), np.ascontiguousarray(b, dtype=np.uint32).ravel()
    st = _f64(stat).ravel()
    if not len(ia) == len(ib) == len(st):
        raise ObviError("map_match_resolve: a, b and stat differ in length")
    if max_pairs is None:
        max_pairs = MAP_GROUP_MAX_ROWS // (int(od) or 7)
    room = max(1, min(int(max_pairs), len(ia)))
    drop, keep, sel = np.zeros(room, np.uint32), np.zeros(room, np.uint32), np.zeros(room, np.uint32)
    q = C.c_int64(0)
    rc = f(C.c_int32(int(od)), C.c_int64(len(ia)), _ptr(ia, C.c_uint32), _ptr(ib, C.c_uint32), _ptr(st, C.c_double), C.c_int64(int(max_pairs)),
           _ptr(drop, C.c_uint32), _ptr(keep, C.c_uint32), _ptr(sel, C.c_uint32), C.byref(q))
    if rc != 0:
        raise ObviError("%smap_match_resolve failed: status %d" % (prefix, rc))
    return drop[:q.value], keep[:q.value], sel[:q.value]


def bbox_assign(is_match, score, n_pending, library=None, prefix="obvi_"):
    """(assigned, is_new) of the boxes of one round (BundleAdjuster.bbox_associate): the matches taken greedily by descending score, ties by box then candidate
    index; a box left over opens a new pending object numbered from n_pending upwards.  Host only: no handle, no device."""
    path = _library_path(library)
    f = _entry(C.CDLL(path), prefix, "bbox_frontend_assign", "obvi_bbox_frontend.h")
    m, sc = np.ascontiguousarray(is_match, dtype=np.uint8), _f64(score)
    if m.ndim != 2 or m.shape != sc.shape:
        raise ObviError("bbox_assign: is_match and score must be [n_box][n_cand] both")
    assigned, is_new = np.zeros(m.shape[0], np.int64), np.zeros(m.shape[0], np.uint8)
    rc = f(C.c_int64(m.shape[0]), C.c_int64(m.shape[1]), C.c_int64(int(n_pending)), _ptr(m, C.c_uint8), _ptr(sc, C.c_double), _ptr(assigned, C.c_int64), _ptr(is_new, C.c_uint8))
    if rc != 0:
        raise ObviError("%sbbox_frontend_assign failed: status %d" % (prefix, rc))
    return assigned, is_new


class BboxStoreOptions(C.Structure):
    """obvi_bbox_store_options (include/obvi_bbox_store.h); 0: the library's default."""
    _fields_ = [("initial_pool_ids", C.c_int64), ("compact_min_dead_ids", C.c_int64)]


class BboxStoreStatsC(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("owners", "views", "live_ids", "dead_ids", "pool_capacity_ids", "pool_growths", "compactions", "replaced_views", "last_round_upload_bytes")]


BboxStoreStats = collections.namedtuple("BboxStoreStats", [k for k, _ in BboxStoreStatsC._fields_])


class BboxStore:
    """The appearance store of the bounding-box association (include/obvi_bbox_store.h): the views of BundleAdjuster.bbox_associate kept on the device between
    rounds.  It belongs to the BundleAdjuster it was made from and must be closed before it."""

    def __init__(self, ba, initial_pool_ids=0, compact_min_dead_ids=0):
        self._ba = ba
        self._s = C.c_void_p()
        opt = BboxStoreOptions(int(initial_pool_ids), int(compact_min_dead_ids))
        ba._check(self._fn("create")(ba._h, C.byref(opt), C.byref(self._s)), "bbox_store_create")

    def _fn(self, name):
        return self._ba._entry("bbox_store_" + name, "obvi_bbox_store.h")

    def _check(self, rc, what):
        self._ba._check(rc, "bbox_store_" + what)

    def close(self):
        if self._s:
            f = self._fn("destroy")
            f.restype = None
            f(self._s)
            self._s = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def new_owners(self, n):
        out = np.zeros(int(n), np.int64)
        self._check(self._fn("new_owners")(self._s, C.c_int64(int(n)), _ptr(out, C.c_int64)), "new_owners")
        return out

    def put_views(self, owner, frame, camera, views):
        """views: one list of feature ids per (owner[k], frame[k], camera[k])."""
        ow = np.ascontiguousarray(owner, dtype=np.int64).ravel(); fr = np.ascontiguousarray(frame, dtype=np.uint64).ravel(); ca = np.ascontiguousarray(camera, dtype=np.uint64).ravel()
        if not (len(ow) == len(fr) == len(ca) == len(views)):
            raise ObviError("put_views: array lengths disagree")
        fp = np.concatenate([[0], np.cumsum([len(v) for v in views])]).astype(np.uint64)
        vf = np.array([i for v in views for i in v], dtype=np.uint64)
        self._check(self._fn("put_views")(self._s, C.c_int64(len(ow)), _ptr(ow, C.c_int64), _ptr(fr, C.c_uint64), _ptr(ca, C.c_uint64), _ptr(fp, C.c_uint64), _ptr(vf, C.c_uint64)), "put_views")

    def associate(self, feat_id, feat_pixel, box_corners, box_label, cand_owner, cand_label, params=None, want_in_box=True, n_views=None):
        """BundleAdjuster.bbox_associate over the stored views of cand_owner: (in_box, feats_in_box, overlap, is_match, score); in_box is None when not wanted.
        n_views: the candidates' views in all, for a caller that knows; otherwise the store's directory is asked, owner by owner."""
        fi = np.ascontiguousarray(feat_id, dtype=np.uint64).ravel(); fx = _f64(feat_pixel, (-1, 2))
        bc = _f64(box_corners, (-1, 4)); bl = np.ascontiguousarray(box_label, dtype=np.int32).ravel()
        co = np.ascontiguousarray(cand_owner, dtype=np.int64).ravel(); cl = np.ascontiguousarray(cand_label, dtype=np.int32).ravel()
        if len(fx) != len(fi) or len(bl) != len(bc) or len(co) != len(cl):
            raise ObviError("BboxStore.associate: array lengths disagree")
        prm = params or BboxFrontendParams()
        nf, nb, nc = len(fi), len(bc), len(cl)
        if n_views is not None:
            nv = int(n_views)
        else:
            nv = sum(self.view_sizes(int(o))[0] for o in co) if len(set(co.tolist())) == nc else 0   # a refusal is the library's to make
        in_box = np.zeros((nb, nf), np.uint8) if want_in_box else None
        count, overlap = np.zeros(nb, np.uint32), np.zeros((nb, nv), np.uint32)
        match, score = np.zeros((nb, nc), np.uint8), np.full((nb, nc), np.nan)
        self._check(self._fn("associate")(self._s, C.c_int64(nf), _ptr(fi, C.c_uint64), _ptr(fx, C.c_double), C.c_int64(nb), _ptr(bc, C.c_double), _ptr(bl, C.c_int32), C.c_int64(nc),
                                          _ptr(co, C.c_int64), _ptr(cl, C.c_int32), C.byref(prm), _ptr(in_box, C.c_uint8), _ptr(count, C.c_uint32), _ptr(overlap, C.c_uint32),
                                          _ptr(match, C.c_uint8), _ptr(score, C.c_double)), "associate")
        return in_box, count, overlap, match, score

    def commit(self, frame_id, camera_id, box_owner):
        bo = np.ascontiguousarray(box_owner, dtype=np.int64).ravel()
        self._check(self._fn("commit")(self._s, C.c_uint64(int(frame_id)), C.c_uint64(int(camera_id)), C.c_int64(len(bo)), _ptr(bo, C.c_int64)), "commit")

    def merge(self, from_owner, into_owner):
        fr = np.ascontiguousarray(from_owner, dtype=np.int64).ravel(); to = np.ascontiguousarray(into_owner, dtype=np.int64).ravel()
        if len(fr) != len(to):
            raise ObviError("BboxStore.merge: array lengths disagree")
        self._check(self._fn("merge")(self._s, C.c_int64(len(fr)), _ptr(fr, C.c_int64), _ptr(to, C.c_int64)), "merge")

    def release(self, owner):
        ow = np.ascontiguousarray(owner, dtype=np.int64).ravel()
        self._check(self._fn("release")(self._s, C.c_int64(len(ow)), _ptr(ow, C.c_int64)), "release")

    def apply_window(self, frame_id, window):
        dropped = C.c_int64(0)
        self._check(self._fn("apply_window")(self._s, C.c_uint64(int(frame_id)), C.c_uint64(int(window)), C.byref(dropped)), "apply_window")
        return dropped.value

    def compact(self):
        self._check(self._fn("compact")(self._s), "compact")

    def view_sizes(self, owner):
        """(number of views, number of ids) of an owner: the host directory's answer, no device work."""
        nv, ni = C.c_int64(0), C.c_int64(0)
        self._check(self._fn("views")(self._s, C.c_int64(int(owner)), C.byref(nv), C.byref(ni), None, None, None, None), "views")
        return nv.value, ni.value

    def views(self, owner):
        """The owner's views in (frame, camera) order: [((frame, camera), [ids])]."""
        nv, ni = self.view_sizes(owner)
        fr, ca, fp, vf = np.zeros(nv, np.uint64), np.zeros(nv, np.uint64), np.zeros(nv + 1, np.uint64), np.zeros(ni, np.uint64)
        self._check(self._fn("views")(self._s, C.c_int64(int(owner)), None, None, _ptr(fr, C.c_uint64), _ptr(ca, C.c_uint64), _ptr(fp, C.c_uint64), _ptr(vf, C.c_uint64)), "views")
        return [((int(fr[k]), int(ca[k])), [int(i) for i in vf[int(fp[k]):int(fp[k + 1])]]) for k in range(nv)]

    def stats(self):
        st = BboxStoreStatsC()
        self._check(self._fn("get_stats")(self._s, C.byref(st)), "get_stats")
        return BboxStoreStats(*[getattr(st, k) for k in BboxStoreStats._fields])


class BundleAdjuster:
    """One handle == one GPU == one HIP stream (include/obvi_ba.h)."""

    def __init__(self, device_id=0, library=None, prefix="obvi_", reprojection_variant=0, deterministic=False, object_block_size=7):
        path = _library_path(library)
        self._lib = C.CDLL(path)
        self._pre = prefix
        self._h = C.c_void_p()
        self.od = int(object_block_size)                                   # parameters of an ellipsoid block: 7 (yaw only) or 9 (axis-angle)
        opt = Options(device_id, self.od, int(reprojection_variant), 1 if deterministic else 0)
        self._check(self._fn("ba_create")(C.byref(opt), C.byref(self._h)), "create")
        self._keep = []
        self._n = {t: 0 for t in FACTOR_TYPES + (FACTOR_MAP_PAIR_PRIOR, FACTOR_MAP_GROUP_PRIOR)}
        self._mg_sizes = []
        self.P = self.L = self.O = 0

    def _fn(self, name):
        return _entry(self._lib, self._pre, name, restype=C.c_int64 if name in ("ba_num_residuals", "ba_num_factors") else C.c_int)

    def _entry(self, name, header):
        return _entry(self._lib, self._pre, name, header)

    def _check(self, rc, what):
        if rc != 0:
            msg = ""
            try:
                fn = getattr(self._lib, self._pre + "ba_last_error")
                fn.restype = C.c_char_p
                msg = (fn(self._h) or b"").decode()
            except AttributeError:
                pass
            raise ObviError("%s%s failed: status %d %s" % (self._pre, what, rc, msg))

    def close(self):
        if self._h:
            f = getattr(self._lib, self._pre + "ba_destroy")
            f.restype = None
            f(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- upload --------------------------------------------------------------------------
    def set_cameras(self, K, ext):
        K, ext = _f64(K, (-1, 4)), _f64(ext, (-1, 7))
        self._check(self._fn("ba_set_cameras")(self._h, C.c_int32(len(K)), _ptr(K, C.c_double), _ptr(ext, C.c_double)), "set_cameras")

    def _set_blocks(self, name, vals, dim, is_const):
        vals = _f64(vals, (-1, dim))
        c = None if is_const is None else np.ascontiguousarray(is_const, dtype=np.uint8)
        self._check(self._fn(name)(self._h, C.c_int64(len(vals)), _ptr(vals, C.c_double), _ptr(c, C.c_uint8)), name)
        return len(vals)

    def set_poses(self, poses, is_const=None):
        self.P = self._set_blocks("ba_set_poses", poses, 6, is_const)

    def set_points(self, pts, is_const=None):
        self.L = self._set_blocks("ba_set_points", pts, 3, is_const)

    def set_objects(self, objs, is_const=None):
        self.O = self._set_blocks("ba_set_objects", objs, self.od, is_const)

    def set_const_flags(self, pose_const=None, point_const=None, object_const=None):
        a = [None if x is None else np.ascontiguousarray(x, dtype=np.uint8) for x in (pose_const, point_const, object_const)]
        self._check(self._fn("ba_set_const_flags")(self._h, _ptr(a[0], C.c_uint8), _ptr(a[1], C.c_uint8), _ptr(a[2], C.c_uint8)), "set_const_flags")

    def set_reproj(self, pose_idx, point_idx, cam_idx, pixel, sigma, huber):
        pi = np.ascontiguousarray(pose_idx, dtype=np.uint32)
        li = np.ascontiguousarray(point_idx, dtype=np.uint32)
        ci = None if cam_idx is None else np.ascontiguousarray(cam_idx, dtype=np.uint16)
        px = _f64(pixel, (-1, 2))
        if np.isscalar(sigma):
            sg, sscalar = None, float(sigma)
        else:
            sg, sscalar = _f64(sigma), 0.0
        self._check(self._fn("ba_set_reproj")(self._h, C.c_int64(len(pi)), _ptr(pi, C.c_uint32), _ptr(li, C.c_uint32),
                                              _ptr(ci, C.c_uint16), _ptr(px, C.c_double), _ptr(sg, C.c_double),
                                              C.c_double(sscalar), C.c_double(huber)), "set_reproj")
        self._n[FACTOR_REPROJECTION] = len(pi)

    def set_bbox(self, obj_idx, pose_idx, cam_idx, corners, cov, huber, invalid_err):
        oi = np.ascontiguousarray(obj_idx, dtype=np.uint32)
        pi = np.ascontiguousarray(pose_idx, dtype=np.uint32)
        ci = None if cam_idx is None else np.ascontiguousarray(cam_idx, dtype=np.uint16)
        co, cv = _f64(corners, (-1, 4)), _f64(cov, (-1, 16))
        self._check(self._fn("ba_set_bbox")(self._h, C.c_int64(len(oi)), _ptr(oi, C.c_uint32), _ptr(pi, C.c_uint32),
                                            _ptr(ci, C.c_uint16), _ptr(co, C.c_double), _ptr(cv, C.c_double),
                                            C.c_double(huber), C.c_double(invalid_err)), "set_bbox")
        self._n[FACTOR_BBOX] = len(oi)

    def set_shape_priors(self, obj_idx, mean3, cov9, huber):
        oi = np.ascontiguousarray(obj_idx, dtype=np.uint32)
        m, cv = _f64(mean3, (-1, 3)), _f64(cov9, (-1, 9))
        self._check(self._fn("ba_set_shape_priors")(self._h, C.c_int64(len(oi)), _ptr(oi, C.c_uint32), _ptr(m, C.c_double),
                                                    _ptr(cv, C.c_double), C.c_double(huber)), "set_shape_priors")
        self._n[FACTOR_SHAPE_PRIOR] = len(oi)

    def set_ltm_priors(self, obj_idx, mean7, cov49, huber):
        oi = np.ascontiguousarray(obj_idx, dtype=np.uint32)
        m, cv = _f64(mean7, (-1, self.od)), _f64(cov49, (-1, self.od * self.od))
        self._check(self._fn("ba_set_ltm_priors")(self._h, C.c_int64(len(oi)), _ptr(oi, C.c_uint32), _ptr(m, C.c_double),
                                                  _ptr(cv, C.c_double), C.c_double(huber)), "set_ltm_priors")
        self._n[FACTOR_LTM_PRIOR] = len(oi)

    def set_relpose(self, idx_a, idx_b, t3, aa3, cov36, huber):
        ia = np.ascontiguousarray(idx_a, dtype=np.uint32)
        ib = np.ascontiguousarray(idx_b, dtype=np.uint32)
        t, a, cv = _f64(t3, (-1, 3)), _f64(aa3, (-1, 3)), _f64(cov36, (-1, 36))
        self._check(self._fn("ba_set_relpose")(self._h, C.c_int64(len(ia)), _ptr(ia, C.c_uint32), _ptr(ib, C.c_uint32),
                                               _ptr(t, C.c_double), _ptr(a, C.c_double), _ptr(cv, C.c_double),
                                               C.c_double(huber)), "set_relpose")
        self._n[FACTOR_REL_POSE] = len(ia)

    def set_map_pair_priors(self, obj_a, obj_b, mean_a, mean_b, cov_joint, form=None, huber=1.0):
        """Joint Gaussian priors on object pairs (include/obvi_map_prior.h): cov_joint [n][2od][2od]; form None = all joint, else MAP_PAIR_JOINT / MAP_PAIR_CONDITIONAL per pair."""
        f = self._entry("map_set_pair_priors", "obvi_map_prior.h")
        ia = np.ascontiguousarray(obj_a, dtype=np.uint32)
        ib = np.ascontiguousarray(obj_b, dtype=np.uint32)
        n2 = 2 * self.od
        ma, mb, cv = _f64(mean_a, (-1, self.od)), _f64(mean_b, (-1, self.od)), _f64(cov_joint, (-1, n2 * n2))
        fm = None if form is None else np.ascontiguousarray(form, dtype=np.uint8)
        self._check(f(self._h, C.c_int64(len(ia)), _ptr(ia, C.c_uint32), _ptr(ib, C.c_uint32), _ptr(ma, C.c_double), _ptr(mb, C.c_double),
                      _ptr(cv, C.c_double), _ptr(fm, C.c_uint8), C.c_double(huber)), "map_set_pair_priors")
        self._n[FACTOR_MAP_PAIR_PRIOR] = len(ia)

    def set_map_group_priors(self, groups, means, covs, huber=1.0):
        """Joint Gaussian priors on groups of objects (include/obvi_map_group_prior.h): groups = a list of object-index lists, means = per group [k][od],
        covs = per group [k od][k od]; empty lists clear the factors."""
        f = self._entry("map_set_group_priors", "obvi_map_group_prior.h")
        sizes = [len(g) for g in groups]
        ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        idx = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.uint32).ravel() for g in groups]) if groups else np.zeros(0), dtype=np.uint32)
        mu = _f64(np.concatenate([np.asarray(m, dtype=np.float64).reshape(-1, self.od) for m in means]) if groups else np.zeros((0, self.od)), (-1, self.od))
        cv = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float64).ravel() for c in covs]) if groups else np.zeros(0), dtype=np.float64)
        if len(mu) != ptr[-1] or len(cv) != sum((k * self.od) ** 2 for k in sizes):
            raise ObviError("map_set_group_priors: means / covs do not match the groups")
        self._check(f(self._h, C.c_int64(len(sizes)), _ptr(ptr, C.c_int64), _ptr(idx, C.c_uint32), _ptr(mu, C.c_double), _ptr(cv, C.c_double), C.c_double(huber)),
                    "map_set_group_priors")
        self._n[FACTOR_MAP_GROUP_PRIOR] = len(sizes)
        self._mg_sizes = sizes

    def set_map_group_priors_from_map(self, map, groups, map_idx, huber=1.0):
        """Group priors cut from a device-resident map (include/obvi_map_resident.h): groups = a list of object-index lists, map_idx = per group the members' map
        objects; means and covariances are the map's, gathered and factored on the device.  Empty lists clear the factors."""
        f = self._entry("map_set_group_priors_from_map", "obvi_map_resident.h")
        sizes = [len(g) for g in groups]
        ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        idx = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.uint32).ravel() for g in groups]) if groups else np.zeros(0), dtype=np.uint32)
        mid = np.ascontiguousarray(np.concatenate([np.asarray(g, dtype=np.uint32).ravel() for g in map_idx]) if groups else np.zeros(0), dtype=np.uint32)
        if len(mid) != len(idx) or [len(g) for g in map_idx] != sizes:
            raise ObviError("map_set_group_priors_from_map: map_idx does not match the groups")
        self._check(f(self._h, map._m, C.c_int64(len(sizes)), _ptr(ptr, C.c_int64), _ptr(idx, C.c_uint32), _ptr(mid, C.c_uint32), C.c_double(huber)),
                    "map_set_group_priors_from_map")
        self._n[FACTOR_MAP_GROUP_PRIOR] = len(sizes)
        self._mg_sizes = sizes

    def set_active_mask(self, factor_type, mask):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self._check(self._fn("ba_set_active_mask")(self._h, C.c_int32(factor_type), _ptr(m, C.c_uint8)), "set_active_mask")

    # ---- evaluate / solve ----------------------------------------------------------------
    def num_factors(self, t):
        return self._n[t]

    def _residual_dim(self, t):
        return self.od if t == 4 else 2 * self.od if t == 9 else RESIDUAL_DIM[t]        # an LTM prior has one residual per ellipsoid parameter, a map pair prior two

    def num_residuals(self):
        return sum(self._residual_dim(t) * n for t, n in self._n.items() if t != FACTOR_MAP_GROUP_PRIOR) + self.od * sum(self._mg_sizes)   # (a group prior: od per member)

    def evaluate(self, apply_loss=True, want_residuals=True):
        cost = C.c_double(0.0)
        res = np.zeros(self.num_residuals()) if want_residuals else None
        sq = np.zeros(sum(self._n.values())) if want_residuals else None
        self._check(self._fn("ba_evaluate")(self._h, C.c_int32(int(apply_loss)), C.byref(cost), _ptr(res, C.c_double),
                                            _ptr(sq, C.c_double)), "evaluate")
        return cost.value, res, sq

    def solve(self, params):
        s = Summary()
        self._check(self._fn("ba_solve")(self._h, C.byref(params), C.byref(s)), "solve")
        return s

    def iterations(self, cap=4096):
        buf = (IterationSummary * cap)()
        n = self._fn("ba_get_iterations")(self._h, buf, C.c_int32(cap))
        return [buf[i] for i in range(n)]

    def select_outliers(self, factor_type, fraction):
        mask = np.ones(self._n[factor_type], dtype=np.uint8)
        nex = C.c_int64(0)
        self._check(self._fn("ba_select_outliers")(self._h, C.c_int32(factor_type), C.c_double(fraction),
                                                   _ptr(mask, C.c_uint8), C.byref(nex)), "select_outliers")
        return mask, nex.value

    def debug_select(self, sq, active, fraction):
        """obvi_ba_debug_select: the two-phase selection rule on block norms given here (active None: all)."""
        v = np.ascontiguousarray(sq, dtype=np.float64)
        a = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
        mask = np.zeros(len(v), dtype=np.uint8)
        nex = C.c_int64(0)
        self._check(self._fn("ba_debug_select")(self._h, C.c_int64(len(v)), _ptr(v, C.c_double), _ptr(a, C.c_uint8), C.c_double(fraction),
                                                _ptr(mask, C.c_uint8), C.byref(nex)), "debug_select")
        return mask, nex.value

    def object_covariances(self, obj_a, obj_b=None):
        """7x7 covariance blocks of object pairs (obj_b None: the objects' own blocks)."""
        a = np.ascontiguousarray(obj_a, dtype=np.uint32)
        b = a if obj_b is None else np.ascontiguousarray(obj_b, dtype=np.uint32)
        out = np.zeros((len(a), self.od, self.od))
        self._check(self._fn("ba_object_covariances")(self._h, C.c_int64(len(a)), _ptr(a, C.c_uint32), _ptr(b, C.c_uint32),
                                                      _ptr(out, C.c_double)), "object_covariances")
        return out

    # ---- covariance blocks by selected inversion (include/obvi_cov.h; not in the oracle: an oracle-backed adjuster raises) ----
    def covariance_compute(self):
        """Linearise at the current estimate, factorise the undamped reduced system and invert it on the factor's tile pattern."""
        self._check(self._entry("cov_compute", "obvi_cov.h")(self._h), "cov_compute")

    def covariance_compute_pairs(self, kind_a, idx_a, kind_b, idx_b):
        """covariance_compute, after which cross_covariances also serves the pairs declared here: any kinds (0 pose / 1 feature / 2 object), on the pattern or not."""
        ka, ia, kb, ib = self._cov_pairs(kind_a, idx_a, kind_b, idx_b)
        self._check(self._entry("cov_compute_pairs", "obvi_cov.h")(self._h, C.c_int64(len(ia)), _ptr(ka, C.c_uint8), _ptr(ia, C.c_uint32), _ptr(kb, C.c_uint8), _ptr(ib, C.c_uint32)),
                    "cov_compute_pairs")

    def covariance_debug_compute_pairs(self, kind_a=(), idx_a=(), kind_b=(), idx_b=(), lhs_in=None, m_cap=4096):
        """covariance_compute_pairs on these pairs (none: covariance_compute), returning (S, grid_row): the system the pass inverts, canonical order, taken
        between its assembly and its factorisation, and the row of the tile grid of every canonical index.  lhs_in: given values in place of the assembly.
        A non-positive pivot or a NaN raises with status -6, an asymmetric system or an entry outside the structural tile mask with status -1."""
        ka, ia, kb, ib = self._cov_pairs(kind_a, idx_a, kind_b, idx_b)
        if lhs_in is not None:
            lin = _f64(lhs_in)
            if lin.ndim != 2 or lin.shape[0] != lin.shape[1]:
                raise ObviError("cov_debug_compute_pairs: lhs_in is not square")
            m_cap = len(lin)                      # (a handle whose system has more rows refuses; fewer is caught below)
        lhs, row = np.zeros((m_cap, m_cap)), np.full(m_cap, -1, dtype=np.int32)
        m = C.c_int32(0)
        rc = self._entry("cov_debug_compute_pairs", "obvi_cov.h")(self._h, C.c_int64(len(ia)), _ptr(ka, C.c_uint8), _ptr(ia, C.c_uint32), _ptr(kb, C.c_uint8), _ptr(ib, C.c_uint32),
                                                     _ptr(lin, C.c_double) if lhs_in is not None else None, _ptr(lhs, C.c_double), _ptr(row, C.c_int32),
                                                     C.c_int32(m_cap), C.byref(m))
        if lhs_in is not None and rc in (0, -6) and m.value != len(lin):
            raise ObviError("cov_debug_compute_pairs: the given system has %d rows, the handle's reduced system %d" % (len(lin), m.value))
        self._check(rc, "cov_debug_compute_pairs")
        mm = m.value
        return lhs.ravel()[:mm * mm].reshape(mm, mm).copy(), row[:mm].copy()

    def _cov_own(self, name, idx, dim):
        i = np.ascontiguousarray(idx, dtype=np.uint32)
        out = np.zeros((len(i), dim, dim))
        self._check(self._entry(name, "obvi_cov.h")(self._h, C.c_int64(len(i)), _ptr(i, C.c_uint32), _ptr(out, C.c_double)), name)
        return out

    def pose_covariances(self, idx):
        return self._cov_own("cov_pose_blocks", idx, 6)

    def point_covariances(self, idx):
        return self._cov_own("cov_point_blocks", idx, 3)

    def object_covariance_blocks(self, idx):
        return self._cov_own("cov_object_blocks", idx, self.od)

    def _cov_pairs(self, kind_a, idx_a, kind_b, idx_b):
        ia, ib = np.ascontiguousarray(idx_a, dtype=np.uint32), np.ascontiguousarray(idx_b, dtype=np.uint32)
        ka = np.ascontiguousarray(np.broadcast_to(np.asarray(kind_a, dtype=np.uint8), ia.shape))
        kb = np.ascontiguousarray(np.broadcast_to(np.asarray(kind_b, dtype=np.uint8), ib.shape))
        return ka, ia, kb, ib

    def cross_covariances(self, kind_a, idx_a, kind_b, idx_b):
        """Cross blocks of pairs of poses (kind 0) / objects (kind 2) on the factor's tile pattern, and of every pair declared to covariance_compute_pairs
        (features, kind 1, included): a list of dim(a) x dim(b) arrays."""
        ka, ia, kb, ib = self._cov_pairs(kind_a, idx_a, kind_b, idx_b)
        dim = lambda k: np.where(k == 0, 6, np.where(k == 1, 3, self.od)).astype(np.int64)
        sz = dim(ka) * dim(kb)
        off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sz)]).astype(np.int64))
        out = np.zeros(int(off[-1]))
        self._check(self._entry("cov_cross_blocks", "obvi_cov.h")(self._h, C.c_int64(len(ia)), _ptr(ka, C.c_uint8), _ptr(ia, C.c_uint32), _ptr(kb, C.c_uint8), _ptr(ib, C.c_uint32),
                                                     _ptr(out, C.c_double), _ptr(off, C.c_int64)), "cov_cross_blocks")
        da, db = dim(ka), dim(kb)
        return [out[off[i]:off[i + 1]].reshape(da[i], db[i]) for i in range(len(ia))]

    def covariance_on_pattern(self, kind_a, idx_a, kind_b, idx_b):
        """1 per pair whose cross block cross_covariances can serve."""
        ka, ia, kb, ib = self._cov_pairs(kind_a, idx_a, kind_b, idx_b)
        on = np.zeros(len(ia), dtype=np.uint8)
        self._check(self._entry("cov_on_pattern", "obvi_cov.h")(self._h, C.c_int64(len(ia)), _ptr(ka, C.c_uint8), _ptr(ia, C.c_uint32), _ptr(kb, C.c_uint8), _ptr(ib, C.c_uint32),
                                                   _ptr(on, C.c_uint8)), "cov_on_pattern")
        return on

    def covariance_stats(self):
        """(linearise + factorise ms, selected inversion ms, scratch bytes) of the last covariance_compute."""
        a, b, n = C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
        self._check(self._entry("cov_get_stats", "obvi_cov.h")(self._h, C.byref(a), C.byref(b), C.byref(n)), "cov_get_stats")
        return a.value, b.value, n.value

    def set_parameter_priors(self, block_kind, block_idx, param_idx, mean, std_dev):
        """ParameterPrior factors for the covariance extraction: kind 0 pose / 1 point / 2 object; empty arrays clear them."""
        k = np.ascontiguousarray(block_kind, dtype=np.uint8); b = np.ascontiguousarray(block_idx, dtype=np.uint32)
        q = np.ascontiguousarray(param_idx, dtype=np.uint8); m, sd = _f64(mean), _f64(std_dev)
        self._check(self._fn("ba_set_parameter_priors")(self._h, C.c_int64(len(k)), _ptr(k, C.c_uint8), _ptr(b, C.c_uint32), _ptr(q, C.c_uint8),
                                                        _ptr(m, C.c_double), _ptr(sd, C.c_double)), "set_parameter_priors")

    def column_sqnorms(self):
        """squared column norms of the robustified Jacobian per scalar parameter: (poses [P,6], points [L,3], objects [O,7]); -1 = not a parameter of the problem"""
        p, l, o = np.zeros((self.P, 6)), np.zeros((self.L, 3)), np.zeros((self.O, self.od))
        self._check(self._fn("ba_column_sqnorms")(self._h, _ptr(p, C.c_double), _ptr(l, C.c_double), _ptr(o, C.c_double)), "column_sqnorms")
        return p, l, o

    # ---- visual-feature front-end gating (include/obvi_frontend.h) --------------------------
    def epipolar_votes(self, K, ext, poses, cand_pose, cand_cam, cand_pixel, ref_ptr, ref_pose, ref_cam, ref_pixel, ref_frame, ref_skip, params=None):
        K, ext, poses = _f64(K, (-1, 4)), _f64(ext, (-1, 7)), _f64(poses, (-1, 6))
        cp = np.ascontiguousarray(cand_pose, dtype=np.uint32); cc = np.ascontiguousarray(cand_cam, dtype=np.uint16); cx = _f64(cand_pixel, (-1, 2))
        rp = np.ascontiguousarray(ref_ptr, dtype=np.uint64); ro = np.ascontiguousarray(ref_pose, dtype=np.uint32); rc = np.ascontiguousarray(ref_cam, dtype=np.uint16)
        rx = _f64(ref_pixel, (-1, 2)); rf = np.ascontiguousarray(ref_frame, dtype=np.uint32); rs = np.ascontiguousarray(ref_skip, dtype=np.uint8)
        prm = params or EpipolarParams()
        n = len(cp)
        votes, voters, inl = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        self._check(self._entry("frontend_epipolar_votes", "obvi_frontend.h")(self._h, C.c_int32(len(K)), _ptr(K, C.c_double), _ptr(ext, C.c_double), C.c_int64(len(poses)), _ptr(poses, C.c_double),
                                                                C.c_int64(n), _ptr(cp, C.c_uint32), _ptr(cc, C.c_uint16), _ptr(cx, C.c_double), _ptr(rp, C.c_uint64), _ptr(ro, C.c_uint32),
                                                                _ptr(rc, C.c_uint16), _ptr(rx, C.c_double), _ptr(rf, C.c_uint32), _ptr(rs, C.c_uint8), C.byref(prm),
                                                                _ptr(votes, C.c_uint32), _ptr(voters, C.c_uint32), _ptr(inl, C.c_uint8)), "frontend_epipolar_votes")
        return votes, voters, inl

    def epipolar_errors(self, K, ext, poses, cand_pose, cand_cam, cand_pixel, ref_ptr, ref_pose, ref_cam, ref_pixel):
        K, ext, poses = _f64(K, (-1, 4)), _f64(ext, (-1, 7)), _f64(poses, (-1, 6))
        cp = np.ascontiguousarray(cand_pose, dtype=np.uint32); cc = np.ascontiguousarray(cand_cam, dtype=np.uint16); cx = _f64(cand_pixel, (-1, 2))
        rp = np.ascontiguousarray(ref_ptr, dtype=np.uint64); ro = np.ascontiguousarray(ref_pose, dtype=np.uint32); rc = np.ascontiguousarray(ref_cam, dtype=np.uint16)
        rx = _f64(ref_pixel, (-1, 2))
        err = np.zeros((len(ro), 2))
        self._check(self._entry("frontend_epipolar_errors", "obvi_frontend.h")(self._h, C.c_int32(len(K)), _ptr(K, C.c_double), _ptr(ext, C.c_double), C.c_int64(len(poses)), _ptr(poses, C.c_double),
                                                                 C.c_int64(len(cp)), _ptr(cp, C.c_uint32), _ptr(cc, C.c_uint16), _ptr(cx, C.c_double), _ptr(rp, C.c_uint64), _ptr(ro, C.c_uint32),
                                                                 _ptr(rc, C.c_uint16), _ptr(rx, C.c_double), _ptr(err, C.c_double)), "frontend_epipolar_errors")
        return err

    def parallax(self, frame_ptr, has_pose, poses, obs_ptr, pixels, params=None):
        fp = np.ascontiguousarray(frame_ptr, dtype=np.uint64); hp = np.ascontiguousarray(has_pose, dtype=np.uint8); po = _f64(poses, (-1, 6))
        op = np.ascontiguousarray(obs_ptr, dtype=np.uint64); px = _f64(pixels, (-1, 2))
        prm = params or ParallaxParams()
        out = np.zeros(len(fp) - 1, np.uint8)
        self._check(self._entry("frontend_parallax", "obvi_frontend.h")(self._h, C.c_int64(len(fp) - 1), _ptr(fp, C.c_uint64), _ptr(hp, C.c_uint8), _ptr(po, C.c_double), _ptr(op, C.c_uint64),
                                                          _ptr(px, C.c_double), C.byref(prm), _ptr(out, C.c_uint8)), "frontend_parallax")
        return out

    # ---- bounding-box data association (include/obvi_bbox_frontend.h) ---------------------------
    def bbox_associate(self, feat_id, feat_pixel, box_corners, box_label, cand_label, view_ptr, feat_ptr, view_feat, params=None):
        """One (frame, camera) round up to the assignment: (in_box [n_box][n_feat], feats_in_box [n_box], overlap [n_box][n_views], is_match [n_box][n_cand],
        score [n_box][n_cand]); score is NaN where is_match is 0 (the library writes it only where there is a match)."""
        fi = np.ascontiguousarray(feat_id, dtype=np.uint64).ravel(); fx = _f64(feat_pixel, (-1, 2))
        bc = _f64(box_corners, (-1, 4)); bl = np.ascontiguousarray(box_label, dtype=np.int32).ravel(); cl = np.ascontiguousarray(cand_label, dtype=np.int32).ravel()
        vp = np.ascontiguousarray(view_ptr, dtype=np.uint64).ravel(); fp = np.ascontiguousarray(feat_ptr, dtype=np.uint64).ravel()
        vf = np.ascontiguousarray(view_feat, dtype=np.uint64).ravel()
        if len(fx) != len(fi) or len(bl) != len(bc) or len(vp) != len(cl) + 1 or len(fp) < 1:
            raise ObviError("bbox_associate: array lengths disagree")
        prm = params or BboxFrontendParams()
        nf, nb, nc, nv = len(fi), len(bc), len(cl), len(fp) - 1
        in_box, count, overlap = np.zeros((nb, nf), np.uint8), np.zeros(nb, np.uint32), np.zeros((nb, nv), np.uint32)
        match, score = np.zeros((nb, nc), np.uint8), np.full((nb, nc), np.nan)
        self._check(self._entry("bbox_frontend_associate", "obvi_bbox_frontend.h")(self._h, C.c_int64(nf), _ptr(fi, C.c_uint64), _ptr(fx, C.c_double), C.c_int64(nb), _ptr(bc, C.c_double), _ptr(bl, C.c_int32),
                                                                C.c_int64(nc), _ptr(cl, C.c_int32), C.c_int64(nv), _ptr(vp, C.c_uint64), C.c_int64(len(vf)), _ptr(fp, C.c_uint64),
                                                                _ptr(vf, C.c_uint64), C.byref(prm), _ptr(in_box, C.c_uint8), _ptr(count, C.c_uint32), _ptr(overlap, C.c_uint32),
                                                                _ptr(match, C.c_uint8), _ptr(score, C.c_double)), "bbox_frontend_associate")
        return in_box, count, overlap, match, score

    # ---- state ---------------------------------------------------------------------------
    def reset(self):
        """obvi_ba_reset: the handle as create left it (no problem, no hook, nothing shared), allocations kept."""
        self._check(self._fn("ba_reset")(self._h), "reset")
        self._n = {t: 0 for t in FACTOR_TYPES + (FACTOR_MAP_PAIR_PRIOR, FACTOR_MAP_GROUP_PRIOR)}
        self._mg_sizes = []
        self.P = self.L = self.O = 0
        self._keep.clear()

    def snapshot(self):
        self._check(self._fn("ba_snapshot")(self._h), "snapshot")

    def restore(self):
        self._check(self._fn("ba_restore")(self._h), "restore")

    def _get(self, name, n, dim):
        out = np.zeros((n, dim))
        self._check(self._fn(name)(self._h, _ptr(out, C.c_double)), name)
        return out

    def get_poses(self):
        return self._get("ba_get_poses", self.P, 6)

    def get_points(self):
        return self._get("ba_get_points", self.L, 3)

    def get_objects(self):
        return self._get("ba_get_objects", self.O, self.od)

    def get_state(self):
        """(poses, points, objects) with one wait for the device (obvi_ba_get_state)."""
        po, pt, ob = np.zeros((self.P, 6)), np.zeros((self.L, 3)), np.zeros((self.O, self.od))
        self._check(self._fn("ba_get_state")(self._h, _ptr(po, C.c_double), _ptr(pt, C.c_double), _ptr(ob, C.c_double)), "get_state")
        return po, pt, ob

    def update_points(self, xyz):
        x = _f64(xyz, (-1, 3))
        self._check(self._fn("ba_update_points")(self._h, C.c_int64(len(x)), _ptr(x, C.c_double)), "update_points")

    def update_state(self, poses=None, points=None, objects=None):
        """Values only (obvi_ba_update_state): constness, factors and the symbolic plan stay."""
        po = None if poses is None else _f64(poses, (self.P, 6))
        pt = None if points is None else _f64(points, (self.L, 3))
        ob = None if objects is None else _f64(objects, (self.O, self.od))
        self._check(self._fn("ba_update_state")(self._h, _ptr(po, C.c_double), _ptr(pt, C.c_double), _ptr(ob, C.c_double)), "update_state")

    def prepare(self):
        """The symbolic phase now (obvi_ba_prepare) instead of inside the first solve / evaluate."""
        self._check(self._fn("ba_prepare")(self._h), "prepare")

    # ---- multi-GPU / test hooks ----------------------------------------------------------
    def set_allreduce(self, pyfunc):
        """pyfunc(device_ptr:int, count_f64:int, op:int (0 sum, 1 max), stream:int) -> int (0 = ok)."""
        if pyfunc is None:
            cb = C.cast(None, ALLREDUCE_FN)
        else:
            cb = ALLREDUCE_FN(lambda user, buf, count, op, stream: int(pyfunc(buf or 0, count, op, stream or 0)))
        self._keep.append(cb)
        self._check(self._fn("ba_set_allreduce")(self._h, cb, None), "set_allreduce")

    def set_shared_objects(self, is_shared, rank, world):
        m = None if is_shared is None else np.ascontiguousarray(is_shared, dtype=np.uint8)
        self._check(self._fn("ba_set_shared_objects")(self._h, _ptr(m, C.c_uint8), C.c_int32(rank), C.c_int32(world)), "set_shared_objects")

    def map_allow_exchange(self, on=True):
        """Joint map priors and Map.condition_on / extend_on / from_handle on a handle that exchanges shared objects (include/obvi_map_shared.h): off by default."""
        f = self._entry("map_allow_exchange", "obvi_map_shared.h")
        self._check(f(self._h, C.c_int32(int(on))), "map_allow_exchange")

    def measure_peaks(self):
        """HBM triad / copy / read bandwidth (GB/s) and the fp64 MFMA rates (TFLOP/s) of this device (obvi_ba_measure_peaks)."""
        class Peaks(C.Structure):
            _fields_ = [("hbm_triad_gbs", C.c_double), ("hbm_copy_gbs", C.c_double), ("hbm_read_gbs", C.c_double), ("mfma_f64_issue_tflops", C.c_double),
                        ("mfma_f64_tile_tflops", C.c_double), ("clock_mhz", C.c_double), ("compute_units", C.c_int32), ("reserved", C.c_int32)]
        p = Peaks()
        self._check(self._fn("ba_measure_peaks")(self._h, C.byref(p)), "measure_peaks")
        return {name: getattr(p, name) for name, _ in Peaks._fields_ if name != "reserved"}

    def debug_linearize(self, factor_type):
        if factor_type == FACTOR_MAP_GROUP_PRIOR:       # r of all groups, and per group its lower triangular W; no second block
            rows = [self.od * k for k in self._mg_sizes]
            r, W = np.zeros(sum(rows)), np.zeros(sum(n * n for n in rows))
            self._check(self._fn("ba_debug_linearize")(self._h, C.c_int32(factor_type), _ptr(r, C.c_double), _ptr(W, C.c_double), None), "debug_linearize")
            ro, wo = np.concatenate([[0], np.cumsum(rows)]).astype(int), np.concatenate([[0], np.cumsum([n * n for n in rows])]).astype(int)
            return [r[ro[g]:ro[g + 1]] for g in range(len(rows))], [W[wo[g]:wo[g + 1]].reshape(rows[g], rows[g]) for g in range(len(rows))], None
        n, m = self._n[factor_type], self._residual_dim(factor_type)
        d0, d1 = (self.od if d == 7 else d for d in BLOCK_DIMS[factor_type])
        r, J0 = np.zeros((n, m)), np.zeros((n, m, d0))
        J1 = np.zeros((n, m, d1)) if d1 else None
        self._check(self._fn("ba_debug_linearize")(self._h, C.c_int32(factor_type), _ptr(r, C.c_double),
                                                   _ptr(J0, C.c_double), _ptr(J1, C.c_double)), "debug_linearize")
        return r, J0, J1

    def debug_reduced_system(self, radius, m_cap=4096):
        lhs, rhs = np.zeros((m_cap, m_cap)), np.zeros(m_cap)
        m = C.c_int32(0)
        self._check(self._fn("ba_debug_reduced_system")(self._h, C.c_double(radius), _ptr(lhs, C.c_double),
                                                        _ptr(rhs, C.c_double), C.c_int32(m_cap), C.byref(m)), "debug_reduced_system")
        mm = m.value
        return lhs.ravel()[:mm * mm].reshape(mm, mm).copy(), rhs[:mm].copy()

    def debug_reduced_solve(self, radius, lhs_in=None, rhs_in=None, m_cap=4096):
        """(status, lhs, rhs, y, grid_row) of obvi_ba_debug_reduced_solve: lhs * y = rhs, canonical order.  status is OBVI_OK (0) or OBVI_ERR_NUMERICAL (-6: the
        step's scalar block reports a non-positive pivot or a non-finite entry); any other status raises.  lhs_in / rhs_in: a given system in place of the assembly."""
        if (lhs_in is None) != (rhs_in is None):
            raise ObviError("debug_reduced_solve: give both lhs_in and rhs_in, or neither")
        if lhs_in is not None:
            rin = _f64(rhs_in, (-1,))
            lin = _f64(lhs_in, (len(rin), len(rin)))
            m_cap = len(rin)                      # (a handle whose system has more rows refuses; fewer is caught below)
        lhs, rhs, y, row = np.zeros((m_cap, m_cap)), np.zeros(m_cap), np.zeros(m_cap), np.full(m_cap, -1, dtype=np.int32)
        m = C.c_int32(0)
        rc = self._fn("ba_debug_reduced_solve")(self._h, C.c_double(radius), _ptr(lin, C.c_double) if lhs_in is not None else None,
                                                _ptr(rin, C.c_double) if lhs_in is not None else None, _ptr(lhs, C.c_double), _ptr(rhs, C.c_double),
                                                _ptr(y, C.c_double), _ptr(row, C.c_int32), C.c_int32(m_cap), C.byref(m))
        if rc != -6:
            self._check(rc, "debug_reduced_solve")
        mm = m.value
        if lhs_in is not None and mm != len(rin):
            raise ObviError("debug_reduced_solve: the given system has %d rows, the handle's reduced system %d" % (len(rin), mm))
        return rc, lhs.ravel()[:mm * mm].reshape(mm, mm).copy(), rhs[:mm].copy(), y[:mm].copy(), row[:mm].copy()

    def problem_stats(self):
        buf = (C.c_double * 23)()
        n = self._fn("ba_get_problem_stats")(self._h, buf, C.c_int32(23))
        names = ["poses_var", "objects_var", "points_var", "reduced_rows", "tiles_per_dim", "schur_blocks", "schur_pairs",
                 "tiles_nonzero", "trsm_jobs", "update_jobs", "chol_flops", "reproj_active", "bbox_active", "chol_levels", "host_threads", "usable_cpus",
                 "potrf_wait_timeouts", "fused_potrf", "point_pieces", "long_points", "schur_pairs_blocks", "schur_batches", "schur_group_cols"]
        return {names[i]: buf[i] for i in range(n)}

    def set_profiling(self, level):
        self._check(self._fn("ba_set_profiling")(self._h, C.c_int32(level)), "set_profiling")

    def kernel_times(self, cap=64):
        names = C.create_string_buffer(4096)
        ms = (C.c_double * cap)()
        cnt = (C.c_int64 * cap)()
        n = self._fn("ba_get_kernel_times")(self._h, names, C.c_int32(4096), ms, cnt, C.c_int32(cap))
        parts = names.raw.split(b"\0")[:n]
        return {parts[i].decode(): (ms[i], cnt[i]) for i in range(n)}
