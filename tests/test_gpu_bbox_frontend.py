"""GPU: one association round of include/obvi_bbox_frontend.h against the restatement of tests/bbox_frontend_cases.py.  The integer outputs (in_box, feats_in_box,
overlap, is_match) must equal it exactly; a score, where is_match is 1, within (V + 2) 2^-53 relative, V the candidate's number of views -- a bound derived from
the V - 1 additions and the divisions (cases.score_bound), not measured; scores elsewhere are not read.  The sizes are the smallest at which the kernels can go
wrong: the wavefront (64 lanes) and bit-row word (64 boxes) edges, the LDS staging limit of the overlap pass taken from the library, empty ranges of both CSR
levels at the start, in the middle and at the end."""
import ctypes as C

import numpy as np
import pytest

import bbox_frontend_cases as cases
import helpers
import obvi_ba

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ba():
    h = helpers.product_ba()
    yield h
    h.close()


def lds_limit():
    lib = C.CDLL(helpers.PRODUCT_LIB)
    lib.obvi_bbox_frontend_lds_feature_limit.restype = C.c_int64
    return int(lib.obvi_bbox_frontend_lds_feature_limit())


def associate(ba, case):
    return ba.bbox_associate(*cases.arrays(case), params=obvi_ba.BboxFrontendParams(case["inflation"], case["min_overlap"]))


def check(ba, case, r=None):
    """One call against the restatement; returns (restated round, outputs)."""
    r = r or cases.restate(case)
    in_box, count, overlap, match, score = associate(ba, case)
    assert np.array_equal(in_box, r.in_box)
    assert np.array_equal(count, r.count)
    assert np.array_equal(overlap, r.overlap)
    assert np.array_equal(match, r.is_match)
    worst = 0.0
    for b, c in zip(*np.nonzero(r.is_match)):
        want, bound = float(r.score[b, c]), cases.score_bound(int(r.n_views_of[c]))
        worst = max(worst, abs(float(score[b, c]) - want) / (bound * want) if want > 0 else float(score[b, c] != 0.0))
        assert abs(float(score[b, c]) - want) <= bound * want, (b, c, float(score[b, c]), want)
    assert np.isnan(score[r.is_match == 0]).all()                                    # written only where there is a match
    print("%d features, %d boxes, %d candidates, %d views: %d matches, largest score error %.2f of its bound" %
          (in_box.shape[1], in_box.shape[0], match.shape[1], overlap.shape[1], int(r.is_match.sum()), worst))
    return r, (in_box, count, overlap, match, score)


MIXED = [[3, 10], [], [20, 1, 7], [5], [], [12, 12, 2]]                             # view sizes of six candidates, two of them without views


@pytest.mark.parametrize("n_feat", [0, 1, 63, 64, 65, 200])
def test_the_number_of_frame_features(ba, n_feat):
    r, _ = check(ba, cases.make_case(100 + n_feat, n_feat, 5, MIXED))
    assert n_feat < 63 or (r.overlap.sum() > 0 and r.count.max() > 0)


@pytest.mark.parametrize("offset", [-1, 0, 1])
def test_both_sides_of_the_lds_staging_limit(ba, offset):
    n_feat = lds_limit() + offset
    r, _ = check(ba, cases.make_case(200 + offset, n_feat, 3, [[40, 64, 5], [129], [], [12]], n_labels=1))
    assert r.overlap.sum() > 0 and r.is_match.sum() > 0


def test_view_sizes_around_the_wavefront_within_one_call(ba):
    r, _ = check(ba, cases.make_case(300, 200, 4, [[0, 1, 63], [64, 65, 129], [129, 0], [0]], n_labels=1))
    assert (r.overlap.max(axis=0) > 0).sum() >= 4


@pytest.mark.parametrize("n_box", [0, 1, 63, 64, 65])
def test_the_number_of_boxes_around_the_bit_row_word(ba, n_box):
    r, _ = check(ba, cases.make_case(400 + n_box, 100, n_box, MIXED))
    assert n_box == 0 or r.overlap.sum() > 0
    if n_box == 65:
        assert r.count[64] > 0 and r.overlap[64].sum() > 0                           # the box in the second word is not an empty one


def mixed_candidates(n_cand, rng):
    """Candidates of 0, 1 and 70 views in turn, the first and the last without views: view_ptr has empty ranges at the start, in the middle and at the end."""
    sizes = []
    for c in range(n_cand):
        n_views = 0 if c in (0, n_cand - 1) else (70, 1, 0)[c % 3]
        sizes.append([int(s) for s in rng.integers(0, 7, n_views)])
    return sizes


@pytest.mark.parametrize("which", ["none", "one_without_views", "one_with_70_views", "65_mixed"])
def test_the_number_of_candidates_and_empty_view_ranges(ba, which):
    rng = np.random.default_rng(77)
    sizes = {"none": [], "one_without_views": [[]], "one_with_70_views": [[int(s) for s in rng.integers(0, 7, 70)]], "65_mixed": mixed_candidates(65, rng)}[which]
    r, _ = check(ba, cases.make_case(500 + len(sizes), 120, 4, sizes, n_labels=1, min_overlap=1.0))
    assert which != "one_with_70_views" or r.is_match.sum() > 0
    if which == "65_mixed":
        assert [len(s) for s in sizes[:4]] == [0, 1, 0, 70] and len(sizes[-1]) == 0 and r.is_match.sum() > 0
        assert r.is_match[:, [0, 64]].sum() == 0


def test_the_closed_set_edges(ba):
    """Corners, inflation and pixels exactly representable: a pixel on each of the four inflated edges and on two corners is inside, the next double outward is
    outside; the same with no inflation."""
    lo, hi = -np.inf, np.inf
    for inflation in (2.5, 0.0):
        x0, x1, y0, y1 = 100.0 - inflation, 200.0 + inflation, 50.0 - inflation, 80.0 + inflation
        inside = [(x0, 60.0), (x1, 60.0), (150.0, y0), (150.0, y1), (x0, y0), (x1, y1)]
        outside = [(np.nextafter(x0, lo), 60.0), (np.nextafter(x1, hi), 60.0), (150.0, np.nextafter(y0, lo)), (150.0, np.nextafter(y1, hi)),
                   (np.nextafter(x0, lo), y0), (x1, np.nextafter(y1, hi))]
        case = dict(feat_id=list(range(10, 22)), feat_pixel=np.array(inside + outside), box_corners=[[100.0, 200.0, 50.0, 80.0]], box_label=[0], cand_label=[0],
                    views=[[list(range(10, 22))]], inflation=inflation, min_overlap=2.0)
        r, (in_box, count, overlap, match, score) = check(ba, case)
        assert list(in_box[0]) == [1] * 6 + [0] * 6 and count[0] == 6 and overlap[0, 0] == 6 and match[0, 0] == 1
        assert score[0, 0] == 6.0 / 12.0


def test_feature_ids_above_32_and_63_bits(ba):
    """Ids that differ from a frame id in the top bit alone, or above bit 32 alone, are other features: a signed or 32-bit compare in the search finds them."""
    top = cases.TOP
    frame = [1, 2, 3, top | 1, top | 2, (1 << 32) + 1, (1 << 32) + 2, 1 << 40, (1 << 64) - 1]
    case = dict(feat_id=frame, feat_pixel=[[10.0 + i, 10.0] for i in range(len(frame))], box_corners=[[0.0, 100.0, 0.0, 100.0]], box_label=[0], cand_label=[0, 0, 0],
                views=[[[top | 1, top | 2, 3], [top | 3, (1 << 32) + 3, (1 << 33) | 1, (1 << 40) | top, (1 << 63)]], [[(1 << 64) - 1, 1 << 40, (1 << 32) + 1, 0]], [list(reversed(frame))]],
                inflation=0.0, min_overlap=1.0)
    r, (in_box, count, overlap, match, score) = check(ba, case)
    assert count[0] == len(frame) and list(overlap[0]) == [3, 0, 3, len(frame)] and list(match[0]) == [1, 1, 1]
    check(ba, dict(case, feat_id=list(reversed(frame))))                             # the caller's order is any order


def test_the_overlap_threshold_is_a_double_and_the_label_decides_first(ba):
    frame = list(range(1, 9))
    base = dict(feat_id=frame, feat_pixel=[[10.0 + i, 10.0] for i in range(8)], box_corners=[[0.0, 100.0, 0.0, 100.0]], box_label=[4], cand_label=[4, 4, 5],
                views=[[[1, 2, 90], [3, 91]], [[1, 92], [4, 5, 6]], [frame]], inflation=0.0)          # best overlaps 2, 3, and 8 under another label
    for min_overlap, want in ((2.0, [1, 1, 0]), (2.5, [0, 1, 0]), (3.0, [0, 1, 0]), (3.5, [0, 0, 0])):
        r, (_, _, overlap, match, _) = check(ba, dict(base, min_overlap=min_overlap))
        assert list(overlap[0]) == [2, 1, 1, 3, 8] and list(match[0]) == want, min_overlap


def test_default_and_deterministic_handles_give_the_same_bytes(ba):
    case, _ = cases.scene()
    det = helpers.product_ba(deterministic=True)
    a, b = associate(ba, case), associate(det, case)
    det.close()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_one_round_through_associate_and_assign(ba):
    """3 classes, 12 objects, 40 earlier views, 9 boxes, 300 features.  The restatement's competing scores are first shown to lie further apart than 100 times the
    bound of the score check, so that a different assignment could not be blamed on rounding."""
    case, r = cases.scene()
    assert cases.competing_scores_are_apart(r, 100.0)
    _, (_, _, _, match, score) = check(ba, case, r)
    assigned, is_new = obvi_ba.bbox_assign(match, score, case["n_pending"], library=helpers.PRODUCT_LIB)
    want = cases.assign_restated(r, case["n_pending"])
    assert [(bool(n), int(a)) for a, n in zip(assigned, is_new)] == want
    assert any(new for new, _ in want) and any(not new for new, _ in want)


def test_the_refusals_beside_a_live_handle_and_outputs_left_out(ba):
    last_error = ba._lib.obvi_ba_last_error
    last_error.restype = C.c_char_p
    for name, change, status in cases.REFUSALS:
        c = cases.Call()
        change(c)
        assert c.run(ba._h) == status and c.untouched(), name
        assert b"bbox associate" in last_error(ba._h), name
    c = cases.Call()                                                                 # the call they all spoil is a valid one
    assert c.run(ba._h) == 0
    assert list(c.out["in_box"][0]) == [1, 0] and c.out["feats_in_box"][0] == 1 and list(c.out["overlap"][0]) == [1, 1, 0]
    assert list(c.out["is_match"][0]) == [0, 0] and (c.out["score"] == cases.SENTINEL).all()          # no match: no score written
    c = cases.Call()
    c.a["params"][1] = 1.0
    for k in ("in_box", "feats_in_box", "overlap"):
        c.out[k] = None
    assert c.run(ba._h) == 0 and list(c.out["is_match"][0]) == [1, 0]
    assert c.out["score"][0, 0] == (1.0 / 1.0 + 1.0 / 2.0) / 2.0 and c.out["score"][0, 1] == cases.SENTINEL
    c = cases.Call()
    for k in c.out:
        c.out[k] = None
    assert c.run(ba._h) == 0
