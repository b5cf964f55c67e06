"""CPU: the appearance store of the bounding-box association (include/obvi_bbox_store.h) is declared under the obvi_bbox_store_ prefix in a header of its own,
exported by libobvi_ba.so and bound in obvi_ba.py; every entry answers a NULL store or a NULL required pointer with OBVI_ERR_INVALID_ARGUMENT before it looks at
anything else, outputs untouched; the model of tests/bbox_store_cases.py is held on a hand-computed sequence; and the session of the GPU test shows, from the
model alone, the growths, compactions, replaced and empty views it is there for.  (The store on a device: tests/test_gpu_bbox_store.py.)"""
import ctypes as C
import os
import sys

import numpy as np

import bbox_frontend_cases as cases
import bbox_store_cases as store_cases
import helpers

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

SYMBOLS = ["obvi_bbox_store_apply_window", "obvi_bbox_store_associate", "obvi_bbox_store_commit", "obvi_bbox_store_compact", "obvi_bbox_store_create",
           "obvi_bbox_store_destroy", "obvi_bbox_store_get_stats", "obvi_bbox_store_merge", "obvi_bbox_store_new_owners", "obvi_bbox_store_put_views",
           "obvi_bbox_store_release", "obvi_bbox_store_views"]
SENTINEL = cases.SENTINEL
INVALID = -1


def test_the_header_declares_the_entries_the_library_exports_them_and_the_binding_has_a_method_for_each():
    assert entry.abi_symbols("obvi_bbox_store.h", "obvi_bbox_store_") == SYMBOLS
    assert entry.abi_symbols("obvi_bbox_store.h", "obvi_ba_") == []
    assert '#include "obvi_bbox_frontend.h"' in open(os.path.join(helpers.ROOT, "include", "obvi_bbox_store.h")).read()
    lib = C.CDLL(helpers.PRODUCT_LIB)
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    import obvi_ba
    for m in ("new_owners", "put_views", "associate", "commit", "merge", "release", "apply_window", "compact", "views", "stats", "close"):
        assert callable(getattr(obvi_ba.BboxStore, m, None)), m
    assert [k for k, _ in obvi_ba.BboxStoreStatsC._fields_] == list(store_cases.STATS) + ["last_round_upload_bytes"]


def lib():
    out = C.CDLL(helpers.PRODUCT_LIB)
    for s in SYMBOLS:
        getattr(out, s).restype = None if s.endswith("destroy") else C.c_int
    return out


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Args:
    """Valid arguments of every entry (one feature, one box, one candidate, one view of one id) and sentinel-filled outputs.  `store` stands for a store: memory
    the library must not look at before it has judged the pointers."""

    def __init__(self):
        self.store = np.zeros(4096, np.uint8)
        self.i64 = {k: np.array(v, np.int64) for k, v in dict(owner=[0], cand_owner=[0], box_owner=[0], frm=[1], into=[0]).items()}
        self.u64 = {k: np.array(v, np.uint64) for k, v in dict(frame=[3], camera=[0], feat_ptr=[0, 1], view_feat=[5], feat_id=[5]).items()}
        self.f64 = dict(feat_pixel=np.array([[10.0, 10.0]]), box_corners=np.array([[0.0, 20.0, 0.0, 20.0]]), params=np.array([0.0, 2.0]))
        self.i32 = dict(box_label=np.array([1], np.int32), cand_label=np.array([1], np.int32))
        self.out = dict(owner_out=np.full(1, -77, np.int64), in_box=np.full((1, 1), SENTINEL, np.uint8), feats_in_box=np.full(1, SENTINEL, np.uint32),
                        overlap=np.full((1, 1), SENTINEL, np.uint32), is_match=np.full((1, 1), SENTINEL, np.uint8), score=np.full((1, 1), float(SENTINEL)),
                        dropped=np.full(1, -77, np.int64), n_views=np.full(1, -77, np.int64), n_ids=np.full(1, -77, np.int64), v_frame=np.full(1, SENTINEL, np.uint64),
                        v_camera=np.full(1, SENTINEL, np.uint64), v_feat_ptr=np.full(2, SENTINEL, np.uint64), v_feat=np.full(1, SENTINEL, np.uint64),
                        stats=np.full(9, -77, np.int64), created=np.full(1, SENTINEL, np.uint64))
        self.a = dict(store=self.store)
        for d in (self.i64, self.u64, self.f64, self.i32, self.out):
            self.a.update(d)

    def untouched(self):
        return all((v == (-77 if v.dtype == np.int64 else SENTINEL)).all() for v in self.out.values()) and not self.store.any()

    def call(self, name, handle=None):
        a, L, one = self.a, lib(), C.c_int64(1)
        g = lambda k: p(a[k])  # noqa: E731
        if name == "create":
            return L.obvi_bbox_store_create(handle, None, g("created"))
        if name == "new_owners":
            return L.obvi_bbox_store_new_owners(g("store"), one, g("owner_out"))
        if name == "put_views":
            return L.obvi_bbox_store_put_views(g("store"), one, g("owner"), g("frame"), g("camera"), g("feat_ptr"), g("view_feat"))
        if name == "associate":
            return L.obvi_bbox_store_associate(g("store"), one, g("feat_id"), g("feat_pixel"), one, g("box_corners"), g("box_label"), one, g("cand_owner"), g("cand_label"),
                                               g("params"), g("in_box"), g("feats_in_box"), g("overlap"), g("is_match"), g("score"))
        if name == "commit":
            return L.obvi_bbox_store_commit(g("store"), C.c_uint64(3), C.c_uint64(0), one, g("box_owner"))
        if name == "merge":
            return L.obvi_bbox_store_merge(g("store"), one, g("frm"), g("into"))
        if name == "release":
            return L.obvi_bbox_store_release(g("store"), one, g("owner"))
        if name == "apply_window":
            return L.obvi_bbox_store_apply_window(g("store"), C.c_uint64(9), C.c_uint64(2), g("dropped"))
        if name == "compact":
            return L.obvi_bbox_store_compact(g("store"))
        if name == "views":
            return L.obvi_bbox_store_views(g("store"), C.c_int64(0), g("n_views"), g("n_ids"), g("v_frame"), g("v_camera"), g("v_feat_ptr"), g("v_feat"))
        if name == "get_stats":
            return L.obvi_bbox_store_get_stats(g("store"), g("stats"))
        raise KeyError(name)


ENTRIES = ["new_owners", "put_views", "associate", "commit", "merge", "release", "apply_window", "compact", "views", "get_stats"]
REQUIRED = {"new_owners": ["owner_out"], "put_views": ["owner", "frame", "camera", "feat_ptr", "view_feat"],
            "associate": ["feat_id", "feat_pixel", "box_corners", "box_label", "cand_owner", "cand_label", "params"], "commit": ["box_owner"], "merge": ["frm", "into"],
            "release": ["owner"], "get_stats": ["stats"]}


def test_every_entry_refuses_a_null_store_and_leaves_its_outputs_untouched():
    for name in ENTRIES:
        c = Args()
        c.a["store"] = None
        assert c.call(name) == INVALID and c.untouched(), name


def test_every_entry_refuses_a_null_required_pointer_before_it_looks_at_the_store():
    """The store argument points at zeroed memory that is no store: an entry that looked at it before judging the pointers would follow a NULL handle."""
    for name, pointers in REQUIRED.items():
        for k in pointers:
            c = Args()
            c.a[k] = None
            assert c.call(name) == INVALID and c.untouched(), (name, k)


def test_create_refuses_null_arguments_and_destroy_takes_null():
    c = Args()
    assert c.call("create", handle=None) == INVALID and c.untouched()
    fake_handle = np.zeros(64, np.uint8)
    L = lib()
    assert L.obvi_bbox_store_create(p(fake_handle), None, None) == INVALID and not fake_handle.any()
    L.obvi_bbox_store_destroy(None)


# ---- the model is itself held ---------------------------------------------------------------------------------------------------------------------------------
def test_the_model_on_a_hand_computed_sequence():
    """A pool of 4 ids, compaction from 1 dead id on.
         put 3 ids and 2 ids          5 > 4: one growth to 8                          live 5
         replace the 3 by 4 ids       5 + 4 = 9 > 8: one growth to 16                 live 6, dead 3: 3 <= 6, no compaction
         release the owner of 4       live 2, dead 7: compaction                      live 2, dead 0, capacity still 16"""
    m = store_cases.Model(4, 1)
    a, b = m.new_owners(2)
    m.put_views([a, b], [7, 7], [0, 0], [[1, 2, 3], [4, 5]])
    assert m.stats() == dict(owners=2, views=2, live_ids=5, dead_ids=0, pool_capacity_ids=8, pool_growths=1, compactions=0, replaced_views=0)
    m.put_views([a], [7], [0], [[1, 2, 3, 9]])
    assert m.stats() == dict(owners=2, views=2, live_ids=6, dead_ids=3, pool_capacity_ids=16, pool_growths=2, compactions=0, replaced_views=1)
    m.release([a])
    assert m.stats() == dict(owners=1, views=1, live_ids=2, dead_ids=0, pool_capacity_ids=16, pool_growths=2, compactions=1, replaced_views=1)
    c, = m.new_owners(1)
    assert c == 2                                                                    # tokens are not reused
    m.put_views([c, c], [9, 7], [1, 0], [[8], [6, 7]])
    m.merge([c], [b])                                                                # from wins on (7, 0); (9, 1) joins in key order
    assert m.views(b) == [((7, 0), [6, 7]), ((9, 1), [8])] and c not in m.owners
    assert m.stats()["views"] == 2 and m.stats()["live_ids"] == 3 and m.stats()["replaced_views"] == 1
    # the window in uint64_t: 7 + 2 == 9 stays, 7 + 1 < 9 goes; a window of 2^64 - 2^31 wraps every frame from 2^31 on to a small sum
    assert m.apply_window(9, 2) == 0 and m.apply_window(9, 1) == 1
    wrap = (1 << 64) - (1 << 31)
    assert ((7 + wrap) & store_cases.MASK) > 9 and m.apply_window(9, wrap) == 0      # below 2^31 the sum does not wrap: nothing is stale
    assert store_cases.upload_bytes(10, 2, 3, 7) == 320 + 72 + 12 + 32 + 112 and store_cases.upload_bytes(10, 0, 3, 7) == 0


def test_the_session_of_the_gpu_test_shows_what_it_is_there_for():
    facts = store_cases.session_facts(store_cases.session())
    assert facts["growths"] >= 2 and facts["compactions"] >= 2 and facts["compacted_before_associate"], facts
    assert facts["replaced"] >= 1 and facts["empty_view"] and facts["apart"], facts
    assert facts["rounds"] == store_cases.SESSION_ROUNDS and facts["kinds"] == ["associate", "commit", "merge", "new_owners", "release", "window"]
    assert facts["matches"] >= 40, facts
