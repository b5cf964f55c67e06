"""GPU (-m gpu): covariance blocks of a CONCURRENT joint solve -- sessions over one object map, one handle each behind one group (tests/test_gpu_session_groups.py) --
through the collective obvi_cov_compute / obvi_ba_object_covariances (include/obvi_cov.h).

The yardstick is never the product: it is the CPU oracle on synth.join_problems(sessions), linearised at the members' own solution -- oracle_ba_object_covariances for
object pairs, numpy's inverse of the oracle's joint reduced system for poses and cross blocks, the feature formula on the oracle's joint linearisation for features:
the routes of tests/test_gpu_covariance_blocks.py.  Bar: that file's 1e-7 of a block's largest entry for a reduced system of several dissection levels and about
1500 rows (260 frames there; 4 x 60 frames and the shared tail, 1437 rows, here) -- its 1e-8 is for the 12-pose window."""
import numpy as np
import pytest
import torch

import dist_util
import helpers
import obvi_ba
import synth
import test_gpu_covariance_blocks as blocks
import test_gpu_session_groups as groups

pytestmark = pytest.mark.gpu

POSE, OBJ = blocks.POSE, blocks.OBJ
BAR = 1e-7
SESSIONS = dict(groups.SESSIONS, const_poses=1)      # the first pose of every session constant: a well-posed joint problem
GROUP_TIMEOUT = 60.0                                  # seconds a member waits for the others in a collective before it fails (never a hang)


@pytest.fixture(scope="module")
def sessions():
    return synth.make_sessions(**SESSIONS)


def open_job(sessions, od=7, deterministic=False):
    group = dist_util.RcclGroup(len(sessions))
    group.set_timeout(GROUP_TIMEOUT)
    handles = []
    for m, q in enumerate(sessions):
        ba = helpers.product_ba(object_block_size=od, deterministic=deterministic)
        synth.upload(ba, q)
        group.attach(m, ba, np.ones(len(q["objects"]), np.uint8))
        handles.append(ba)
    return group, handles


def close_job(group, handles):
    for ba in handles:
        ba.close()
    group.close()


def collective(handles, call, timeout_s=300.0):
    """call(member, handle) on every member, one thread each; the results, or the first member's exception"""
    res = dist_util.run_members([lambda m=m, h=h: call(m, h) for m, h in enumerate(handles)], timeout_s)
    for r in res:
        if isinstance(r, Exception):
            raise r
    return res


def statuses(handles, call, timeout_s=300.0):
    """the status code per member (0: no error) of a collective call that may fail"""
    res = dist_util.run_members([lambda m=m, h=h: call(m, h) for m, h in enumerate(handles)], timeout_s)
    out = []
    for r in res:
        if isinstance(r, obvi_ba.ObviError):
            out.append(int(str(r).split("status ")[1].split()[0].rstrip(":,.")))
        elif isinstance(r, Exception):
            raise r
        else:
            out.append(0)
    return out


class Yardstick:
    """The oracle on the joint problem at the members' state: Sigma = inv(S_joint), the object blocks by oracle_ba_object_covariances."""

    def __init__(self, sessions, states, od=7, priors=None):
        self.od = od
        joint = synth.join_problems(sessions)
        joint.update(poses=np.concatenate([s[0] for s in states]), points=np.concatenate([s[1] for s in states]), objects=states[0][2])
        self.joint, self.po, self.lo = joint, joint["session_pose_offsets"], joint["session_point_offsets"]
        self.o = o = helpers.oracle_ba(object_block_size=od)
        synth.upload(o, joint)
        if priors is not None:
            o.set_parameter_priors(*priors)
        self.pvar, self.lvar, self.ovar = blocks.parameters(o)
        self.prow, self.orow = blocks.canonical(self.pvar, self.ovar, od)
        self.ids = np.arange(len(joint["objects"]))
        self.obj = o.object_covariances(self.ids)              # (checked on the CPU: succeeds on this joint problem, smallest eigenvalue 1e-3)

    def sigma(self):
        S, _ = self.o.debug_reduced_system(1e300)
        assert S.shape[0] == 6 * self.pvar.sum() + self.od * self.ovar.sum()
        self.cond = float(np.linalg.cond(S))
        self.Sigma = np.linalg.inv(S)
        return self.Sigma


def member_states(handles):
    return [(h.get_poses(), h.get_points(), h.get_objects()) for h in handles]


def solve_job(handles, max_it=15):
    out = collective(handles, lambda m, h: h.solve(helpers.ba_params(max_it=max_it)))
    assert len({o.num_iterations for o in out}) == 1 and all(o.is_solution_usable for o in out)
    return out


def check_every_block_of_the_job(sessions, od, deterministic=False):
    if od == 9:
        sessions = [synth.nine_dof(q) for q in sessions]
    group, handles = open_job(sessions, od, deterministic)
    try:
        solve_job(handles)
        before = group.stats()[0]
        collective(handles, lambda m, h: h.covariance_compute())
        assert group.stats()[0] - before == 4            # tail order, shared blocks, shared tail, scalars: the sequence include/obvi_cov.h states
        y = Yardstick(sessions, member_states(handles), od)
        Sigma = y.sigma()
        shared = [h.object_covariance_blocks(y.ids) for h in handles]
        assert shared[0].shape == (len(y.ids), od, od)
        worst_obj = max(blocks.block_err(c[i], y.obj[i]) for c in shared for i in y.ids)
        across = max(float(np.abs(c - shared[0]).max() / np.abs(shared[0]).max()) for c in shared)
        print("od %d: shared object blocks against the oracle's joint blocks %.3e (bar %.0e), across members %.3e, cond(S_joint) %.2e" % (od, worst_obj, BAR, across, y.cond))
        assert worst_obj < BAR
        # every member factorises the same summed tail: equal to round-off (bitwise on deterministic handles, tested below)
        assert across < 1e-12
        rng = np.random.default_rng(20250101)
        samples = [rng.choice(len(q["points"]), size=40, replace=False) for q in sessions]
        want_pts = blocks.point_blocks_from_the_oracle(y.o, y.joint, Sigma, y.prow, y.lvar, np.concatenate([y.lo[s] + samples[s] for s in range(len(sessions))]))
        for s, (q, g) in enumerate(zip(sessions, handles)):
            P = len(q["poses"])
            prow = y.prow[y.po[s]:y.po[s + 1]]
            cp = g.pose_covariances(np.arange(P))
            worst = 0.0
            for p in range(P):
                if prow[p] < 0:
                    assert np.all(cp[p] == 0.0)
                else:
                    worst = max(worst, blocks.block_err(cp[p], Sigma[prow[p]:prow[p] + 6, prow[p]:prow[p] + 6]))
            got = g.point_covariances(samples[s])
            worst_pt = 0.0
            for x, l in zip(got, samples[s]):
                if y.lvar[y.lo[s] + l]:
                    worst_pt = max(worst_pt, blocks.block_err(x, want_pts[y.lo[s] + l]))
                else:
                    assert np.all(x == 0.0)
            print("od %d member %d: pose blocks %.3e, %d feature blocks %.3e (bar %.0e)" % (od, s, worst, len(got), worst_pt, BAR))
            assert worst < BAR and worst_pt < BAR
            rows = {(POSE, p): int(prow[p]) for p in range(P) if prow[p] >= 0}
            rows.update({(OBJ, int(i)): int(y.orow[i]) for i in y.ids})
            dims = {k: (6 if k[0] == POSE else od) for k in rows}
            pairs = [pr for pr in blocks.joined_pairs(q, prow >= 0, y.ovar) if pr[1][0] == OBJ]          # pose x shared object, joined by a bounding-box factor
            pairs += [((OBJ, int(a)), (OBJ, int(b))) for a in y.ids for b in y.ids if a < b]             # shared x shared
            assert len(pairs) > 100
            ka, ia, kb, ib = zip(*[(a[0], a[1], b[0], b[1]) for a, b in pairs])
            assert g.covariance_on_pattern(ka, ia, kb, ib).all()
            blocks.check_cross(g, pairs, rows, dims, Sigma, BAR, "od %d member %d" % (od, s))
    finally:
        close_job(group, handles)


def test_four_sessions_on_one_rank_every_block_against_the_oracles_joint_problem(sessions):
    """Four sessions behind the compiled group, a joint solve, ONE collective obvi_cov_compute (four collectives): every shared object's block on every member is the
    oracle's joint block and the same on every member; every member's pose blocks, 40 sampled feature blocks and its pose x shared-object and shared x shared
    cross blocks are those of the joint inverse.  Without the collective pass the call is refused with OBVI_ERR_INVALID_ARGUMENT."""
    check_every_block_of_the_job(sessions, 7)


def test_nine_parameter_blocks(sessions):
    """The same with object_block_size = 9: the shared blocks are 9 x 9.  On deterministic handles: the upright 9-parameter objects leave cond(S_joint) between 4e11 and
    7e12 depending on where the fifteen LM steps of a default handle end (measured on two runs: shared x shared cross blocks 1.3e-9 and 1.5e-8 of their largest entry,
    everything else below 3e-10), so the estimate the blocks are taken at is pinned to reproducible bits; the bar is the same."""
    check_every_block_of_the_job(sessions, 9, deterministic=True)


def test_the_merged_route_is_collective_too(sessions):
    """obvi_ba_object_covariances on every member (own blocks and every cross pair of the shared objects; one member asks for nothing and still takes part):
    against the oracle's joint blocks, and against obvi_cov_object_blocks / obvi_cov_cross_blocks at that route's bars."""
    group, handles = open_job(sessions)
    try:
        solve_job(handles)
        y = Yardstick(sessions, member_states(handles))
        a, b = np.array([(i, j) for i in y.ids for j in y.ids if i != j]).T
        before = group.stats()[0]
        own = collective(handles, lambda m, h: h.object_covariances(y.ids if m != 1 else []))
        assert group.stats()[0] - before == 4 and own[1].shape[0] == 0
        cross = collective(handles, lambda m, h: h.object_covariances(a, b))
        want = y.o.object_covariances(a, b)
        scale = float(np.abs(y.obj).max())
        collective(handles, lambda m, h: h.covariance_compute())
        for m, h in enumerate(handles):
            e_own = max(blocks.block_err(own[m][i], y.obj[i]) for i in y.ids) if m != 1 else 0.0
            e_x = float(np.abs(cross[m] - want).max()) / scale
            sel = h.object_covariance_blocks(y.ids)
            selx = np.stack(h.cross_covariances(np.full(len(a), OBJ), a, np.full(len(a), OBJ), b))
            e_sel = max(blocks.block_err(sel[i], own[m][i]) for i in y.ids) if m != 1 else 0.0
            e_selx = float(np.abs(selx - cross[m]).max()) / scale
            print("member %d: merged route against the oracle: own %.3e cross %.3e; selected inversion against the merged route: own %.3e cross %.3e (bars %.0e)" % (m, e_own, e_x, e_sel, e_selx, BAR))
            assert max(e_own, e_x, e_sel, e_selx) < BAR
    finally:
        close_job(group, handles)


def test_one_handle_holding_the_joint_problem_with_everything_shared(sessions):
    """The joint problem on ONE handle, every object marked shared, an identity hook: the tail path (tail-order proof, pack, exchange, unpack, tail levels) changes
    the elimination order and nothing else.  Two elimination orders of one matrix: each is held to 1e-7 of the exact block at this size, and so is their difference."""
    joint = synth.join_problems(sessions)
    P, O = len(joint["poses"]), len(joint["objects"])
    out = []
    for shared in (False, True):
        g = helpers.product_ba(); synth.upload(g, joint)
        if shared:
            g.set_shared_objects(np.ones(O, np.uint8), 0, 1)
            g.set_allreduce(lambda ptr, n, op, stream: 0)
        g.covariance_compute()
        pr = blocks.joined_pairs(joint, ~joint["pose_const"].astype(bool), np.ones(O, bool))
        pr = [x for x in pr if x[1][0] == OBJ]
        ka, ia, kb, ib = zip(*[(x[0][0], x[0][1], x[1][0], x[1][1]) for x in pr])
        assert g.covariance_on_pattern(ka, ia, kb, ib).all()
        out.append((g.pose_covariances(np.arange(P)), g.object_covariance_blocks(np.arange(O)), g.point_covariances(np.arange(0, len(joint["points"]), 7)),
                    np.stack(g.cross_covariances(ka, ia, kb, ib)), g.object_covariances(np.arange(O))))
        g.close()
    worst = 0.0
    for x, w in zip(out[1], out[0]):
        live = [i for i in range(len(w)) if np.any(w[i] != 0.0)]
        assert all(np.all(x[i] == 0.0) for i in range(len(w)) if i not in live)
        worst = max(worst, max(blocks.block_err(x[i], w[i]) for i in live))
    print("everything shared on one handle against the plain handle: %.3e" % worst)
    assert worst < BAR


def test_the_joint_marginal_is_not_the_local_one(sessions):
    """Every shared object is seen by all four sessions: its joint block is below (Loewner) and strictly smaller in trace than the block an unshared handle gets
    from one session alone at the same estimate.  A pass that skipped the exchange would return the local block."""
    group, handles = open_job(sessions)
    try:
        solve_job(handles)
        collective(handles, lambda m, h: h.covariance_compute())
        states = member_states(handles)
        joint_blocks = handles[0].object_covariance_blocks(np.arange(3))
        for s, q in enumerate(sessions):
            alone = dict(q); alone.update(poses=states[s][0], points=states[s][1], objects=states[s][2])
            g = helpers.product_ba(); synth.upload(g, alone)
            g.covariance_compute()
            local = g.object_covariance_blocks(np.arange(3))
            g.close()
            for i in range(3):
                scale = float(np.abs(local[i]).max())
                lo = float(np.linalg.eigvalsh(local[i] - joint_blocks[i]).min())
                print("session %d object %d: smallest eigenvalue of local - joint %.3e (scale %.3e), trace %.4e -> %.4e" % (s, i, lo, scale, np.trace(local[i]), np.trace(joint_blocks[i])))
                assert lo >= -1e-9 * scale and np.trace(joint_blocks[i]) < np.trace(local[i])
    finally:
        close_job(group, handles)


def test_priors_on_a_shared_object_and_symmetric_failure(sessions):
    """A parameter prior on a shared object follows the rule for object-only factors: exactly ONE member uploads it (any member) and the joint block changes as the
    oracle says; uploaded by two members it is counted twice -- the documented rule, as two Jacobian rows in the oracle.  ONE member whose session floats freely (no constant pose,
    no sighting of the map) makes the joint problem rank deficient: every member returns OBVI_ERR_NUMERICAL from the same call, within the group's time-out, and the
    group serves the next valid pass."""
    group, handles = open_job(sessions)
    try:
        solve_job(handles)
        states = member_states(handles)
        ids = np.arange(3)
        prior = ([2, 2], [1, 1], [0, 4], [0.0, 0.0], [0.05, 0.02])           # object 1: x and the first extent
        handles[2].set_parameter_priors(*prior)
        collective(handles, lambda m, h: h.covariance_compute())
        once = Yardstick(sessions, states, priors=prior).obj
        plain = Yardstick(sessions, states).obj
        assert blocks.block_err(once[1], plain[1]) > 1e-4                      # (the prior matters)
        for h in handles:
            e = max(blocks.block_err(h.object_covariance_blocks(ids)[i], once[i]) for i in ids)
            print("prior uploaded by member 2: %.3e (bar %.0e)" % (e, BAR))
            assert e < BAR
        merged = collective(handles, lambda m, h: h.object_covariances(ids))
        assert max(blocks.block_err(c[i], once[i]) for c in merged for i in ids) < BAR
        handles[1].set_parameter_priors(*prior)
        collective(handles, lambda m, h: h.covariance_compute())
        twice = Yardstick(sessions, states, priors=tuple(list(p) * 2 for p in prior)).obj
        assert blocks.block_err(twice[1], once[1]) > 1e-4
        for h in handles:
            e = max(blocks.block_err(h.object_covariance_blocks(ids)[i], twice[i]) for i in ids)
            print("the same prior uploaded by members 1 and 2: counted twice, %.3e" % e)
            assert e < BAR
        for h in handles:
            h.set_parameter_priors([], [], [], [], [])
        # member 3 alone: no constant pose and no sighting of the map -- its session floats freely (a gauge of six), the joint problem is rank deficient
        q = sessions[3]
        handles[3].set_const_flags(pose_const=np.zeros(len(q["poses"]), np.uint8))
        handles[3].set_active_mask(2, np.zeros(len(q["bb_obj"]), np.uint8))
        assert statuses(handles, lambda m, h: h.covariance_compute(), timeout_s=GROUP_TIMEOUT + 30) == [-6] * 4
        assert statuses(handles, lambda m, h: h.object_covariances(ids), timeout_s=GROUP_TIMEOUT + 30) == [-6] * 4
        with pytest.raises(obvi_ba.ObviError, match="status -5"):
            handles[0].object_covariance_blocks(ids)
        # the group is usable: the next valid pass gives the joint blocks again
        handles[3].set_const_flags(pose_const=q["pose_const"])
        handles[3].set_active_mask(2, np.ones(len(q["bb_obj"]), np.uint8))
        collective(handles, lambda m, h: h.covariance_compute())
        assert max(blocks.block_err(handles[0].object_covariance_blocks(ids)[i], plain[i]) for i in ids) < BAR
    finally:
        close_job(group, handles)


def test_two_collective_passes_on_deterministic_handles_are_bit_identical(sessions):
    """Per member: two passes over the same state give the same bits.  Across members: the group sums in member order and every member factorises and inverts the
    same summed tail with the same kernels, so the shared blocks carry the same bits on every member."""
    group, handles = open_job(sessions, deterministic=True)
    try:
        solve_job(handles, max_it=4)
        runs = []
        for _ in range(2):
            collective(handles, lambda m, h: h.covariance_compute())
            runs.append([(h.pose_covariances(np.arange(len(q["poses"]))), h.point_covariances(np.arange(0, len(q["points"]), 5)), h.object_covariance_blocks(np.arange(3)),
                          np.concatenate([x.ravel() for x in h.cross_covariances([OBJ, OBJ, POSE], [0, 1, 5], [OBJ, OBJ, POSE], [1, 2, 6])]))
                         for h, q in zip(handles, sessions)])
        for m in range(len(handles)):
            for a, b in zip(runs[0][m], runs[1][m]):
                assert np.array_equal(a, b) and np.any(a != 0.0)
        diff = max(float(np.abs(runs[0][m][2] - runs[0][0][2]).max()) for m in range(len(handles)))
        print("shared blocks across deterministic members: largest difference %.3e" % diff)
        for m in range(1, len(handles)):
            assert np.array_equal(runs[0][m][2], runs[0][0][2])
    finally:
        close_job(group, handles)


def _cov_worker(rank, world, port, sessions, out):
    import os
    import sys
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    sys.path.insert(0, os.path.join(helpers.ROOT, "obvi-slam_amd", "python")); sys.path.insert(0, os.path.join(helpers.ROOT, "tests"))
    import torch.distributed as dist
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    k = len(sessions) // world
    log = dist_util.IssueLog()
    group = dist_util.RcclGroup(k, inner=dist_util.staged_allreduce(dist, log), rank=rank, world=world, device=0)
    group.set_timeout(GROUP_TIMEOUT)
    handles = []
    for m in range(k):
        q = sessions[rank * k + m]
        ba = helpers.product_ba()
        synth.upload(ba, q)
        group.attach(m, ba, np.ones(len(q["objects"]), np.uint8))
        handles.append(ba)
    solve_job(handles)
    calls0 = log.calls
    collective(handles, lambda m, h: h.covariance_compute())
    per_pass = log.calls - calls0
    same = dist_util.same_issue_order(dist, log.calls, log.digest())
    out[rank] = dict(same=same, per_pass=per_pass, states=member_states(handles), shared=[h.object_covariance_blocks(np.arange(3)) for h in handles],
                     pose=[h.pose_covariances(np.arange(len(sessions[rank * k + m]["poses"]))) for m, h in enumerate(handles)])
    close_job(group, handles)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_of_two_handles(sessions):
    """Two processes over gloo on one GPU, two handles each behind the group: one inter-rank collective per group collective (four per pass), the same issue order
    on both ranks, and every handle's shared blocks and pose blocks are the joint yardstick's."""
    import socket
    import torch.multiprocessing as mp
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    mgr = mp.Manager(); out = mgr.dict()
    mp.spawn(_cov_worker, args=(2, port, sessions, out), nprocs=2, join=True)
    assert set(out.keys()) == {0, 1}
    states = out[0]["states"] + out[1]["states"]
    y = Yardstick(sessions, states)
    Sigma = y.sigma()
    for rank in (0, 1):
        o = out[rank]
        assert o["same"] and o["per_pass"] == 4
        for m in range(2):
            s = 2 * rank + m
            e = max(blocks.block_err(o["shared"][m][i], y.obj[i]) for i in y.ids)
            prow = y.prow[y.po[s]:y.po[s + 1]]
            ep = max(blocks.block_err(o["pose"][m][p], Sigma[prow[p]:prow[p] + 6, prow[p]:prow[p] + 6]) for p in range(len(prow)) if prow[p] >= 0)
            print("rank %d handle %d: shared blocks %.3e, pose blocks %.3e (bar %.0e)" % (rank, m, e, ep, BAR))
            assert e < BAR and ep < BAR


def test_the_joint_map_feeds_the_next_session(sessions):
    """Closing the loop of the concurrent mode: four concurrent sessions, the joint map through dist_util.joint_long_term_map, a following session that starts from it
    as long-term-map priors -- against the same chain on the oracle (joint solve, oracle covariances, next session), at the bars of
    test_multi_session_chain_through_the_long_term_map; and the map makes the next session more certain about every object it holds."""
    prm = helpers.ba_params(max_it=30)
    ids = np.arange(3, dtype=np.uint32)
    following = synth.make_problem(P=60, L=900, O=3, seed=777, object_seed=33, min_obj_obs=6, object_classes=("bench",), bbox_noise=5.0)
    assert np.array_equal(following["objects"], sessions[0]["objects"])

    def next_session(make, mean, cov):
        s2 = dict(following)
        s2.update(lt_obj=ids, lt_mean=mean, lt_cov=cov.reshape(-1, 49), lt_huber=1.0)
        ba2 = make(); synth.upload(ba2, s2)
        s = ba2.solve(prm)
        assert s.is_solution_usable
        cov2 = ba2.object_covariances(ids)
        bare = {k: v for k, v in s2.items() if not k.startswith("lt_")}
        bare.update(poses=ba2.get_poses(), points=ba2.get_points(), objects=ba2.get_objects())
        free = make(); synth.upload(free, bare)
        cov_free = free.object_covariances(ids)
        for o in ids:
            assert np.all(np.diag(cov2[o]) <= np.diag(cov_free[o]) * (1 + 1e-6))
        return ba2.get_objects(), cov2, s.final_cost

    orc = helpers.oracle_ba(); synth.upload(orc, synth.join_problems(sessions))
    assert orc.solve(prm).is_solution_usable
    m1o, c1o = orc.get_objects(), orc.object_covariances(ids)
    m2o, c2o, fo = next_session(helpers.oracle_ba, m1o, c1o)
    group, handles = open_job(sessions)
    try:
        out = collective(handles, lambda m, h: h.solve(prm))
        assert all(o.is_solution_usable for o in out)
        ltm = dist_util.joint_long_term_map(handles, ids, cross_pairs=[(0, 1), (1, 2)])
        assert set(ltm["cross"]) == {(0, 1), (1, 2)} and ltm["cross"][(0, 1)].shape == (7, 7)
    finally:
        close_job(group, handles)
    m1g, c1g = ltm["mean"], ltm["cov"]
    m2g, c2g, fg = next_session(helpers.product_ba, m1g, c1g)
    close = lambda cg, co, tol: bool(np.all(np.abs(cg - co) <= tol * np.abs(co).max(axis=(1, 2), keepdims=True)))      # noqa: E731
    print("map: mean %.3e, cov %.3e; next session: cost %.3e, mean %.3e, cov %.3e" % (np.abs(m1g - m1o).max(), np.abs(c1g - c1o).max() / np.abs(c1o).max(), abs(fg - fo) / fo,
                                                                                      np.abs(m2g - m2o).max(), np.abs(c2g - c2o).max() / np.abs(c2o).max()))
    assert np.abs(m1g - m1o).max() < 1e-6 and close(c1g, c1o, 1e-5)
    assert abs(fg - fo) <= 1e-6 * fo and np.abs(m2g - m2o).max() < 1e-5 and close(c2g, c2o, 1e-4)
