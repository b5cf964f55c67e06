"""GPU (-m gpu): independent windows that share object blocks.  One GPU is enough to check the algebra: two
handles are driven from two threads and the all-reduce hook is emulated by summing their exchange buffers; the result
must equal one handle solving the joint problem."""
import threading

import numpy as np
import pytest
import torch

import dist_util
import helpers
import obvi_ba
import synth

pytestmark = pytest.mark.gpu


split_problem = helpers.split_problem


def check_collectives(log, n_shared, world):
    """The protocol of include/obvi_ba.h: once per solve the fixed cost + the hash of the shared tail's order (2 doubles); per LM submission three sums -- the shared objects' blocks
    (56 per object), the shared tail of the reduced system (skipped by a linearisation-only submission), the scalar block + one
    gradient-maximum slot per rank -- and nothing else (no max-reduction, no fourth collective)."""
    assert all(op == 0 for _, op in log)
    blocks = sum(1 for n, _ in log if n == 56 * n_shared)
    scalars = sum(1 for n, _ in log if n == 9 + world)
    fixed = sum(1 for n, _ in log if n == 2)
    tails = len(log) - blocks - scalars - fixed
    assert blocks == scalars >= 1 and fixed == 1 and tails in (blocks, blocks - 1), (blocks, scalars, fixed, tails)
    return blocks


class EmulatedAllReduce:
    """Stands in for RCCL: sums / maximises the exchange buffers of `world` handles living on one GPU."""
    def __init__(self, world):
        self.world, self.bar, self.slots, self.res, self.calls, self.log = world, threading.Barrier(world), [None] * world, None, 0, []
        self.issue = [dist_util.IssueLog() for _ in range(world)]      # per rank: (count, op, stream ordinal) in host issue order

    def hook(self, rank):
        def fn(ptr, count, op, stream):
            self.issue[rank].note(count, op, stream)
            torch.cuda.synchronize()
            t = dist_util.device_tensor(ptr, count)
            self.slots[rank] = t
            self.bar.wait()
            if rank == 0:
                st = torch.stack(self.slots)
                self.res = st.max(0).values if op else st.sum(0)
                self.calls += 1
                self.log.append((int(count), int(op)))
            self.bar.wait()
            t.copy_(self.res)
            torch.cuda.synchronize()
            self.bar.wait()
            return 0
        return fn


@pytest.fixture(scope="module")
def scene():
    prob = synth.make_problem(P=60, L=900, O=3, seed=33, min_obj_obs=6, object_classes=("bench",), bbox_noise=5.0)
    return prob


def test_single_rank_identity_hook(scene):
    """world = 1: shared objects are merely ordered last and the three exchanges are identities -> same solve."""
    a, b = helpers.product_ba(), helpers.product_ba()
    for ba in (a, b):
        synth.upload(ba, scene)
    calls = []
    b.set_shared_objects(np.ones(len(scene["objects"]), np.uint8), 0, 1)
    b.set_allreduce(lambda ptr, n, op, stream: calls.append((n, op)) or 0)
    prm = helpers.ba_params(max_it=12)
    sa, sb = a.solve(prm), b.solve(prm)
    assert calls and sb.num_iterations == sa.num_iterations
    assert abs(sb.final_cost - sa.final_cost) <= 1e-9 * sa.final_cost
    assert np.abs(b.get_poses() - a.get_poses()).max() < 1e-9 and np.abs(b.get_objects() - a.get_objects()).max() < 1e-8
    # per LM submission three collectives, all sums: shared blocks (56 per object), tail, scalar block + one gradient-maximum slot per rank
    assert check_collectives(calls, len(scene["objects"]), 1) >= sb.num_iterations - 1


def run_windows(wins, prm, hooks):
    """One handle per window on this GPU, one host thread per handle, `hooks[rank]` as its all-reduce callback."""
    handles, out = [], [None] * len(wins)
    for rank, (q, pts, rng) in enumerate(wins):
        ba = helpers.product_ba()
        synth.upload(ba, q)
        ba.set_shared_objects(np.ones(len(q["objects"]), np.uint8), rank, len(wins))
        ba.set_allreduce(hooks[rank])
        handles.append(ba)

    def run(rank):
        out[rank] = handles[rank].solve(prm)
    th = [threading.Thread(target=run, args=(r,)) for r in range(len(wins))]
    [t.start() for t in th]; [t.join(timeout=600) for t in th]
    return handles, out


def test_two_windows_sharing_objects_equal_the_oracles_joint_solve(scene):
    """parity for the shared-object split is against the CPU ORACLE solving the same joint problem on one device
    (the product's own joint solve is kept as a second check)."""
    wins, joint, keep_pts = split_problem(scene, 30)
    prm = helpers.ba_params(max_it=15)
    orc = helpers.oracle_ba()
    synth.upload(orc, joint)
    sorc = orc.solve(prm)
    ref = helpers.product_ba()
    synth.upload(ref, joint)
    sref = ref.solve(prm)
    assert sref.num_iterations == sorc.num_iterations and abs(sref.final_cost - sorc.final_cost) <= 1e-8 * sorc.final_cost
    emu = EmulatedAllReduce(2)
    handles, out = run_windows(wins, prm, [emu.hook(0), emu.hook(1)])
    assert all(o is not None for o in out) and emu.calls > 0
    io = orc.iterations()
    for rank, o in enumerate(out):
        assert o.num_iterations == sorc.num_iterations and o.termination_type == sorc.termination_type
        assert abs(o.initial_cost - sorc.initial_cost) <= 1e-10 * sorc.initial_cost
        assert abs(o.final_cost - sorc.final_cost) <= 1e-8 * sorc.final_cost        # every rank reports the job-wide cost
        ig = handles[rank].iterations()
        assert [i.step_is_successful for i in ig] == [i.step_is_successful for i in io]
        assert max(abs(a.cost - b.cost) / b.cost for a, b in zip(ig, io)) < 1e-8
    jp, jo, jpts = orc.get_poses(), orc.get_objects(), orc.get_points()
    assert np.abs(handles[0].get_poses() - jp[:30]).max() < 1e-8 and np.abs(handles[1].get_poses() - jp[30:]).max() < 1e-8
    assert np.abs(handles[0].get_objects() - jo).max() < 1e-7 and np.abs(handles[1].get_objects() - handles[0].get_objects()).max() == 0.0
    pos = {int(p): i for i, p in enumerate(keep_pts)}
    for rank, (q, pts, rng) in enumerate(wins):
        idx = np.array([pos[int(p)] for p in pts])
        assert np.abs(handles[rank].get_points() - jpts[idx]).max() < 1e-7


def test_ranks_that_upload_the_shared_objects_differently_are_refused(scene):
    """The shared tail is laid out along the shared objects' UPLOADED positions (plan.cpp), the same on every rank because the contract says every rank
    uploads the shared objects with the same values.  A host that breaks the contract -- here: rank 1 starts two objects from each other's place -- would have
    its tail tiles summed against the wrong objects; the hash of the order travels with the fixed cost at the start of the solve and every rank refuses."""
    wins, joint, keep_pts = split_problem(scene, 30)
    q1 = dict(wins[1][0]); q1["objects"] = q1["objects"].copy()
    q1["objects"][[0, 2], :2] = q1["objects"][[2, 0], :2] + 40.0        # far enough apart to change the curve's order
    emu = EmulatedAllReduce(2)
    handles, errs = [], [None, None]
    for rank, q in enumerate((wins[0][0], q1)):
        ba = helpers.product_ba()
        synth.upload(ba, q)
        ba.set_shared_objects(np.ones(len(q["objects"]), np.uint8), rank, 2)
        ba.set_allreduce(emu.hook(rank))
        handles.append(ba)

    def run(rank):
        try:
            handles[rank].solve(helpers.ba_params(max_it=3))
        except obvi_ba.ObviError as e:
            errs[rank] = str(e)
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in th]; [t.join(timeout=120) for t in th]
    assert all(e is not None and "status -1" in e and "order the shared objects differently" in e for e in errs), errs
    assert emu.calls == 1                                               # the solve stopped at its first collective, on both ranks


def test_a_rank_planned_ahead_with_placeholder_objects_orders_the_tail_like_the_others(scene):
    """a handle uploaded with PLACEHOLDER object values and planned ahead (obvi_ba_prepare) used to keep the tail order of the placeholders
    after obvi_ba_update_state had delivered the real values, and was then refused by the order check of the solve.  The values that arrive through
    update_state count as uploaded: the key is refreshed, the plan rebuilt, and the rank solves with the others -- the same joint solution as two
    ranks uploaded normally."""
    wins, joint, keep_pts = split_problem(scene, 30)
    prm = helpers.ba_params(max_it=8)
    emu0 = EmulatedAllReduce(2)
    ref_handles, ref_out = run_windows(wins, prm, [emu0.hook(0), emu0.hook(1)])
    emu = EmulatedAllReduce(2)
    handles, out = [], [None, None]
    for rank, (q, pts, rng) in enumerate(wins):
        ba = helpers.product_ba()
        if rank == 1:
            ph = dict(q); ph["objects"] = np.zeros_like(q["objects"]); ph["objects"][:, 4:] = 1.0; ph["poses"] = np.zeros_like(q["poses"]); ph["points"] = np.ones_like(q["points"])
            synth.upload(ba, ph)
            ba.set_shared_objects(np.ones(len(q["objects"]), np.uint8), rank, 2)
            ba.prepare()
            ba.update_state(q["poses"], q["points"], q["objects"])
        else:
            synth.upload(ba, q)
            ba.set_shared_objects(np.ones(len(q["objects"]), np.uint8), rank, 2)
        ba.set_allreduce(emu.hook(rank))
        handles.append(ba)

    def run(rank):
        out[rank] = handles[rank].solve(prm)
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in th]; [t.join(timeout=300) for t in th]
    assert all(o is not None for o in out)
    for rank in range(2):
        assert out[rank].num_iterations == ref_out[rank].num_iterations
        assert abs(out[rank].final_cost - ref_out[rank].final_cost) <= 1e-9 * ref_out[rank].final_cost
        assert np.abs(handles[rank].get_objects() - ref_handles[rank].get_objects()).max() < 1e-8


def config4_windows(world, P=500, L=50000, O=25):
    """BASELINE configs[3] as bench.py builds it: `world` local-BA windows over the same place (own seed each) sharing one object
    set; object-only factors of a shared object are uploaded by rank 0 only."""
    wins = []
    for rank in range(world):
        q = synth.make_problem(P=P, L=L, O=O, seed=dist_util.rank_seed(20241008, 4, rank), const_poses=5, object_seed=20241008 + 4, min_obj_obs=10)
        if rank != 0:
            for k in ("sp_obj", "sp_mean", "sp_cov"):
                q[k] = q[k][:0]
        wins.append((q, None, None))
    return wins


def test_config4_size_windows_invariants():
    """2 x 500 keyframes / 50 000 features sharing 25 objects (the per-GPU size of BASELINE configs[3]): too large for the oracle,
    so checked through size-independent properties: the job-wide cost both ranks report = the sum of the windows' own costs with
    the shared priors counted once; at a tiny trust-region radius (quadratic model exact) relative_decrease = 1 +- 5e-2, which
    exercises the exchanged diagonal blocks, the summed tail and its factorisation together; identical decisions and identical
    shared objects on both ranks; cost decreases."""
    wins = config4_windows(2)
    assert len(wins[0][0]["objects"]) == 25 and np.array_equal(wins[0][0]["objects"], wins[1][0]["objects"])
    seen = [set(np.unique(w[0]["bb_obj"]).tolist()) for w in wins]
    assert len(seen[0] & seen[1]) >= 20                    # the objects really are observed from both windows
    # cost bookkeeping: every window evaluated alone (rank 1 carries no shape priors)
    own = []
    for q, _, _ in wins:
        ba = helpers.product_ba(); synth.upload(ba, q); own.append(ba.evaluate(True, False)[0]); ba.close()
    emu = EmulatedAllReduce(2)
    tiny = helpers.ba_params(max_it=1, radius=1e-2, max_radius=1e-2, ftol=0, gtol=0, ptol=0)
    handles, out = run_windows(wins, tiny, [emu.hook(0), emu.hook(1)])
    for rank in range(2):
        assert abs(out[rank].initial_cost - (own[0] + own[1])) <= 1e-10 * (own[0] + own[1])
        it = handles[rank].iterations()[1]
        assert it.step_is_valid and it.step_is_successful and abs(it.relative_decrease - 1.0) < 5e-2
    a, b = handles[0].iterations()[1], handles[1].iterations()[1]
    assert a.cost == b.cost and a.relative_decrease == b.relative_decrease and a.step_norm == b.step_norm
    # a real solve from there
    emu2 = EmulatedAllReduce(2)
    for rank, hdl in enumerate(handles):
        hdl.set_allreduce(emu2.hook(rank))
    out2 = [None, None]
    prm = helpers.ba_params(max_it=8, ftol=0, gtol=0, ptol=0)

    def run(rank):
        out2[rank] = handles[rank].solve(prm)
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in th]; [t.join(timeout=600) for t in th]
    assert out2[0].num_iterations == out2[1].num_iterations == 9
    assert out2[0].final_cost == out2[1].final_cost and out2[0].final_cost < 0.5 * out2[0].initial_cost
    assert np.array_equal(handles[0].get_objects(), handles[1].get_objects())
    assert [i.step_is_successful for i in handles[0].iterations()] == [i.step_is_successful for i in handles[1].iterations()]
    for rank, hdl in enumerate(handles):                    # the state handed back is the job-wide minimum-cost iterate
        hdl.set_allreduce(None)
    own_end = [hdl.evaluate(True, False)[0] for hdl in handles]
    assert abs(sum(own_end) - out2[0].final_cost) <= 1e-9 * out2[0].final_cost


def test_config4_eight_windows_on_one_device():
    """BASELINE configs[3] at its stated shape -- EIGHT 500-keyframe / 50 000-feature windows sharing 25 objects -- with the eight ranks' handles on
    this one GPU (eight host threads, the all-reduce emulated by summing their exchange buffers).  World-size-8 bookkeeping: the shape and
    LTM priors of the shared objects enter once (rank 0), the tail and the scalars are sums over eight contributions, three collectives
    per LM step, and all eight ranks take the same decisions and hold the same objects."""
    world = 8
    wins = config4_windows(world)
    seen = [set(np.unique(w[0]["bb_obj"]).tolist()) for w in wins]
    assert len(set.intersection(*seen)) >= 15                                               # objects observed from all eight windows
    own = []
    for q, _, _ in wins:
        ba = helpers.product_ba(); synth.upload(ba, q); own.append(ba.evaluate(True, False)[0]); ba.close()
    assert len(wins[0][0]["sp_obj"]) == 25 and all(len(w[0]["sp_obj"]) == 0 for w in wins[1:])     # object-only factors: rank 0 only
    emu = EmulatedAllReduce(world)
    tiny = helpers.ba_params(max_it=1, radius=1e-2, max_radius=1e-2, ftol=0, gtol=0, ptol=0)
    handles, out = run_windows(wins, tiny, [emu.hook(r) for r in range(world)])
    assert all(o is not None for o in out)
    assert check_collectives(emu.log, 25, world) == 2                                      # two submissions: the step, then the gradient of the accepted point
    total = sum(own)
    recs = [h.iterations()[1] for h in handles]
    for rank in range(world):
        assert abs(out[rank].initial_cost - total) <= 1e-10 * total                          # priors counted once, eight windows summed
        assert recs[rank].step_is_valid and recs[rank].step_is_successful and abs(recs[rank].relative_decrease - 1.0) < 5e-2
        assert (recs[rank].cost, recs[rank].relative_decrease, recs[rank].step_norm, recs[rank].gradient_max_norm) == (recs[0].cost, recs[0].relative_decrease, recs[0].step_norm, recs[0].gradient_max_norm)
    emu2 = EmulatedAllReduce(world)
    for rank, hdl in enumerate(handles):
        hdl.set_allreduce(emu2.hook(rank))
    out2 = [None] * world
    prm = helpers.ba_params(max_it=6, ftol=0, gtol=0, ptol=0)

    def run(rank):
        out2[rank] = handles[rank].solve(prm)
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in th]; [t.join(timeout=900) for t in th]
    assert all(o is not None and o.num_iterations == 7 for o in out2)
    assert check_collectives(emu2.log, 25, world) == 7                                     # three collectives per LM submission, seven submissions
    # ONE communicator is driven from two streams of a handle (shared blocks on the side stream, tail and scalars on the main stream): legal for
    # RCCL only if every rank enqueues the same collectives in the same host order -- the per-rank issue logs must be identical, and the
    # stream pattern is the documented one
    for rank in range(1, world):
        assert emu2.issue[rank].records == emu2.issue[0].records and emu2.issue[rank].digest() == emu2.issue[0].digest()
    recs0 = emu2.issue[0].records
    assert len({st for n, _, st in recs0 if n == 56 * 25}) == 1                          # shared blocks: always the same stream (the side stream) ...
    assert all(st == recs0[0][2] for n, _, st in recs0 if n != 56 * 25)                  # ... everything else on the stream the solve started on
    for rank in range(1, world):
        assert out2[rank].final_cost == out2[0].final_cost and np.array_equal(handles[rank].get_objects(), handles[0].get_objects())
        assert [i.step_is_successful for i in handles[rank].iterations()] == [i.step_is_successful for i in handles[0].iterations()]
    assert out2[0].final_cost < 0.5 * out2[0].initial_cost
    for hdl in handles:
        hdl.set_allreduce(None)
    own_end = [hdl.evaluate(True, False)[0] for hdl in handles]
    assert abs(sum(own_end) - out2[0].final_cost) <= 1e-9 * out2[0].final_cost               # the state handed back is the job-wide minimum-cost iterate


def _two_process_worker(rank, world, port, wins, prm_kw, out):
    import os
    import sys
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    sys.path.insert(0, os.path.join(helpers.ROOT, "obvi-slam_amd", "python")); sys.path.insert(0, os.path.join(helpers.ROOT, "tests"))
    import torch.distributed as dist
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    q = wins[rank]
    ba = helpers.product_ba()
    synth.upload(ba, q)
    ba.set_shared_objects(np.ones(len(q["objects"]), np.uint8), rank, world)
    calls = []
    hook = dist_util.staged_allreduce(dist)
    ba.set_allreduce(lambda ptr, n, op, stream: calls.append((n, op)) or hook(ptr, n, op, stream))
    s = ba.solve(helpers.ba_params(**prm_kw))
    out[rank] = dict(num_iterations=s.num_iterations, termination_type=s.termination_type, initial_cost=s.initial_cost, final_cost=s.final_cost,
                     accepted=[i.step_is_successful for i in ba.iterations()], costs=[i.cost for i in ba.iterations()],
                     poses=ba.get_poses(), objects=ba.get_objects(), points=ba.get_points(), calls=len(calls), ops=sorted(set(calls)))
    ba.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_processes_exchange_shared_objects_and_land_on_the_oracles_joint_solution(scene):
    """The three-collective protocol of a shared-object solve across a PROCESS boundary: two ranks (both on this GPU -- RCCL will
    not form a communicator of two ranks on one device, so the callback stages through the host and a gloo group carries the
    all-reduce: D2H -> all_reduce -> H2D on the handle's stream).  Both ranks must follow the oracle's joint solve."""
    import socket
    import torch.multiprocessing as mp
    wins, joint, keep_pts = split_problem(scene, 30)
    prm_kw = dict(max_it=15)
    orc = helpers.oracle_ba()
    synth.upload(orc, joint)
    sorc = orc.solve(helpers.ba_params(**prm_kw))
    io = orc.iterations()
    sock = socket.socket(); sock.bind(("127.0.0.1", 0)); port = sock.getsockname()[1]; sock.close()
    mgr = mp.Manager(); out = mgr.dict()
    mp.spawn(_two_process_worker, args=(2, port, [w[0] for w in wins], prm_kw, out), nprocs=2, join=True)
    assert set(out.keys()) == {0, 1}
    jp, jo, jpts = orc.get_poses(), orc.get_objects(), orc.get_points()
    pos = {int(p): i for i, p in enumerate(keep_pts)}
    n_obj = len(scene["objects"])
    for rank in (0, 1):
        o = out[rank]
        assert o["num_iterations"] == sorc.num_iterations and o["termination_type"] == sorc.termination_type
        assert abs(o["initial_cost"] - sorc.initial_cost) <= 1e-10 * sorc.initial_cost and abs(o["final_cost"] - sorc.final_cost) <= 1e-8 * sorc.final_cost
        assert o["accepted"] == [i.step_is_successful for i in io]
        assert max(abs(a - b.cost) / b.cost for a, b in zip(o["costs"], io)) < 1e-8
        a, b = wins[rank][2]
        assert np.abs(o["poses"] - jp[a:b]).max() < 1e-8 and np.abs(o["objects"] - jo).max() < 1e-7
        idx = np.array([pos[int(p)] for p in wins[rank][1]])
        assert np.abs(o["points"] - jpts[idx]).max() < 1e-7
        # per LM submission three collectives, all sums: shared blocks (56 per object), tail, scalars + one gradient-maximum slot per rank
        assert (56 * n_obj, 0) in o["ops"] and (9 + 2, 0) in o["ops"] and all(op == 0 for _, op in o["ops"]) and o["calls"] <= 1 + 3 * sorc.num_iterations
    assert np.array_equal(out[0]["objects"], out[1]["objects"])


def test_two_windows_sharing_objects_equal_the_joint_solve(scene):
    wins, joint, keep_pts = split_problem(scene, 30)
    ref = helpers.product_ba()
    synth.upload(ref, joint)
    prm = helpers.ba_params(max_it=15)
    sref = ref.solve(prm)
    emu = EmulatedAllReduce(2)
    handles, out = [], [None, None]
    for rank, (q, pts, rng) in enumerate(wins):
        ba = helpers.product_ba()
        synth.upload(ba, q)
        ba.set_shared_objects(np.ones(len(q["objects"]), np.uint8), rank, 2)
        ba.set_allreduce(emu.hook(rank))
        handles.append(ba)

    def run(rank):
        out[rank] = handles[rank].solve(prm)
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    [t.start() for t in th]; [t.join(timeout=300) for t in th]
    assert all(o is not None for o in out) and emu.calls > 0
    for o in out:
        assert o.num_iterations == sref.num_iterations and o.termination_type == sref.termination_type
        assert abs(o.final_cost - sref.final_cost) <= 1e-8 * sref.final_cost        # every rank reports the job-wide cost
    jp, jo, jpts = ref.get_poses(), ref.get_objects(), ref.get_points()
    assert np.abs(handles[0].get_poses() - jp[:30]).max() < 1e-8 and np.abs(handles[1].get_poses() - jp[30:]).max() < 1e-8
    assert np.abs(handles[0].get_objects() - jo).max() < 1e-7 and np.abs(handles[1].get_objects() - handles[0].get_objects()).max() == 0.0
    pos = {int(p): i for i, p in enumerate(keep_pts)}
    for rank, (q, pts, rng) in enumerate(wins):
        idx = np.array([pos[int(p)] for p in pts])
        assert np.abs(handles[rank].get_points() - jpts[idx]).max() < 1e-7


def test_rccl_hook_through_torch_distributed(scene):
    """The production hook (dist_util.torch_allreduce: RCCL via torch.distributed, enqueued on the library's own stream
    through torch.cuda.ExternalStream) on a one-rank process group: the plumbing must leave the solve unchanged."""
    import os
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
    torch.cuda.set_device(0)
    dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        a, b = helpers.product_ba(), helpers.product_ba()
        for ba in (a, b):
            synth.upload(ba, scene)
        b.set_shared_objects(np.ones(len(scene["objects"]), np.uint8), 0, 1)
        b.set_allreduce(dist_util.torch_allreduce(dist))
        prm = helpers.ba_params(max_it=10)
        sa, sb = a.solve(prm), b.solve(prm)
        assert sb.num_iterations == sa.num_iterations and abs(sb.final_cost - sa.final_cost) <= 1e-9 * sa.final_cost
        assert np.abs(b.get_poses() - a.get_poses()).max() < 1e-9
    finally:
        dist.destroy_process_group()


def test_compiled_rccl_hook_one_rank_communicator(scene):
    """libobvi_rccl.so (include/obvi_rccl.h): the compiled ncclAllReduce forwarder a C/C++ host attaches to the handle.  A box has
    one GPU, so the communicator has one rank: the exchange is an identity and the solve must equal the plain one; the callback
    runs inside obvi_ba_solve without any Python frame."""
    comm = dist_util.RcclComm(0, 1, 0, unique_id=dist_util.RcclComm.unique_id())
    try:
        assert comm.world() == 1
        assert comm.host_allreduce([3.0, -1.0], op=0) == [3.0, -1.0] and comm.host_allreduce([2.5], op=1) == [2.5]
        comm.barrier()
        a, b = helpers.product_ba(), helpers.product_ba()
        for ba in (a, b):
            synth.upload(ba, scene)
        comm.attach(b, np.ones(len(scene["objects"]), np.uint8))
        prm = helpers.ba_params(max_it=10)
        sa, sb = a.solve(prm), b.solve(prm)
        assert sb.num_iterations == sa.num_iterations and abs(sb.final_cost - sa.final_cost) <= 1e-9 * sa.final_cost
        assert np.abs(b.get_poses() - a.get_poses()).max() < 1e-9 and np.abs(b.get_objects() - a.get_objects()).max() < 1e-8
        b.close()
    finally:
        comm.close()


def test_bench_two_ranks_oversubscribed():
    """`bench.py --gpus 2` end to end where only one GPU exists: the script spawns its two ranks itself, both on device 0, process group gloo,
    the three per-step collectives through dist_util.staged_allreduce.  Everything of the N > 1 path that does not need a second device runs:
    self-spawn, per-rank seeds, the scaling baseline, the shared-object exchange, the issue-order check, the timing reduction, the JSON line."""
    import json
    import os
    import subprocess
    import sys
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--gpus", "2", "--oversubscribe", "--full", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"],
                         capture_output=True, text=True, timeout=1500, env=env)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    cfg = line["config"]
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["scaling"] == "weak" and line["unit"] == "LM iterations/s"
    assert cfg["rccl_ranks"] == 2 and cfg["parallelism"] == "windows+allreduce" and cfg["oversubscribed"] and cfg["allreduce_hook"] == "staged-gloo"
    assert cfg["steps_done"] == 3 and cfg["collective_issue_order"]["same_on_every_rank"] and cfg["collective_issue_order"]["collectives_issued"] >= 3 * 3
    assert set(cfg["collectives_us"]) == {"shared_blocks", "shared_tail", "scalars"}
    sb = line["scaling_baseline"]
    assert sb["steps"] == 3 and len(sb["per_rank_value"]) == 2 and sb["value_one_gpu"] > 0
    assert 0 < line["weak_scaling_efficiency"] <= 1.5 and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["roofline"]["kernel"] and "cpu_baseline" not in line


@pytest.mark.parametrize("config", [4, 5])
def test_bench_four_ranks_oversubscribed(config):
    """The N > 2 command line of both shared-object workloads -- `bench.py --gpus 4` -- with all four ranks on this one GPU (`--oversubscribe`: process group gloo, the
    three collectives staged through the host): config 4 (four 500-keyframe windows sharing 25 objects) and config 5 (eight sessions over one 200-object map, two
    fused per rank, as on an eight-GPU node), both with `--full`.  A smoke test of the WHOLE N > 2 path -- self-spawn, seeds, uploads, the scaling baseline / the
    one-session yardstick, three collectives per step in the same order on every rank, the time limit around them, the reduction of the timings, the instrumented
    solves, the one JSON line -- not a timing (DESIGN section 8 used to say "run by hand").  Four ranks rather than eight: eight ranks and this
    process put nine processes on the one device, more than the machines the suite runs on allow at once."""
    import json
    import os
    import subprocess
    import sys
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(helpers.ROOT, "bench.py"), "--gpus", "4", "--oversubscribe", "--full", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--config", str(config)]
    cmd += ["--sessions", "8"] if config == 5 else []                                      # two fused sessions per rank, the split of eight ranks x sixteen sessions
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1700, env=env)
    assert out.returncode == 0, out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    line = json.loads(lines[0])
    cfg = line["config"]
    assert line["n_gpus"] == 4 and line["steps"] == 2 and line["scaling"] == ("weak" if config == 4 else "strong") and line["value"] > 0
    assert cfg["rccl_ranks"] == 4 and cfg["oversubscribed"] and cfg["steps_done"] == 2
    assert cfg["collective_issue_order"]["same_on_every_rank"] and cfg["collective_issue_order"]["collectives_issued"] >= 3 * 2
    if config == 5:
        assert cfg["sessions"] == 8 and cfg["sessions_per_rank"] == 2
        assert line["concurrency"]["sessions_on_this_gpu"] == 2 and line["concurrency"]["one_session_alone_ms_per_step"] > 0 and line["roofline"]["kernel"]
    if config == 4:
        assert len(line["scaling_baseline"]["per_rank_value"]) == 4                      # (config 5 is a strong-scaling workload: no one-window baseline)


def test_rccl_rendezvous_file(tmp_path, monkeypatch):
    """obvi_rccl_comm_create_from_file: the launcher-less rendezvous of a C++ host (rank 0 writes the id, the others poll).  The file lives only
    for the rendezvous: rank 0 replaces whatever an earlier run left at the path and removes its own file once the communicator exists, so a
    second run on the same path can never pick up the first run's id."""
    import os
    for name in ("OBVI_RCCL_JOB", "TORCHELASTIC_RUN_ID", "MASTER_PORT"):      # (no per-launch tag: the file is `path` itself; another test of this process may have left MASTER_PORT behind)
        monkeypatch.delenv(name, raising=False)
    path = str(tmp_path / "rccl_id")
    with open(path, "wb") as f:
        f.write(b"\x5a" * dist_util.RcclComm.ID_BYTES)        # a leftover of a crashed run: a syntactically valid, wrong id
    for _ in range(2):                                        # ... and the same path twice in a row
        comm = dist_util.RcclComm(0, 1, 0, id_file=path)
        try:
            assert comm.world() == 1 and not os.path.exists(path)
        finally:
            comm.close()
    # a per-launch tag from the environment becomes part of the file name: a leftover at the untagged path is not even looked at
    with open(path, "wb") as f:
        f.write(b"\x5a" * dist_util.RcclComm.ID_BYTES)
    monkeypatch.setenv("OBVI_RCCL_JOB", "job 42/a")
    comm = dist_util.RcclComm(0, 1, 0, id_file=path)
    try:
        assert comm.world() == 1 and os.path.exists(path) and not os.path.exists(path + ".job_42_a")
    finally:
        comm.close()


def test_rccl_library_reports_its_version_and_issue_sequence(scene):
    """obvi_rccl_nccl_version (compared with torch's before a communicator is formed: dist_util.RcclComm.check_against_torch) and
    obvi_rccl_sequence (calls + hash of the data-path collectives, what ranks compare to prove the same host issue order)."""
    ok, ours, theirs = dist_util.RcclComm.check_against_torch()
    assert ours > 20000 and (theirs is None or ok == (ours == theirs))
    comm = dist_util.RcclComm(0, 1, 0, unique_id=dist_util.RcclComm.unique_id())
    try:
        assert comm.sequence()[0] == 0
        b = helpers.product_ba()
        synth.upload(b, scene)
        comm.attach(b, np.ones(len(scene["objects"]), np.uint8))
        s = b.solve(helpers.ba_params(max_it=4))
        calls, digest = comm.sequence()
        assert calls >= 3 * (s.num_iterations - 1) and digest != 1469598103934665603 and comm.same_issue_order()
        b.close()
    finally:
        comm.close()
