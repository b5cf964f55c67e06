"""CPU: the C-ABI library builds for gfx950, loads, exports every declared symbol and refuses to run without a GPU."""
import ctypes as C
import os

import pytest

import helpers
import obvi_ba


def _abi_symbols():
    import __graft_entry__ as ge
    return ge.abi_symbols()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(helpers.PRODUCT_LIB):
        import __graft_entry__ as ge
        ge.build()
    return C.CDLL(helpers.PRODUCT_LIB)


def test_exports_every_declared_symbol(lib):
    syms = _abi_symbols()
    assert len(syms) >= 30
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing


def test_frontend_and_rccl_libraries_export_their_headers(lib):
    import __graft_entry__ as ge
    front = ge.abi_symbols("obvi_frontend.h", "obvi_frontend_")
    assert set(front) == {"obvi_frontend_epipolar_votes", "obvi_frontend_epipolar_errors", "obvi_frontend_parallax"}
    assert not [s for s in front if not hasattr(lib, s)]
    o = C.CDLL(helpers.ensure_oracle())
    assert all(hasattr(o, s.replace("obvi_", "oracle_", 1)) for s in front)
    rccl_path = os.path.join(os.path.dirname(helpers.PRODUCT_LIB), "libobvi_rccl.so")
    syms = ge.abi_symbols("obvi_rccl.h", "obvi_rccl_")
    assert len(syms) >= 10 and "obvi_rccl_allreduce" in syms
    rccl = C.CDLL(rccl_path)                       # links librccl: loads without a GPU; communicators need one
    assert not [s for s in syms if not hasattr(rccl, s)]
    # libobvi_ba.so itself must not depend on RCCL (the collective is a callback)
    import subprocess
    needed = subprocess.run(["readelf", "-d", helpers.PRODUCT_LIB], capture_output=True, text=True).stdout
    assert "rccl" not in needed.lower()


def test_oracle_mirrors_the_abi():
    o = C.CDLL(helpers.ensure_oracle())
    skip = {"obvi_ba_last_error", "obvi_ba_version", "obvi_ba_get_kernel_times", "obvi_ba_get_problem_stats", "obvi_ba_set_profiling", "obvi_ba_measure_peaks"}   # device-only hooks
    for s in _abi_symbols():
        if s not in skip:
            assert hasattr(o, s.replace("obvi_", "oracle_", 1)), s


def test_version_and_struct_sizes(lib):
    lib.obvi_ba_version.restype = C.c_char_p
    assert b"gfx950" in lib.obvi_ba_version()
    assert C.sizeof(obvi_ba.SolverParams) == 48 and C.sizeof(obvi_ba.IterationSummary) == 80 and C.sizeof(obvi_ba.Summary) == 248


def test_no_cpu_fallback(lib):
    """Without a HIP device the product refuses to create a handle (OBVI_ERR_NO_DEVICE); it never computes on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    h = C.c_void_p()
    opt = obvi_ba.Options(0, 7)
    assert lib.obvi_ba_create(C.byref(opt), C.byref(h)) == -2
    with pytest.raises(obvi_ba.ObviError):
        obvi_ba.BundleAdjuster(device_id=0)
    with pytest.raises(obvi_ba.ObviError):
        obvi_ba.BundleAdjuster(library="/nonexistent/libobvi_ba.so")


def test_invalid_arguments(lib):
    assert lib.obvi_ba_create(None, None) == -1
    bad = obvi_ba.Options(0, 8)     # an ellipsoid block has 7 (yaw only) or 9 (axis-angle) parameters
    h = C.c_void_p()
    assert lib.obvi_ba_create(C.byref(bad), C.byref(h)) == -1
    assert lib.obvi_ba_solve(None, None, None) == -1
    assert lib.obvi_ba_object_covariances(None, C.c_int64(0), None, None, None) == -1


def _relpose_between_a_pose_and_itself_is_refused(ba):
    """set_relpose with pose_idx_a[i] == pose_idx_b[i]: OBVI_ERR_INVALID_ARGUMENT, nothing stored, the factors set before stay"""
    import numpy as np
    import synth
    prob = synth.make_problem(P=8, L=60, O=0, seed=5)
    synth.upload(ba, prob)
    cost0, _, sq0 = ba.evaluate(True)
    n = len(prob["rl_a"])
    assert n == 7 and ba.num_factors(obvi_ba.FACTOR_REL_POSE) == n
    f = ba._fn("ba_num_factors")
    a, b = prob["rl_a"].copy(), prob["rl_b"].copy()
    for at in (0, 3, n - 1):                      # first, middle and last factor of the call
        bad_b = b.copy(); bad_b[at] = a[at]
        with pytest.raises(obvi_ba.ObviError, match="status -1"):
            ba.set_relpose(a, bad_b, prob["rl_t"], prob["rl_aa"], prob["rl_cov"], prob["rl_huber"])
        assert f(ba._h, C.c_int32(obvi_ba.FACTOR_REL_POSE)) == n
    with pytest.raises(obvi_ba.ObviError, match="status -1"):   # a call of one such factor alone
        ba.set_relpose(a[:1], a[:1], prob["rl_t"][:1], prob["rl_aa"][:1], prob["rl_cov"][:1], prob["rl_huber"])
    assert f(ba._h, C.c_int32(obvi_ba.FACTOR_REL_POSE)) == n
    cost1, _, sq1 = ba.evaluate(True)
    assert cost1 == cost0 and np.array_equal(sq1, sq0) and sq1[-n:].min() > 0
    ba.set_relpose(b, a, prob["rl_t"], prob["rl_aa"], prob["rl_cov"], prob["rl_huber"])   # the reverse order is a valid factor
    assert f(ba._h, C.c_int32(obvi_ba.FACTOR_REL_POSE)) == n


def test_oracle_refuses_a_relpose_factor_between_a_pose_and_itself():
    _relpose_between_a_pose_and_itself_is_refused(helpers.oracle_ba())


@pytest.mark.gpu
def test_product_refuses_a_relpose_factor_between_a_pose_and_itself():
    g = helpers.product_ba()
    _relpose_between_a_pose_and_itself_is_refused(g)
    with pytest.raises(obvi_ba.ObviError, match="a pose and itself"):
        g.set_relpose([2], [2], [[0.1, 0, 0]], [[0, 0, 0.01]], [[1 if i % 7 == 0 else 0 for i in range(36)]], 1.0)


def test_generator_shapes():
    import numpy as np
    import synth
    prob = synth.make_problem(P=40, L=500, O=3, seed=3, min_obj_obs=5)
    st = synth.problem_stats(prob)
    assert st["P"] == 40 and st["L"] == 500 and st["O"] == 3 and st["N_rel"] == 39
    cnt = np.bincount(prob["rp_point"], minlength=500)
    assert cnt.min() >= 5                                  # min_low_level_feature_observations
    assert np.all(np.diff(prob["rp_point"].astype(np.int64)) >= 0)
    assert np.bincount(prob["bb_obj"], minlength=3).min() >= 5
    px, z = synth.project_points(prob["gt_poses"][prob["rp_pose"]], prob["gt_points"][prob["rp_point"]])
    inl = ~prob["rp_is_outlier"]
    assert np.abs(px - prob["rp_pixel"])[inl].std() < 1.2 and z.min() > 0.5


def test_host_pool_hands_every_part_out_exactly_once(tmp_path):
    """csrc/host_util.h HostPool (the worker threads of the symbolic phase): 40 000 back-to-back runs of changing part counts from two
    caller threads -- every part exactly once, nothing after run() has returned (a part index could cross from one run to the next)."""
    import subprocess
    exe = str(tmp_path / "hostpool_stress")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", exe, os.path.join(helpers.ROOT, "tests", "hostpool_stress.cpp")])
    out = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout + out.stderr


def _function_body(src, signature):
    """The definition of the C++ function that starts with `signature`, up to its matching closing brace."""
    start = src.index(signature)
    depth = 0
    for j in range(src.index("{", start), len(src)):
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        if depth == 0:
            return src[start:j + 1]
    raise AssertionError("unbalanced braces after " + signature)


def test_knobs_are_read_in_one_place_and_documented():
    """The library reads its environment in read_knobs() and process_knobs() alone (abi.cpp; obvi_rccl.cpp reads the rendezvous names), the host
    mirror's headers in host_knobs() alone (obvi_params.h), and INTEGRATION.md section 5 lists exactly the OBVI_* names these functions read."""
    import re
    csrc = os.path.join(helpers.ROOT, "obvi-slam_amd", "csrc")
    host = os.path.join(helpers.ROOT, "obvi-slam_amd", "host")
    readers = {os.path.join(csrc, "abi.cpp"): ("Knobs read_knobs()", "const ProcessKnobs& process_knobs()"),
               os.path.join(host, "obvi_params.h"): ("inline const HostKnobs& host_knobs()",)}
    sources = [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".h")) and f != "obvi_rccl.cpp"]
    sources += [os.path.join(host, f) for f in sorted(os.listdir(host)) if f.endswith(".h")]
    read = set()
    for path in sources:
        src = open(path).read()
        for signature in readers.get(path, ()):
            body = _function_body(src, signature)
            read |= set(re.findall(r'"(OBVI_[A-Z0-9_]+)"', body))
            src = src.replace(body, "")
        assert "getenv" not in src, path
    text = open(os.path.join(helpers.ROOT, "INTEGRATION.md")).read()
    section = text[text.index("## 5. "):text.index("## 6. ")]
    first_cells = [line.split("|")[1] for line in section.splitlines() if line.startswith("| `OBVI_")]
    table = set(re.findall(r"`(OBVI_[A-Z0-9_]+)`", "\n".join(first_cells))) - {"OBVI_RCCL_JOB", "OBVI_BA_LIBRARY"}
    assert read == table, (sorted(read - table), sorted(table - read))


def test_only_the_lm_step_launches_the_assembly():
    """The kernels that assemble the reduced system are launched from lm.cpp alone (assemble_step): obvi_ba_debug_reduced_system runs the
    LM step's own stage, not a copy of its launch sequence that the parity tests would check instead of the solver's."""
    import re
    csrc = os.path.join(helpers.ROOT, "obvi-slam_amd", "csrc")
    names = ("launch_point_pass", "launch_pose_pass", "launch_small_factors", "launch_reduced_diag", "launch_schur_window", "launch_schur_blocks")
    callers = {name: set() for name in names}
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".cpp", ".hip", ".h")):
            src = open(os.path.join(csrc, f)).read()
            for name in names:
                if re.search(r"(?<!void )\b%s\s*\(" % name, src):   # a call, not the declaration or the definition
                    callers[name].add(f)
    assert callers == {name: {"lm.cpp"} for name in names}, callers
