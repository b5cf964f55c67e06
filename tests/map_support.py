"""What the tests of the device-resident map share (tests/test_gpu_map_*.py, tests/test_map_*_abi.py): the handles that only lend their stream and workspaces,
the status and error text of a call, the two error figures of a new map, the short iteration record, and the reader of the ABI headers.  A plain module,
imported like `helpers`; nothing here touches a device before it is called."""
import ctypes as C
import os

import numpy as np

import helpers
import obvi_ba
import synth


def header(name):
    return open(os.path.join(helpers.ROOT, "include", name)).read()


def objects_only(objects, od=7, **options):
    """One constant pose, no features, no factors but what the caller adds."""
    ba = helpers.product_ba(object_block_size=od, **options)
    ba.set_cameras(synth.K_DEFAULT[None], synth.EXT_DEFAULT[None])
    ba.set_poses(np.zeros((1, 6)), np.ones(1, np.uint8))
    ba.set_points(np.zeros((0, 3)), np.zeros(0, np.uint8))
    ba.set_objects(objects, np.zeros(len(objects), np.uint8))
    return ba


def det_objects_only(objects, od=7):
    return objects_only(objects, od, deterministic=True)


def lender(od, deterministic=False):
    """A handle that only lends its stream and workspaces."""
    return (det_objects_only if deterministic else objects_only)(np.zeros((1, od)), od)


def status_of(call):
    try:
        call()
    except obvi_ba.ObviError as e:
        return int(str(e).split("status ")[1].split()[0])
    return 0


def last_error(ba):
    f = ba._fn("ba_last_error")
    f.restype = C.c_char_p
    return (f(ba._h) or b"").decode()


def errors(mean, cov, mean_ref, cov_ref):
    """(covariance, means): the largest difference over the largest entry of the reference."""
    return (float(np.abs(cov - cov_ref).max() / np.abs(cov_ref).max()), float(np.abs(mean - mean_ref).max() / np.abs(mean_ref).max()))


def records(ba):
    return [(i.iteration, i.step_is_successful, i.cost) for i in ba.iterations()]
