"""What the fused learner updates show through the C ABI without a device: every `armenv_*_workspace_bytes` answer over a grid of
shapes, and the return code and `armenv_last_error()` text of every refusal that the three host test modules parametrise (and of a
NULL `args`).  `record()` takes them from the library that armenv._lib loads; tests/golden/gen_learner_abi.py wrote
tests/golden/learner_abi.json with it, and test_learner_abi.py holds every later build to that file."""
import ctypes as C
import importlib

ALGOS = {"td3": ("test_td3_fused_host", "test_bad_arguments_are_refused_before_any_device_call"),
         "daddpg": ("test_daddpg_fused_host", "test_daddpg_bad_arguments_are_refused_before_any_device_call"),
         "datd3": ("test_datd3_host", "test_datd3_bad_arguments_are_refused_before_any_device_call")}
STATE_DIMS = tuple(range(14))
HIDDEN_DIMS = (128, 256)
BATCHES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 2048, 8192, 1 << 20, (1 << 20) + 1)


def _mutations(algo):
    """(the module's `_args`, [(field, mutate)]) of the host test's parametrised refusals"""
    module, test = ALGOS[algo]
    mod = importlib.import_module(module)
    (mark,) = [m for m in getattr(mod, test).pytestmark if m.name == "parametrize"]
    return mod._args, list(mark.args[1])


def record():
    from armenv import _lib as L
    lib = L.load()
    out = {"sizes": {}, "refusals": {}}
    for algo in ALGOS:
        query = getattr(lib, "armenv_%s_workspace_bytes" % algo)
        update = getattr(lib, "armenv_%s_update" % algo)
        out["sizes"][algo] = [[D, H, B, int(query(D, H, B))] for D in STATE_DIMS for H in HIDDEN_DIMS for B in BATCHES]
        make, muts = _mutations(algo)
        rows = []
        for i, (field, mutate) in enumerate(muts):
            a = make()
            mutate(a)
            rc = update(C.byref(a), None)
            rows.append(["%d %s" % (i, field), int(rc), lib.armenv_last_error().decode()])
        rc = update(None, None)
        rows.append(["NULL args", int(rc), lib.armenv_last_error().decode()])
        out["refusals"][algo] = rows
    return out
