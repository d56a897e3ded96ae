"""What the fused learner updates show through the C ABI without a device: every `armenv_*_workspace_bytes` answer over a grid of
shapes, and the return code and `armenv_last_error()` text of every refusal of learner_host.REFUSALS, which the three host test
modules parametrise (and of a NULL `args`).  `record()` takes them from the library that armenv._lib loads;
tests/golden/gen_learner_abi.py wrote tests/golden/learner_abi.json with it, and test_learner_abi.py holds every later build to that
file."""
import ctypes as C

from learner_host import REFUSALS, fake_args

ALGOS = {"td3": "td3", "daddpg": "daddpg", "datd3": "darc"}        # entry point -> the kind whose fake_args its refusals break
STATE_DIMS = tuple(range(14))
HIDDEN_DIMS = (128, 256)
BATCHES = (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 2048, 8192, 1 << 20, (1 << 20) + 1)


def record():
    from armenv import _lib as L
    lib = L.load()
    out = {"sizes": {}, "refusals": {}}
    for algo in ALGOS:
        query = getattr(lib, "armenv_%s_workspace_bytes" % algo)
        update = getattr(lib, "armenv_%s_update" % algo)
        out["sizes"][algo] = [[D, H, B, int(query(D, H, B))] for D in STATE_DIMS for H in HIDDEN_DIMS for B in BATCHES]
        rows = []
        for i, (field, mutate) in enumerate(REFUSALS[algo]):
            a = fake_args(ALGOS[algo])
            mutate(a)
            rc = update(C.byref(a), None)
            rows.append(["%d %s" % (i, field), int(rc), lib.armenv_last_error().decode()])
        rc = update(None, None)
        rows.append(["NULL args", int(rc), lib.armenv_last_error().decode()])
        out["refusals"][algo] = rows
    return out
