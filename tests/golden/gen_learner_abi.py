#!/usr/bin/env python3
"""Generates tests/golden/learner_abi.json (companion of gen_fixtures.py; needs no reference checkout): the workspace sizes and the
refusals (return code and armenv_last_error() text) of armenv_td3_update, armenv_daddpg_update and armenv_datd3_update, recorded by
tests/learner_abi.py from the library that ARMENV_LIB names (default: the built armenv/libarmenv.so).

The committed file was recorded from the build of the commit BEFORE the three updates were folded into one launch sequence
("Add DATD3 and DARC learners and their fused HIP update (ABI 8)"), so test_learner_abi.py holds the ABI-visible behaviour to that
commit's.  Regenerate it only for a change that is meant to alter a size or a message, from a build that has the change."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "drl-on-robot-arm_amd"), ROOT):
    sys.path.insert(0, p)

import learner_abi  # noqa: E402

if __name__ == "__main__":
    rec = learner_abi.record()
    with open(os.path.join(HERE, "learner_abi.json"), "w") as fh:
        json.dump(rec, fh, indent=0, separators=(",", ":"))
        fh.write("\n")
    print({k: {a: len(v) for a, v in rec[k].items()} for k in rec})
