#!/bin/bash
# A/B timing of two builds of libarmenv.so with the kernel-time probe (time_rollout.py) inside ONE GPU session:
#   gpurun -- 'bash tests/tools/ab_time.sh drl-on-robot-arm_amd/build/ab/libarmenv_x.so [rounds] -- <time_rollout args>'
# alternates `other` and the current library (ARMENV_LIB of the caller, else the tree's) `rounds` times (default 3).  Every run has a
# time limit of its own, and the first one that fails ends the script: nothing more is started on a GPU that has faulted.
set -o pipefail
OTHER=$PWD/$1; shift
R=3; if [ "$1" != "--" ]; then R=$1; shift; fi; shift
run() { timeout -k 10 300 python tests/tools/time_rollout.py "$@" 2>&1 | grep -v amdgpu.ids; }
for r in $(seq $R); do
  ARMENV_LIB=$OTHER run "$@" || exit 1
  run "$@" || exit 1
done
