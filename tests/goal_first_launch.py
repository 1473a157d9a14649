"""TEST INFRASTRUCTURE — run as a program, in a process of its own, by tests/test_hip_goal_distance.py:

    python tests/goal_first_launch.py W H

The process's FIRST launch of goal_lds_kernel is the edge shape W x H of tests/goal_cases.py, through the bare C ABI with the LDS
kernel named.  hipFuncSetAttribute(hipFuncAttributeMaxDynamicSharedMemorySize) acts on the function for the rest of a process,
so only a process that has not yet launched a larger grid shows what the runtime accepts at 146 x 193 — exactly 65 536 bytes of
dynamic LDS, for which launch_goal_distance sets no attribute.  The launch must return 0 and give the reference's distances and
field, with the field and without; then the line FIRST_LDS_LAUNCH_OK W H bytes is printed."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE, os.path.join(HERE, "native")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(W, H):
    import numpy as np
    import goal_cases
    import test_hip_goal_distance as T
    from marlgrid_amd import _native as N
    case, dist, field = goal_cases.edge(W, H)
    assert not goal_cases.reg_fits(W, H)
    dev = T._Device(case)
    d, f = dev.run(N.GOAL_PATH_LDS)         # (asserts the return code)
    assert np.array_equal(d, dist) and np.array_equal(f, field)
    d, f = dev.run(N.GOAL_PATH_LDS, field=False)
    assert np.array_equal(d, dist) and (f == -7).all()
    print("FIRST_LDS_LAUNCH_OK %d %d %d" % (W, H, goal_cases.scratch_bytes(W, H)))


if __name__ == "__main__":
    main(int(sys.argv[1]), int(sys.argv[2]))
