"""Helper of tests/test_gpu_solve_slots.py: cases of tests/solve_slots_cases.py in THIS process, whose environment decides the
number of solve slots (MI_ILQR_SOLVE_SLOTS is read once per process).
`python tests/_solve_slots_child.py OUT.npz blocking|pipelined [case ...]` writes one array per case and result (no case named: all
but `lazy`, which measures the process's device memory and wants a process of its own)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

if __name__ == "__main__":
    import solve_slots_cases as cases
    names = sys.argv[3:] or [c for c in cases.CASES if c != "lazy"]
    np.savez(sys.argv[1], **cases.run_all(pipelined=sys.argv[2] == "pipelined", names=names))
