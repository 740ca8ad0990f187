"""Recorder of tests/golden/optim_parent.npz: what run() of tests/test_optim_parent_gpu.py gives on a build of the commit named on the command
line.  run() uses only the optimizer's public surface: on a commit that does not have that test yet, copy it and this script next to that
commit's build (they need nothing else that is newer).

The optimizer's kernels have no atomics and a fixed order of additions, so every case runs twice, in fresh optimizers, and a case in which
anything differs between the two runs is reported and not recorded at all.

    python tests/golden/make_optim_parent.py --commit <hash> [--out tests/golden/optim_parent.npz]
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import test_optim_parent_gpu as G     # noqa: E402  (tests/ must be on the path first)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "optim_parent.npz"))
    args = ap.parse_args()
    data = {"commit": np.array(args.commit), "device": np.array(f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})"),
            "toolchain": np.array(f"torch {torch.__version__}, HIP {torch.version.hip}")}
    dropped = []
    for case, precision in G.RUNS:
        a, b = G.run(case, precision), G.run(case, precision)
        same = str(a["names"]) == str(b["names"]) and np.array_equal(a["values"], b["values"])
        print(f"{case}.{precision}: {a['values'].shape[0]} records of {a['values'].shape[1]} quantities"
              + ("" if same else "; NOT RECORDED, differs between two runs"), flush=True)
        if not same:
            dropped.append(f"{case}.{precision}")
            continue
        for k, x in a.items():
            data[f"{case}.{precision}.{k}"] = x
    np.savez_compressed(args.out, **data)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, commit {args.commit}, device {data['device']}, not recorded: {dropped}")
    return 1 if dropped else 0


if __name__ == "__main__":
    sys.exit(main())
