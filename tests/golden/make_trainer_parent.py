"""Recorder of tests/golden/trainer_parent.npz: what run() of tests/test_trainer_parent_gpu.py gives on a build of the commit named on the command
line.  run() uses only the trainer's public surface: on a commit that does not have that test yet, copy it, tests/trainer_util.py and this script
next to that commit's build (they need nothing else that is newer).

A recording of a program that is not reproducible from run to run would be worthless, so every case runs twice, in fresh trainers, and only what
is bit-equal between the two runs is kept.  The step-1 scalars, everything from evaluate() and align(), and every parameter checksum must be
equal; only ``k_proj.bias`` tensors (test_step_gpu.py says why) and step-2 scalars may be left out, and they are listed per case under
``<case>.<precision>.left_out``.  A case in which anything else differs is reported and not recorded at all.

    python tests/golden/make_trainer_parent.py --commit <hash> [--out tests/golden/trainer_parent.npz]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import test_trainer_parent_gpu as G     # noqa: E402  (tests/ must be on the path first)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "trainer_parent.npz"))
    args = ap.parse_args()
    data = {"commit": np.array(args.commit), "device": np.array(f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})"),
            "toolchain": np.array(f"torch {torch.__version__}, HIP {torch.version.hip}")}
    dropped = []
    for case, precision in G.RUNS:
        a, b = G.run(case, precision), G.run(case, precision)
        assert sorted(a) == sorted(b), (case, precision)
        names = json.loads(str(a["state.names"]))
        out_state = [n for n, x, y in zip(names, a["state.sums"], b["state.sums"]) if x != y]
        out_q = [k for k in a if k != "state.sums" and not np.array_equal(a[k], b[k])]
        bad = [n for n in out_state if not n.endswith("k_proj.bias")] + [k for k in out_q if not k.startswith("step2.")]
        print(f"{case}.{precision}: left out {out_state + out_q}" + (f"; NOT RECORDED, differs between two runs: {bad}" if bad else ""), flush=True)
        if bad:
            dropped.append(f"{case}.{precision}")
            continue
        for k, x in a.items():
            if k not in out_q:
                data[f"{case}.{precision}.{k}"] = x
        data[f"{case}.{precision}.left_out"] = np.array(json.dumps({"state": out_state, "quantities": out_q}))
    np.savez_compressed(args.out, **data)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, commit {args.commit}, device {data['device']}, not recorded: {dropped}")


if __name__ == "__main__":
    main()
