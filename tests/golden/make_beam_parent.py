"""Recorder of tests/golden/beam_parent.npz: the outputs of av_ctc_beam_search and av_ctc_beam_search_lm on the cases of
tests/test_beam_parent_gpu.py, taken from a build of the commit named on the command line (the last one with two separate search kernels).
Only the exported C entry points are used, through run() of tests/test_beam_parent_gpu.py: on a commit that does not have that test yet,
copy it and this script next to that commit's build (they need nothing else that is newer).  Both libraries are run and must agree; the
file holds outputs only (the inputs are regenerated from their seeds), compressed, with the commit and the device named inside.

    python tests/golden/make_beam_parent.py --commit <hash> [--out tests/golden/beam_parent.npz]
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import test_beam_parent_gpu as G        # noqa: E402  (tests/ must be on the path first)
from conftest import pkg                # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "beam_parent.npz"))
    args = ap.parse_args()
    P = pkg("precision")
    data = {"commit": np.array(args.commit), "device": np.array(f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName})"),
            "toolchain": np.array(f"torch {torch.__version__}, HIP {torch.version.hip}")}
    for case in G.PLAIN + G.FUSED:
        runs = []
        for mode in ("fp32", "fp16"):
            P.set_precision(mode)
            runs.append(G.run(case))
        for k, x in runs[0].items():
            assert np.array_equal(x, runs[1][k]), f"{G.name(case)}.{k}: the two libraries differ"
            data[f"{G.name(case)}.{k}"] = x
        n = runs[0]["len"]
        print(f"{G.name(case)}: hypotheses per utterance {(n >= 0).sum(axis=1).tolist()}, longest {int(n.max())}")
    np.savez_compressed(args.out, **data)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, commit {args.commit}, device {data['device']}")


if __name__ == "__main__":
    main()
