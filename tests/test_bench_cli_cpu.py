"""CPU: bench.py's command-line contract that needs no GPU - `--gpus N` typed directly starts N ranks under torch.distributed.run
(before anything touches the GPU) and relays their exit code; the FLOP accounting of the two variants."""
import importlib.util
import os
import sys

from conftest import ROOT, pkg


def _load_bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_gpus_n_spawns_one_rank_per_gpu(monkeypatch):
    b = _load_bench()
    seen = {}

    def fake_call(cmd, env=None):
        seen["cmd"], seen["env"] = cmd, env
        return 7

    import subprocess
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3", "--warmup", "1"])
    assert b.spawn_ranks(4) == 7                                  # the children's exit code is relayed
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-6:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"] and cmd[-7].endswith("bench.py")
    assert seen["env"].get("HSA_ENABLE_IPC_MODE_LEGACY") == "0"


def test_flop_accounting_matches_survey_numbers():
    """4 s clips - 419 GF per utterance de-duplicated, 682 GF with two full audio passes (bench.py counts the shared conv
    feature extractor once: 662 GF)."""
    b = _load_bench()
    cfg = pkg("utils.init").W2V2_LARGE
    one = b.flops_per_utt(cfg, 64000, 100, 1) / 1e9
    two = b.flops_per_utt(cfg, 64000, 100, 2) / 1e9
    assert abs(one - 418.5) < 1.0 and abs(two - 662.2) < 1.0
    conv = sum(2.0 * k * ci * c * L for k, ci, c, L in zip(cfg["conv_kernel"], (1,) + tuple(cfg["conv_dim"][:-1]), cfg["conv_dim"],
                                                            (12799, 6399, 3199, 1599, 799, 399, 199))) / 1e9
    assert abs((two + conv) - 682.0) < 2.0


def test_flop_accounting_counts_executed_layers():
    """The LayerDrop draws are on the host, so bench.py prices the layers actually executed (forward / backward without / with weight
    gradients, summed over the passes), not an expectation: all layers executed = the plain two-pass figure; a dropped layer removes exactly
    its own forward and backward products."""
    b = _load_bench()
    cfg = pkg("utils.init").W2V2_LARGE
    full = b.flops_per_utt(cfg, 64000, 100, 2)
    assert b.flops_per_utt(cfg, 64000, 100, 2, (48, 28, 8)) == full
    H, I, T = cfg["hidden_size"], cfg["intermediate_size"], 199
    lin = (8.0 * H * H + 4.0 * H * I) * T
    att = 4.0 * T * T * H
    # one frozen layer (no backward) and one trainable layer (dX + dW) dropped in one pass each
    got = b.flops_per_utt(cfg, 64000, 100, 2, (46, 28, 7))
    assert abs((full - got) - ((lin + att) + (lin + att) + (2 * lin + 2 * att))) < 1.0
    # per-step averages need not be integers (LayerDrop over 30 timed steps)
    assert b.flops_per_utt(cfg, 64000, 100, 2, (43.0, 25.13, 7.13)) < full


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """--dump-outputs: small arrays are written whole in float32, a large one as a seeded sample at the same positions from run to run,
    the trainable parameters flattened in order; the whole dump stays within 64 MB."""
    import numpy as np
    import torch
    b = _load_bench()
    big = torch.arange(3 * b.DUMP_MAX_ELEMS, dtype=torch.float64).reshape(3, -1)
    out = {"total": torch.tensor(1.5), "lengths": torch.tensor([3, 4]), "big": big.to(torch.bfloat16)}
    params = [torch.ones(2, 3), torch.zeros(5)]
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), out, params)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(got) == {"total", "lengths", "big", "trainable_params"}
    assert all(a.dtype == np.float32 for a in got.values())
    assert float(got["total"]) == 1.5 and got["lengths"].tolist() == [3.0, 4.0]
    assert got["trainable_params"].tolist() == [1.0] * 6 + [0.0] * 5
    s = got["big"]
    assert s.shape == (b.DUMP_MAX_ELEMS,) and np.all(np.diff(s) >= 0)            # sorted positions of an increasing array
    assert np.array_equal(s, big.reshape(-1).to(torch.bfloat16).float().numpy()[np.sort(np.random.default_rng(0).choice(big.numel(), b.DUMP_MAX_ELEMS, replace=False))])
    assert np.array_equal(s, np.load(tmp_path / "b" / "big.npy"))
    assert sum(a.nbytes for a in got.values()) <= 64 << 20


def test_plain_run_leaves_the_extra_legs_to_full():
    """Without --full a run times the headline variant only (no other variant, probe leg or CPU baseline); --full brings them back, and
    the three options that leave one of them out still work under it."""
    b = _load_bench()
    a = b.parse_args(["--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert a.single_variant and a.no_probe and a.no_cpu_baseline
    a = b.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d" and not (a.single_variant or a.no_probe or a.no_cpu_baseline)
    a = b.parse_args(["--full", "--no-cpu-baseline"])
    assert a.no_cpu_baseline and not (a.single_variant or a.no_probe)
