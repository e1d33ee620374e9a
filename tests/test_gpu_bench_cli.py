"""bench.py as the driver calls it: `python bench.py --gpus N ...` must start its own ranks and print ONE JSON
line on rank 0.  Two ranks on ONE GPU over gloo (test hooks SBMC_BENCH_BACKEND / SBMC_BENCH_SINGLE_DEVICE):
everything but the RCCL transport, on a tiny frame."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--height", "64", "--width", "96", "--spp", "2", "--ksize", "5", "--steps", "2", "--warmup", "2"]
# what takes runs of its own sits behind --full; the CPU baseline is left out of it here, the stages where a test does not read them
FULL = ["--full", "--no-cpu-baseline"]


def _run(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                         env=e, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def _dumped(path):
    import numpy as np
    return {f.name[:-4]: np.load(str(f)) for f in sorted(path.iterdir())}


def test_bench_line_carries_the_inference_matrix():
    """north_star's matrix in the --full line: forward-only stages at 4 / 8 / 32 spp, the forward kernel's
    roofline entry, the whole step's TFLOP/s and the U-nets' layout (tiny frame here)."""
    d = _run(SMALL + FULL)
    for spp in (4, 8, 32):
        st = d["stages"]["infer_%dspp" % spp]
        assert st["value"] > 0 and st["unit"] == "Msamples/s" and st["steps"] == 10
    assert d["whole_step_tflops"] > 0 and 0 < d["multiples_of_fp32_mfma_peak"] < 3 and "unet_layout" in d
    assert "roofline" in d and "stages" in d and "splat" in d["stages"]


def test_bench_single_gpu_line(tmp_path):
    """The plain line: the timed steps and nothing that takes runs of its own; --dump-outputs writes what the last timed
    step returned."""
    import numpy as np
    d = _run(SMALL + ["--dump-outputs", str(tmp_path)])
    assert d["full"] is False and d["ms_per_step"] > 0
    for key in ("stages", "fp32_pipe", "cpu_baseline", "parity", "pointwise_layers", "conv3x3"):
        assert key not in d, key
    out = _dumped(tmp_path)
    assert sorted(out) == ["grads", "loss", "radiance"]
    for a in out.values():
        assert a.dtype == np.float32 and np.isfinite(a).all()
    assert out["radiance"].ndim == 4 and out["radiance"].shape[:2] == (1, 3)
    assert out["loss"].shape == () and out["grads"].ndim == 1
    assert np.abs(out["grads"]).max() > 0
    assert d["n_gpus"] == 1 and d["world_size"] == 1 and d["value"] > 0 and d["unit"] == "Msamples/s"
    assert d["steps"] == 2 and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step_median"] > 0 and len(d["ms_per_step_min_max"]) == 2
    # the roofline kernel is timed INSIDE the training step's timed region: one launch of each splat operator per timed step
    ks = d["kernels_in_step"]
    assert ks["splat_update_bwd_all"]["calls"] == 2 and ks["splat_update_fwd_all"]["calls"] == 2
    assert d["roofline"]["launches"] == 2 and "inside the timed steps" in d["roofline"]["timed"]
    assert d["roofline"]["avg_launch_ms"] == ks["splat_update_bwd_all"]["avg_ms"]


def test_bench_dumps_the_last_timed_step(tmp_path):
    """The run is seeded and every step moves the weights, so the dump tells how many steps ran before it was taken:
    3 timed steps behind 2 warm-up steps and 2 behind 3 (five steps either way) leave the same arrays, up to the order of
    fp32 sums (1e-5 of an array's scale, the bound the operators are held to); 2 behind 2 leave others: Adam's early
    updates move every weight by about the learning rate, 1e-4 against weights of 1e-2 to 1e-1, so the image and the
    gradients follow by more than 1e-5 of their scale (the loss, a mean over the image, need only differ at all)."""
    import numpy as np
    runs = {}
    for steps, warmup in ((3, 2), (2, 3), (2, 2)):
        path = tmp_path / ("%d_%d" % (steps, warmup))
        args = [a for a in SMALL]
        args[args.index("--steps") + 1], args[args.index("--warmup") + 1] = str(steps), str(warmup)
        d = _run(args + ["--dump-outputs", str(path)])
        assert d["steps"] == steps and d["warmup"] == warmup
        runs[steps, warmup] = _dumped(path)
    for name, a in runs[3, 2].items():
        scale = np.abs(a).max()
        same = np.abs(a - runs[2, 3][name]).max() / scale
        other = np.abs(a - runs[2, 2][name]).max() / scale
        print(name, "five steps vs five: %.3g, five vs four: %.3g of the scale" % (same, other))
        assert same <= 1e-5, name
        assert other > (0 if name == "loss" else 1e-5) and other > same, name


@pytest.mark.parametrize("workload", ["splat", "infer"])
def test_bench_dumps_of_the_other_workloads(workload, tmp_path):
    import numpy as np
    names = {"splat": ["d_logits", "d_radiance", "radiance"], "infer": ["radiance"]}[workload]
    d = _run(["--workload", workload] + SMALL + ["--dump-outputs", str(tmp_path)])
    out = _dumped(tmp_path)
    assert d["value"] > 0 and sorted(out) == names
    for a in out.values():
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.abs(a).max() > 0
    assert out["radiance"].ndim == 4 and out["radiance"].shape[:2] == (1, 3)


@pytest.mark.parametrize("workload", ["model", "splat", "infer"])
def test_bench_starts_its_own_ranks(workload, tmp_path):
    d = _run(["--gpus", "2", "--workload", workload] + SMALL + FULL + ["--no-stages", "--dump-outputs", str(tmp_path)],
             env={"SBMC_BENCH_BACKEND": "gloo", "SBMC_BENCH_SINGLE_DEVICE": "1"})
    # rank 0's arrays; the sharded training step hands back its loss, not the image
    assert sorted(_dumped(tmp_path)) == {"model": ["grads", "loss"], "splat": ["d_logits", "d_radiance", "radiance"],
                                         "infer": ["radiance"]}[workload]
    assert d["n_gpus"] == 2 and d["world_size"] == 2 and d["backend"] == "gloo"
    assert d["value"] > 0 and d["scaling"] == "strong"
    assert "H-slabs x2" in d["config"]["parallelism"]
    if workload in ("model", "infer"):
        # the per-rank split of the sharded step: neighbour exchanges, exposed all-reduce, the rest
        assert [r["rank"] for r in d["per_rank"]] == [0, 1]
        for r in d["per_rank"]:
            assert r["step_ms"] > 0 and r["exchanges"] > 0 and r["exchange_ms"] >= 0
            assert abs(r["compute_ms"] + r["exchange_ms"] + r["all_reduce_exposed_ms"] - r["step_ms"]) < 1e-2
        assert d["whole_step_tflops"] > 0 and "unet_layout" in d
        for r in d["per_rank"]:
            assert r["transport"] in ("ipc", "p2p")
    if workload == "model":
        # the first thing N ranks do is a correctness check against rank 0's single-GPU forward of the whole frame
        v = d["validation"]
        assert v["rel_diff"] is not None and v["rel_diff"] <= 1e-5, v
        assert d["transport"] in ("ipc", "p2p") and d["rccl_ranks"] == 2
