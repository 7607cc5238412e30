"""bench.py's host-side pieces that need no GPU: the averaging ceiling from the committed counters and probe prices, the
self-launch of N ranks from a plain command (here: that a failure of the ranks reaches the caller as a non-zero exit
code and no line), and the refusal of a packed grid on an engine without a device."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_averaging_ceiling_is_built_from_the_committed_counters():
    import bench
    nvv = 512 ** 3 * 72
    for form in ("u8", "f32"):
        ceiling_ms, lane_ops, ns_vv, mix, stream_ms = bench.valu_ceiling(form, float(nvv))
        d = json.load(open(os.path.join(ROOT, bench.AVG_COUNTERS[form])))
        k = [v for n, v in d["kernels"].items() if n.startswith("average_brick_kernel")][0]
        assert abs(lane_ops - k["SQ_INSTS_VALU"] * 64 / nvv) < 1e-9 and 30 < lane_ops < 40
        assert abs(sum(mix.values()) - lane_ops) < 1e-6 and mix["other"] >= 0
        # a lower bound of the time the mix needs: cheaper than the measured launch, dearer than the cheapest class flat;
        # the rate a stream of the projection's own mix reaches lies between the two
        assert ceiling_ms < stream_ms < k["mean_us"] / 1e3
        assert ceiling_ms > lane_ops / 64 * bench.VALU_COST_NS["other"] * nvv / bench.SIMDS * 1e-6
        half = bench.valu_ceiling(form, nvv / 2.0)[0]
        assert abs(half * 2 - ceiling_ms) < 1e-9
    # the prices are the probe's: every class the model names stands in the committed table
    table = open(os.path.join(ROOT, bench.VALU_PROBE)).read()
    for name in ("v_add_f32", "v_mul_f32", "v_fma_f32", "v_rcp_f32", "v_cvt_i32_f32", "v_mad_u32_u24", "four voxels"):
        assert name in table


@pytest.mark.timeout(300)
def test_a_failure_of_the_self_launched_ranks_reaches_the_caller():
    """`python3 bench.py --gpus 2` from a plain shell starts its ranks as children; here they cannot get a device (the
    CPU suite runs without one, or with HIP_VISIBLE_DEVICES emptied), so the parent must exit non-zero and print no line."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--n", "64", "--views", "8", "--dist-backend", "gloo", "--share-device"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280)
    assert r.returncode != 0
    assert r.stdout.decode().strip() == ""


def test_a_packed_grid_needs_the_hip_engine():
    """`all_gather(unpack=False)` hands out a PackedGrid, which only HIP kernels read; on an engine without
    a device (the CPU rehearsal's stand-in) that is a clear error, not a torch failure three calls later."""
    from plant3dvision_amd.sharded import ShardedBackprojection
    from tests.helpers import OracleEngine, scene
    shape, origin, vs, views = scene((6, 16, 64), 3, "plant")
    sb = ShardedBackprojection(shape, origin, vs, rank=0, world_size=1, engine_factory=OracleEngine)
    for K, R, t, m in views:
        sb.process_view(K, R, t, m)
    for comp in ("2bit", "1bit"):
        with pytest.raises(ValueError, match="HIP engine"):
            sb.all_gather(compress=comp, unpack=False)
    with pytest.raises(ValueError, match="overlap"):
        sb.all_gather(compress="2bit", overlap=True)
    sb.close()


def test_dump_outputs_writes_seeded_float_arrays_of_the_labels(tmp_path, monkeypatch):
    """--dump-outputs: float32 / float64 only; a volume up to DUMP_SAMPLE voxels whole, a larger one as the same seeded
    sample in every run; the histograms count every voxel."""
    import bench
    rng = np.random.default_rng(7)
    small = rng.integers(-1, 2, (4, 6, 8)).astype(np.int32)
    assert bench.dump_outputs(str(tmp_path / "a"), small) == ["labels_histogram", "labels_per_plane", "labels_sample"]
    got = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("labels_histogram", "labels_per_plane", "labels_sample")}
    assert got["labels_sample"].dtype == np.float32 and np.array_equal(got["labels_sample"], small.ravel())
    assert got["labels_histogram"].dtype == np.float64 and got["labels_per_plane"].dtype == np.float64
    assert got["labels_histogram"].tolist() == [float((small == v).sum()) for v in (-1, 0, 1)]
    assert got["labels_per_plane"].shape == (4, 3) and got["labels_per_plane"][2].tolist() == [float((small[2] == v).sum()) for v in (-1, 0, 1)]
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    big = rng.integers(-1, 2, (10, 20, 30)).astype(np.int32)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big)
    s1, s2 = (np.load(str(tmp_path / d / "labels_sample.npy")) for d in ("b", "c"))
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, big.size, 100))
    assert s1.shape == (100,) and np.array_equal(s1, s2) and np.array_equal(s1, big.ravel()[idx])
    assert np.load(str(tmp_path / "b" / "labels_histogram.npy")).sum() == big.size


def test_a_plain_run_is_the_default(monkeypatch):
    """The legs beside the headline need --full; --dump-outputs is off unless given."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs == "" and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"
