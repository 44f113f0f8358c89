"""bench.py's launcher: `python bench.py --gpus N` with no rank environment must start its own ranks, print ONE JSON
line last and hand back the ranks' status -- the driver's multi-GPU run cannot be allowed to die on the launch.  On a box without a
GPU the ranks run the rendezvous, the slab partition and the frame's collectives over gloo (a dry run, value null); the GPU variants
of this test are in tests/test_gpu_sharded.py."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env)


def have_gpu():
    import torch
    return torch.cuda.is_available()


def test_gpus_2_without_rank_environment_launches_itself():
    if have_gpu():
        import pytest
        pytest.skip("GPU box: covered by tests/test_gpu_sharded.py (oversubscribed / RCCL variants)")
    r = run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1"])
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = r.stdout.strip().splitlines()
    assert len([ln for ln in lines if ln.startswith('{"metric"')]) == 1 and lines[-1].startswith('{"metric"'), r.stdout[-800:]
    d = json.loads(lines[-1])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] is None and "dry_run" in d                       # no GPU here: nothing measured, and the line says so
    b = d["config"]["slab_bounds"]
    assert b[0] == 0 and b[-1] == 512 and len(b) == 3 and all(x % 8 == 0 for x in b) and b[1] > 256      # work-balanced: the near slab is the thick one


def test_a_failing_rank_fails_the_launcher():
    if have_gpu():
        import pytest
        pytest.skip("CPU variant")
    r = run_bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"DFUSION_BENCH_TEST_FAIL_RANK": "1"})
    assert r.returncode != 0
    assert not any(ln.startswith('{"metric"') for ln in r.stdout.splitlines())
    assert "fails on purpose" in r.stderr


def test_three_ranks_uniform_slabs_dry_run():
    if have_gpu():
        import pytest
        pytest.skip("CPU variant")
    r = run_bench(["--gpus", "3", "--steps", "1", "--warmup", "0", "--slabs", "uniform", "--config", "256"])
    assert r.returncode == 0, r.stderr[-1500:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["n_gpus"] == 3 and d["config"]["slab_bounds"] == [0, 88, 176, 256]


def test_dump_outputs_sample_and_budget(tmp_path):
    """--dump-outputs: the ray-cast images whole, the volume as tsdf / weight at seeded voxel indices that depend on the volume's size
    only, all float32, under the byte limit even at the 1024^3 config's image size."""
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    import bench
    bench.torch = torch
    g = torch.Generator().manual_seed(0)
    tsdf = (torch.rand((256, 256, 256), generator=g) * 2 - 1).half().view(torch.int16).to(torch.int32) & 0xFFFF    # lo16: a half in [-1, 1]
    vol = tsdf | (torch.randint(0, 1 << 15, (256, 256, 256), generator=g, dtype=torch.int32) << 16)                    # hi16: the weight
    for rows, cols in ((480, 640), (960, 1280)):
        pts, nrm = torch.randn((rows, cols, 4), generator=g), torch.randn((rows, cols, 4), generator=g)
        pts[0, 0] = float("nan")
        d = tmp_path / ("%d" % rows)
        info = bench.dump_outputs(str(d), pts, nrm, vol)
        files = {p.stem: np.load(p) for p in d.glob("*.npy")}
        assert set(files) == {"points", "normals", "hit_mask", "tsdf_sample", "weight_sample"} and all(a.dtype == np.float32 for a in files.values())
        assert all(np.isfinite(a).all() for a in files.values())
        assert sum(p.stat().st_size for p in d.glob("*.npy")) <= bench.DUMP_LIMIT_BYTES and info["bytes"] <= bench.DUMP_LIMIT_BYTES
        hit = np.ones((rows, cols), np.float32); hit[0, 0] = 0                          # (the NaN point: a missed ray, zeros in both images)
        want_p, want_n = pts.numpy().copy(), nrm.numpy().copy()
        want_p[0, 0] = 0; want_n[0, 0] = 0
        assert np.array_equal(files["hit_mask"], hit) and np.array_equal(files["points"], want_p) and np.array_equal(files["normals"], want_n)
        n = files["tsdf_sample"].size
        idx = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, vol.numel(), size=min(bench.DUMP_VOXELS, (bench.DUMP_LIMIT_BYTES - 9 * rows * cols * 4 - (1 << 16)) // 8)))
        assert n == idx.size == files["weight_sample"].size > 1 << 20
        raw = vol.reshape(-1).numpy().view(np.uint32)[idx]
        assert np.array_equal(files["weight_sample"], (raw >> 16).astype(np.float32))
        assert np.array_equal(files["tsdf_sample"], (raw & 0xFFFF).astype(np.uint16).view(np.float16).astype(np.float32))
    small = torch.arange(4096, dtype=torch.int32).reshape(16, 16, 16)                # smaller than the sample: every voxel, in order
    bench.dump_outputs(str(tmp_path / "small"), pts, nrm, small)
    assert np.array_equal(np.load(tmp_path / "small" / "weight_sample.npy"), np.zeros(4096, np.float32))
    assert np.load(tmp_path / "small" / "tsdf_sample.npy").size == 4096


def test_dump_outputs_refuses_what_it_cannot_dump(tmp_path):
    if have_gpu():
        import pytest
        pytest.skip("CPU variant")
    r = run_bench(["--gpus", "2", "--dump-outputs", str(tmp_path)])
    assert r.returncode != 0 and "--dump-outputs needs --gpus 1" in r.stderr
    r = run_bench(["--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path)])       # nothing computed on a box without a GPU
    assert r.returncode != 0 and "no GPU visible" in r.stderr and not any(tmp_path.iterdir())
