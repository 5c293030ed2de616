"""bench.py --dump-outputs without a device: the fields written, their dtype, the seeded sample of a large field (the
same indices from run to run, under 64 MB for the metric's size) and the refusal of a sharded run."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


class FakeField:
    def __init__(self, a):
        self.a = a

    def __getitem__(self, layout):
        assert layout == "c"
        return self.a


METRIC_SHAPES = dict(p=(512, 512, 256), b=(512, 512, 256), u=(3, 512, 512, 256), tau_b1=(512, 512), tau_b2=(512, 512),
                     tau_u1=(3, 512, 512), tau_u2=(3, 512, 512))      # the state fields of the benchmark's problem


def test_small_fields_are_written_whole(tmp_path):
    rng = np.random.default_rng(1)
    fields = dict(b=FakeField(rng.standard_normal((4, 6, 8))), u=FakeField(rng.standard_normal((3, 4, 6, 8))))
    written = bench.dump_outputs(fields, str(tmp_path))
    assert written == dict(b=192, u=576)
    for name, f in fields.items():
        got = np.load(os.path.join(tmp_path, name + ".npy"))
        assert got.dtype == np.float64
        assert np.array_equal(got, f.a.ravel())


def test_metric_sized_dump_stays_under_64_MB():
    assert sum(8 * min(int(np.prod(sh)), bench.DUMP_SAMPLE) for sh in METRIC_SHAPES.values()) <= 64 << 20


def test_large_fields_are_sampled_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    rng = np.random.default_rng(2)
    fields = dict(b=FakeField(rng.standard_normal((16, 16, 8))), u=FakeField(rng.standard_normal((3, 16, 16, 8))),
                  tau_b1=FakeField(rng.standard_normal((16, 16))))
    bench.dump_outputs(fields, str(tmp_path / "a"))
    bench.dump_outputs(fields, str(tmp_path / "b"))
    for name in fields:
        a = np.load(os.path.join(tmp_path, "a", name + ".npy"))
        b = np.load(os.path.join(tmp_path, "b", name + ".npy"))
        assert a.dtype == np.float64 and np.array_equal(a, b), name
        assert a.size == min(fields[name].a.size, 1000), name
    # the sample is the field at sorted, distinct, seeded flat indices
    u = fields["u"].a
    idx = np.sort(np.random.default_rng(0).choice(u.size, 1000, replace=False))
    assert np.unique(idx).size == 1000
    assert np.array_equal(np.load(os.path.join(tmp_path, "a", "u.npy")), u.ravel()[idx])


def test_dump_outputs_refuses_a_sharded_run(tmp_path):
    env = dict(os.environ, BENCH_DRY_LAUNCH="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "--gpus 1" in r.stderr
    assert not os.listdir(tmp_path)
