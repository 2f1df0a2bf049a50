"""The driver parses bench.py's last stdout line: it must stay valid JSON of bounded size
(round 5's 22.9 KB line went unparsed; bench.py LINE_MAX_BYTES), keep the contract's keys
(value, roofline, cpu_baseline) and every record's numbers, and be the last line printed."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FULL = os.path.join(ROOT, "tests", "fixtures", "bench_line_r05_full.json")


def _full():
    with open(FULL) as fh:
        return json.load(fh)


def test_compact_line_of_round5_full_line_is_bounded_and_complete():
    import bench
    full = _full()
    assert len(json.dumps(full)) > 20000          # the line the driver could not parse
    line = bench.compact_line(full)
    s = json.dumps(line)
    assert len(s) <= bench.LINE_MAX_BYTES
    assert json.loads(s) == line
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config"):
        assert line[k] == full[k] if k != "config" else line[k]["workload"] == full[k]["workload"]
    rl = line["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert rl[k] == full["roofline"][k]
    assert rl["valu_profile"]["valu_busy_frac"] == full["roofline"]["valu"]["valu_busy_frac"]
    cpu = line["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind"):
        assert cpu[k] == full["cpu_baseline"][k]
    assert cpu["sample"].startswith("8 block rows")
    assert line["section4_region"]["value"] == full["section4_region"]["value"]
    assert set(line["records"]) == set(full["records"])
    for name, r in full["records"].items():
        c = line["records"][name]
        assert c["ms_per_step"] == r["ms_per_step"] and c["value"] == r["value"]
        assert c["parity"]["bit_exact"] is True
        if "roofline" in r:
            assert c["roofline"]["frac"] == r["roofline"]["frac"]
            assert c["roofline"]["traffic"] == r["roofline"]["traffic"]
    assert "algorithmic_bytes" in line["defs"] and "valu_profile" in line["defs"]


def test_compact_line_stays_bounded_when_every_record_fails():
    """Error entries and wait-timeout records must not push the line past the bound."""
    import bench
    full = _full()
    for name in list(full["records"]):
        full["records"][name] = {"error": "RuntimeError: " + "x" * 300}
    for i in range(20):
        full["records"][f"extra{i}"] = {"value": 1.0, "ms_per_step": 1.0, "workload": "w" * 200,
                                        "wait_health": {"timeouts": 3, "records": [{"task": 35, "frame": 0}] * 4}}
    line = bench.compact_line(full)
    assert len(json.dumps(line)) <= bench.LINE_MAX_BYTES


def test_cpu_plumbing_line_is_last_bounded_json(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    detail = tmp_path / "detail.json"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-plumbing", "--frames", "2",
                          "--steps", "1", "--warmup", "0", "--detail-out", str(detail)],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    last = out.stdout.rstrip("\n").splitlines()[-1]
    import bench
    assert len(last.encode()) <= bench.LINE_MAX_BYTES
    line = json.loads(last)
    assert line["value"] > 0 and line["n_gpus"] == 1 and "defs" in line
    assert json.loads(detail.read_text())["value"] == line["value"]


class _StubEngine:
    class wait_health:
        @staticmethod
        def as_dict():
            return {"timeouts": 0}

    def check_run(self):
        pass

    def pipelined_ok(self, *a, **kw):
        return True


class _StubCodec:
    def engine(self):
        return _StubEngine()


def _main_with_stubbed_legs(monkeypatch, capsys, argv):
    """bench.main() at N = 1 with the encode and every secondary leg replaced by a recorder:
    returns (the printed line, the names of the legs that ran, the number of steps run)."""
    import torch
    import bench
    calls, steps = [], []

    def leg(name, result):
        def fn(*a, **kw):
            calls.append(name)
            return result
        monkeypatch.setattr(bench, name, fn)

    def run_single(cfg, args, dev, parity):
        def step():
            steps.append(1)
            return {"symbols": [], "sse": torch.zeros(cfg["frames"], dtype=torch.int64)}
        return _StubCodec(), None, [], step

    monkeypatch.setattr(bench, "run_single", run_single)
    monkeypatch.setattr(bench, "dist_setup", lambda backend="nccl": (1, 0, 0))
    monkeypatch.setattr(bench, "sync", lambda dev: None)
    leg("kernel_roofline", {"stub": True})
    leg("roofline_of", {"bound": "hbm", "frac": 0.1})
    leg("parity_of", {"bit_exact": True, "psnr_delta_db": 0.0})
    leg("dense_fallback_of", {"frac": 0.0})
    leg("pcie_inclusive", {"error": "stub"})
    leg("record_single", {"value": 1.0, "ms_per_step": 1.0})
    leg("record_gops_in_flight", {"value": 1.0, "ms_per_step": 1.0})
    leg("cpu_baseline", {"value": 1.0, "unit": "Mpx/s", "cores": 1, "kind": "port"})
    bench.main(argv + ["--detail-out", ""])
    return json.loads(capsys.readouterr().out.rstrip("\n").splitlines()[-1]), calls, len(steps)


HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")


def test_plain_run_times_the_steps_and_runs_no_secondary_leg(monkeypatch, capsys):
    """`bench.py --gpus 1 --steps N --warmup W` runs W + N steps and none of the roofline, parity,
    dense-fallback, PCIe, record or CPU-baseline legs; its line holds the headline fields, the
    secondary ones are null or absent."""
    line, calls, nsteps = _main_with_stubbed_legs(monkeypatch, capsys, ["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert calls == []
    assert nsteps == 6
    for k in HEADLINE_KEYS:
        assert line[k] is not None
    assert line["steps"] == 4 and line["warmup"] == 2 and line["unit"] == "Mpx/s" and line["dtype"] == "u8"
    assert line["roofline"] is None and line["parity"] is None and line["cpu_baseline"] is None
    for k in ("records", "section4_region", "dense_frac", "gpu_over_cpu", "psnr_mean_db"):
        assert line.get(k) is None


def test_full_run_runs_every_secondary_leg_after_the_same_steps(monkeypatch, capsys):
    """--full: the same W + N headline steps, then every leg that a plain run leaves out."""
    line, calls, nsteps = _main_with_stubbed_legs(monkeypatch, capsys,
                                                  ["--gpus", "1", "--steps", "4", "--warmup", "2", "--full"])
    assert nsteps == 6         # the stubbed legs run no step of their own
    assert set(calls) == {"kernel_roofline", "roofline_of", "parity_of", "dense_fallback_of", "pcie_inclusive",
                          "record_single", "record_gops_in_flight", "cpu_baseline"}
    for k in HEADLINE_KEYS:
        assert line[k] is not None
    assert line["roofline"]["frac"] == 0.1 and line["parity"]["bit_exact"] is True
    assert line["cpu_baseline"]["value"] == 1.0 and line["dense_frac"] == 0.0
    assert set(line["records"]) == {"1080p", "1080p_x2gop", "4k_x2gop", "4k_lowtex", "4k_noise", "4k_vbs", "4k_rc2pass"}


def test_dump_sample_is_the_seeded_index_set_of_the_frame_order_concatenation(tmp_path, monkeypatch):
    """An array above DUMP_SAMPLE elements is written as the elements of the frames' concatenation
    at the sorted indices from default_rng(crc32(name)); a smaller one whole; frames of different
    shapes (I / P motion vectors) and a frame no index falls into are handled."""
    import zlib
    from types import SimpleNamespace
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 50)
    g = torch.Generator().manual_seed(3)
    shapes = [(7, 4), (9, 4, 3), (1, 4, 3), (11, 4, 3)]
    syms = [SimpleNamespace(split=torch.randint(0, 2, (s[0],), generator=g, dtype=torch.uint8),
                            mv=torch.randint(-16, 17, s, generator=g, dtype=torch.int16),
                            qtc=torch.randint(-99, 99, (s[0], 16), generator=g, dtype=torch.int16),
                            tokens=torch.zeros(s[0], dtype=torch.int32), mae_num=torch.full((s[0],), 2 ** 30, dtype=torch.int32),
                            recon=None, sse=torch.zeros(s[0], dtype=torch.int32)) for s in shapes]
    wrote = bench.dump_outputs({"symbols": syms, "sse": torch.arange(4) * 2 ** 40}, str(tmp_path))
    for name in ("mv", "qtc"):
        whole = np.concatenate([getattr(s, name).numpy().reshape(-1) for s in syms])
        idx = np.sort(np.random.default_rng(zlib.crc32(name.encode())).integers(0, whole.size, size=50))
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, whole[idx].astype(np.float32))
        assert wrote[name] == {"elements": 50, "of": whole.size}
    assert np.array_equal(np.load(tmp_path / "split.npy"), np.concatenate([s.split.numpy() for s in syms]))
    assert np.load(tmp_path / "mae_num.npy").dtype == np.float64 and np.all(np.load(tmp_path / "mae_num.npy") == 2 ** 30)
    assert np.array_equal(np.load(tmp_path / "sse.npy"), np.arange(4) * 2.0 ** 40)
    assert not (tmp_path / "recon.npy").exists()


def test_dump_outputs_writes_the_last_steps_arrays(tmp_path):
    """--dump-outputs DIR: every array of the timed step's result as DIR/<name>.npy in float32 /
    float64, a larger array cut to the same DUMP_SAMPLE positions on every run, under 64 MB in all;
    --steps sets the number of timed steps the line reports, with their ms_per_step."""
    import numpy as np
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-plumbing", "--frames", "2",
                              "--steps", "2", "--warmup", "0", "--detail-out", "", "--dump-outputs", str(d)],
                             env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads(out.stdout.rstrip("\n").splitlines()[-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0
    names = sorted(p.name for p in dirs[0].iterdir())
    assert names == sorted(n + ".npy" for n in ("split", "mv", "qtc", "tokens", "mae_num", "recon", "block_sse", "sse"))
    total = 0
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype in (np.float32, np.float64) and a.ndim == 1 and a.size <= bench.DUMP_SAMPLE
        assert np.array_equal(a, b)
        total += a.nbytes
    assert total <= 64 << 20
    # the stand-in engine's reconstruction is the source frames (128-padded): the sample is of real values
    assert np.load(dirs[0] / "recon.npy").size == bench.DUMP_SAMPLE and np.load(dirs[0] / "recon.npy").std() > 0
    assert np.load(dirs[0] / "sse.npy").shape == (2,)
