"""bench.py's --full and --dump-outputs on the CPU (the device call replaced by the oracle, as in
tests/test_multiproc.py): a run without --full starts none of the side legs, --full starts them, and
--dump-outputs writes the last timed step's arrays, the same from run to run."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402
import oracle_py as orc  # noqa: E402
from recordio import generate  # noqa: E402
from test_multiproc import OracleBackend, _bench_cli  # noqa: E402

SIZES = (150, 2048)


def _main_with_oracle(monkeypatch, capsys, argv, backend=OracleBackend):
    """bench.main(argv) in this process on the oracle backend; returns (line, legs that ran)."""
    import functools

    ran = []
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(bench, "make_device", lambda local: torch.device("cpu"))
    monkeypatch.setattr(bench, "make_backend", lambda local, device, own=False: backend())
    monkeypatch.setattr(bench, "run_decode", functools.partial(bench.run_decode, sizes=SIZES))
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **k: ran.append("cpu_baseline") or {"oracle_match": True})
    monkeypatch.setattr(bench, "e2e_rate", lambda *a, **k: ran.append("e2e") or {})
    monkeypatch.setattr(bench, "live_traffic", lambda *a, **k: ran.append("live_traffic") or {"error": "stub"})
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    bench.main(argv)
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return lines[0], ran


def test_plain_run_starts_no_side_leg(monkeypatch, capsys):
    line, ran = _main_with_oracle(monkeypatch, capsys, ["--gpus", "1", "--steps", "4", "--warmup", "1"])
    assert ran == []
    assert "cpu_baseline" not in line and "e2e" not in line and line["roofline"]["traffic"] is None
    assert line["verified"] is None and line["reproducible"] is True
    assert line["metric"] == bench.METRIC and line["unit"] == "GiB/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u8" and line["steps"] == 4 and line["ms_per_step"] > 0 and line["value"] > 0


def test_full_run_starts_every_side_leg(monkeypatch, capsys):
    line, ran = _main_with_oracle(monkeypatch, capsys, ["--gpus", "1", "--steps", "2", "--warmup", "1", "--full"])
    assert ran == ["live_traffic", "cpu_baseline", "e2e"]
    assert line["verified"] is True and "cpu_baseline" in line and "e2e" in line
    # the switches that pick among the legs still do under --full
    line, ran = _main_with_oracle(monkeypatch, capsys, ["--steps", "2", "--warmup", "1", "--full", "--no-e2e",
                                                        "--traffic", "none"])
    assert ran == ["cpu_baseline"] and "e2e" not in line


def test_timed_steps_are_the_steps_asked_for(monkeypatch, capsys):
    made = []

    class Counting(OracleBackend):
        def __init__(self):
            super().__init__()
            made.append(self)

    _main_with_oracle(monkeypatch, capsys, ["--steps", "5", "--warmup", "2", "--config", "c2"], backend=Counting)
    # load + 2 warm-ups + exactly 5 timed + the 5 MALL-flushed steps of a file this small
    assert made[0].steps == 1 + 2 + 5 + 5


def test_dump_outputs_are_the_last_steps_arrays_and_repeat(tmp_path):
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        r = _bench_cli(["--gpus", "1", "--config", "c2", "--steps", "2", "--warmup", "1", "--dump-outputs", d])
        assert r.returncode == 0, r.stderr[-3000:]
        line = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")][0]
        assert line["dumped_outputs"]["written_of_total"]["out"] == [150 * 2048, 150 * 2048]
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1])) == ["flags.npy", "out.npy", "out_block_sums.npy", "out_off.npy",
                                                    "rec_off.npy"]
    got = {n[:-4]: np.load(os.path.join(dirs[0], n)) for n in names}
    for n in names:
        assert np.array_equal(got[n[:-4]], np.load(os.path.join(dirs[1], n))), n
    want = orc.file_reader_decode_arrays(generate(*SIZES, 2, kind=1, seed=bench.rank_seed(0)))
    assert got["out"].dtype == np.float32 and got["flags"].dtype == np.float32
    assert got["out_off"].dtype == np.float64 and got["rec_off"].dtype == np.float64
    for k in ("out", "out_off", "rec_off", "flags"):
        assert np.array_equal(got[k], np.asarray(want[k]).astype(got[k].dtype)), k
    sums = got["out_block_sums"]
    assert sums.shape == (150 * 2048 // 4096 + 1,) and sums.sum() == want["out"].astype(np.int64).sum()
    assert sums[0] == want["out"][:4096].astype(np.int64).sum() and sums[-1] == 0


def test_dump_outputs_samples_what_exceeds_its_share(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    big = torch.arange(100_000, dtype=torch.int64) * 3
    small = np.arange(7, dtype=np.uint8)
    w = bench.dump_outputs(str(tmp_path), {"big": big, "small": small})
    assert w == {"big": [250, 100_000], "small": [7, 7]}  # 2000 bytes each: 250 float64, 7 float32 written whole
    b = np.load(tmp_path / "big.npy")
    assert b.dtype == np.float64 and b.shape == (250,) and np.all(np.diff(b) >= 0) and np.all(b % 3 == 0)
    assert np.array_equal(np.load(tmp_path / "small.npy"), small.astype(np.float32))
    # the sample's places depend on the seed and the array's length alone
    bench.dump_outputs(str(tmp_path / "again"), {"big": big.clone(), "small": small})
    assert np.array_equal(np.load(tmp_path / "again" / "big.npy"), b)
    assert sum(os.path.getsize(tmp_path / f) for f in ("big.npy", "small.npy")) <= 4000 + 2 * 128


@pytest.mark.gpu
def test_dump_outputs_of_the_device_decode_equal_the_oracle(tmp_path, monkeypatch):
    """bench.run_decode on the device backend with --dump-outputs: offsets and flags whole, the arena as a sample
    taken on the device (a budget cut so that 3 MB of records exceed their share) plus its block sums, all equal
    to the oracle's decode of the same seeded file."""
    import argparse

    n_rec, rec_len = 3000, 1024
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 5 * 400_000)
    args = argparse.Namespace(config="c2", steps=2, warmup=1, no_cpu_baseline=True, no_e2e=True, traffic="none",
                              traffic_json=None, dump_outputs=str(tmp_path))
    line = bench.run_decode(args, 1, 0, bench.make_backend(0, bench.make_device(0)), sizes=(n_rec, rec_len))
    want = orc.file_reader_decode_arrays(generate(n_rec, rec_len, 2, kind=1, seed=bench.rank_seed(0)))
    nb = int(want["out"].shape[0])
    assert line["dumped_outputs"]["written_of_total"]["out"] == [100_000, nb]
    got = {n[:-4]: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    for k in ("out_off", "rec_off", "flags"):
        assert np.array_equal(got[k], np.asarray(want[k]).astype(got[k].dtype)), k
    idx = np.sort(np.random.default_rng([bench.DUMP_SEED, nb]).integers(0, nb, 100_000))
    assert got["out"].dtype == np.float32 and np.array_equal(got["out"], want["out"][idx].astype(np.float32))
    m = nb // 4096 * 4096
    sums = np.append(want["out"][:m].reshape(-1, 4096).sum(axis=1, dtype=np.int64), want["out"][m:].sum(dtype=np.int64))
    assert np.array_equal(got["out_block_sums"], sums.astype(np.float64))


def test_dump_outputs_refused_where_a_line_keeps_no_arrays():
    r = _bench_cli(["--config", "wal", "--steps", "1", "--warmup", "0", "--dump-outputs", "unused"])
    assert r.returncode == 2 and "--dump-outputs" in r.stderr
