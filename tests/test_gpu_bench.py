"""GPU tests of bench.py's plain run and --dump-outputs, in-process (bench.main with its own
argv) at sizes of a few hundred thousand keys.

  * a plain run's line carries the headline fields and nothing of what --full adds;
  * --steps sets the number of timed steps: the dumped output is the sort of the LAST timed
    step's input (step warmup + steps - 1 of the seeded splitmix64 stream), so one step more or
    fewer gives another array;
  * the dump equals the oracle's sort of that input (keys, and for a pair config the stable
    permutation), in float64, identically from run to run;
  * an output larger than bench.DUMP_SAMPLE is written at bench.dump_sample_index's positions.
"""
import json
import sys

import numpy as np
import pytest

import bench
import oracle

pytestmark = pytest.mark.gpu


def _run(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", *argv])
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _expected_keys(config, n, step):
    cid, _, kb, _, _, _ = bench.CONFIGS[config]
    return oracle.splitmix_keys(n, kb, bench.config_seed(cid), first=step * n)


def test_plain_line_and_dump_u32(gpu, monkeypatch, capsys, tmp_path):
    n, steps, warmup = 300_007, 3, 2
    d1, d2 = tmp_path / "a", tmp_path / "b"
    out = _run(monkeypatch, capsys, "--config", "c2", "--n", str(n), "--steps", str(steps),
               "--warmup", str(warmup), "--dump-outputs", str(d1))
    assert out["metric"] == bench.METRIC and out["unit"] == "Gkeys/s"
    assert out["higher_is_better"] is True and out["dtype"] == "u32"
    assert (out["steps"], out["warmup"]) == (steps, warmup)
    assert out["ms_per_step"] > 0
    # value = keys x steps / wall time, ms_per_step = wall time / steps (both rounded)
    assert out["value"] == pytest.approx(n / (out["ms_per_step"] * 1e-3) / 1e9, rel=0.02, abs=2e-3)
    assert out["check"]["inversions_last_step"] == 0
    for k in ("roofline", "moved_roofline", "phases_ms", "cpu_baseline", "traffic_pmc",
              "north_star", "reference_input"):
        assert k not in out

    got = np.load(d1 / "keys.npy")
    assert got.dtype == np.float64 and got.shape == (n,)
    want = np.sort(_expected_keys("c2", n, warmup + steps - 1))
    assert np.array_equal(got, want.astype(np.float64))
    assert sorted(p.name for p in d1.iterdir()) == ["keys.npy"]

    # the same arguments: the same output; one timed step fewer: the previous step's input
    _run(monkeypatch, capsys, "--config", "c2", "--n", str(n), "--steps", str(steps),
         "--warmup", str(warmup), "--dump-outputs", str(d2))
    assert np.array_equal(np.load(d2 / "keys.npy"), got)
    _run(monkeypatch, capsys, "--config", "c2", "--n", str(n), "--steps", str(steps - 1),
         "--warmup", str(warmup), "--dump-outputs", str(d2))
    prev = np.sort(_expected_keys("c2", n, warmup + steps - 2))
    assert np.array_equal(np.load(d2 / "keys.npy"), prev.astype(np.float64))


def test_dump_pairs_and_u64(gpu, monkeypatch, capsys, tmp_path):
    n = 200_003
    _run(monkeypatch, capsys, "--config", "c3", "--n", str(n), "--steps", "1", "--warmup", "1",
         "--dump-outputs", str(tmp_path / "c3"))
    keys = _expected_keys("c3", n, 1)
    perm = oracle.stable_argsort(keys)
    assert np.array_equal(np.load(tmp_path / "c3" / "keys.npy"), keys[perm].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "c3" / "vals.npy"), perm.astype(np.float64))

    out = _run(monkeypatch, capsys, "--config", "c5", "--n", str(n), "--steps", "1", "--warmup", "0",
               "--dump-outputs", str(tmp_path / "c5"))
    assert out["dtype"] == "u64"
    want = np.sort(_expected_keys("c5", n, 0))
    hi, lo = np.load(tmp_path / "c5" / "keys_hi32.npy"), np.load(tmp_path / "c5" / "keys_lo32.npy")
    assert hi.dtype == lo.dtype == np.float64
    assert np.array_equal(hi, (want >> np.uint64(32)).astype(np.float64))
    assert np.array_equal(lo, (want & np.uint64(0xFFFFFFFF)).astype(np.float64))


def test_dump_is_sampled_beyond_the_limit(gpu, monkeypatch, capsys, tmp_path):
    n = bench.DUMP_SAMPLE + 12_345
    _run(monkeypatch, capsys, "--config", "ns", "--n", str(n), "--steps", "1", "--warmup", "0",
         "--dump-outputs", str(tmp_path))
    got = np.load(tmp_path / "keys.npy")
    assert got.shape == (bench.DUMP_SAMPLE,)
    want = np.sort(_expected_keys("ns", n, 0))[bench.dump_sample_index(n)]
    assert np.array_equal(got, want.astype(np.float64))
