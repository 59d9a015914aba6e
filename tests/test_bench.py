"""bench.py's own contract: a plain run times the headline leg and prints its line, `--full` adds the other legs and the oracle
check, `--dump-outputs DIR` writes what the timed path returned in its last step as .npy files, the same on every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv, timeout=300):
    e = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_pads_rows_and_keeps_to_its_budget(tmp_path, monkeypatch):
    import bench
    results = [([5, 7, 9], [0, 3, 8]), ([], []), ([4], [2])]
    bench.dump_outputs(str(tmp_path / "d"), results, 6)
    got = _load(tmp_path / "d")
    assert sorted(got) == ["timestamps", "token_counts", "tokens", "utterance_ids"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["tokens"].tolist() == [[5, 7, 9], [-1, -1, -1], [4, -1, -1]]
    assert got["timestamps"].tolist() == [[0, 3, 8], [-1, -1, -1], [2, -1, -1]]
    assert got["token_counts"].tolist() == [3, 0, 1] and got["utterance_ids"].tolist() == [6, 7, 8]
    # past the budget the first utterances are kept
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 8 * (2 * 3 + 2))
    bench.dump_outputs(str(tmp_path / "e"), results, 6)
    got = _load(tmp_path / "e")
    assert got["tokens"].shape == (2, 3) and got["utterance_ids"].tolist() == [6, 7]


@pytest.mark.gpu
def test_plain_run_is_the_headline_leg_and_dumps_the_last_step(tmp_path):
    common = ["--preset", "zipformer2-tiny-test", "--batch", "3", "--seconds", "1.2", "--warmup", "1"]
    # 4 steps over 3 utterance sets: the last step decodes set 0, the one --dump-results holds
    d1, d2, res = str(tmp_path / "d1"), str(tmp_path / "d2"), str(tmp_path / "res.json")
    line = _bench(*common, "--steps", "4", "--dump-outputs", d1, "--dump-results", res)
    assert line["steps"] == 4 and line["ms_per_step"] > 0 and line["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in line, k
    for k in ("value_from_host_memory", "value_sync_get_results", "roofline", "cpu_baseline", "oracle_match", "secondary"):
        assert k not in line, k
    got = _load(d1)
    want = json.load(open(res))["results"]
    assert got["utterance_ids"].tolist() == [0, 1, 2] and got["token_counts"].tolist() == [len(t) for t, _ in want]
    for u, (t, s) in enumerate(want):
        assert got["tokens"][u, :len(t)].tolist() == t and got["timestamps"][u, :len(s)].tolist() == s
    assert sum(len(t) for t, _ in want) > 0
    # the same arguments give the same inputs, hence the same outputs
    _bench(*common, "--steps", "4", "--dump-outputs", d2)
    again = _load(d2)
    assert sorted(again) == sorted(got) and all(np.array_equal(got[k], again[k]) for k in got)


@pytest.mark.gpu
def test_full_run_adds_the_other_legs_and_the_oracle_check():
    line = _bench("--preset", "zipformer2-tiny-test", "--batch", "3", "--seconds", "1.2", "--steps", "2", "--warmup", "1", "--full")
    assert line["steps"] == 2 and "value_from_host_memory" in line and "value_sync_get_results" in line and "roofline" in line
    om = line["oracle_match"]
    assert om["streams"] > 0 and om["exact"] == om["streams"]
