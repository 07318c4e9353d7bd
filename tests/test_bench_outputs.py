"""bench.py's plain run, --full and --dump-outputs.

A plain run prints the headline line only; --full adds the secondary measurements and
checks.  --dump-outputs DIR writes what the last timed step computed as float32/float64
.npy files of at most 64 MB: the GPU test compares them with the CPU oracle's run of the
same instances.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from snapcheck import ROOT, TEST_DATA

sys.path.insert(0, ROOT)
import bench  # noqa: E402

BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("parity", "parity_ref", "checks", "fresh_run", "collect", "replay", "roofline", "cpu_baseline")


def test_full_and_dump_outputs_are_off_by_default():
    args = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert args.full is False and args.dump_outputs is None
    assert (args.steps, args.warmup) == (7, 2)
    args = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert args.full is True and args.dump_outputs == "out"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]])
def test_step_counts_that_cannot_be_timed_are_refused(argv):
    with pytest.raises(SystemExit) as e:
        bench.parse_args(argv)
    assert e.value.code not in (0, None)


def test_save_outputs_refuses_more_than_the_limit(tmp_path):
    big = {"a": np.zeros(bench.DUMP_LIMIT // 4 + 1, dtype=np.float32)}
    with pytest.raises(SystemExit):
        bench.save_outputs(str(tmp_path), big, 0)
    assert not list(tmp_path.iterdir())
    bench.save_outputs(str(tmp_path), {"a": np.arange(5, dtype=np.float64)}, 0)
    assert np.array_equal(np.load(tmp_path / "a.npy"), np.arange(5.0))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_the_timed_path_computed(tmp_path):
    n = 4096
    r = subprocess.run([sys.executable, "-u", BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--instances", str(n), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["full"] is False and not [k for k in FULL_ONLY if k in d]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["metric"] == "delivered packets/sec (whole node)" and d["unit"] == "packets/s"
    assert d["higher_is_better"] is True and d["dtype"] == "int32"
    assert d["value"] == pytest.approx(d["packets_per_step"] / (d["ms_per_step"] * 1e-3), rel=1e-9)

    out = {p.name[:-4]: np.load(p) for p in tmp_path.iterdir()}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 << 20

    top, events = (open(os.path.join(TEST_DATA, f)).read() for f in bench.CONFIGS["c3"][:2])
    _, st, ticks, cnt, hashes = O.run_batch_prepared(top, events, n, threads=8)
    ok = st == 0
    assert ok.any() and not ok.all()          # both outcomes are in the batch
    assert np.array_equal(out["status"], st)
    assert np.array_equal(out["time"][ok], ticks[ok])
    h = out["instance_hash"].astype(np.uint64)
    assert np.array_equal(((h[:, 0] << np.uint64(32)) | h[:, 1])[ok], hashes[ok].astype(np.uint64))
    assert d["status"] == {"ok": int(ok.sum()), "fatal": int((~ok).sum()), "other": 0}
    assert d["packets_per_step"] == int((cnt[ok, 2] + cnt[ok, 3]).sum())

    lo, hi = (int(v) for v in out["sample_range"])
    assert 0 <= lo < hi <= n
    checked = 0
    for i in range(lo, min(hi, lo + 48)):
        if not ok[i]:
            continue
        ref = O.OracleSim()
        ref.seed_go(O.REFERENCE_SEED + i)
        ref.read_topology(os.path.join(TEST_DATA, bench.CONFIGS["c3"][0]))
        ref.read_events(os.path.join(TEST_DATA, bench.CONFIGS["c3"][1]))
        ids = sorted(ref.node_ids())          # the engine's rank order (getSortedKeys)
        final = ref.node_tokens()
        assert out["final_tokens"][i - lo].tolist() == [final[k] for k in ids]
        for sid in range(5):
            want = ref.collect(sid)
            assert out[f"snap{sid}_complete"][i - lo] == 1
            assert out[f"snap{sid}_tokens"][i - lo].tolist() == [want.tokens[k] for k in ids]
            ch = (out[f"snap{sid}_offsets"].size - 1) // (hi - lo)
            a, b = (int(out[f"snap{sid}_offsets"][j * ch]) for j in (i - lo, i - lo + 1))
            assert sorted(out[f"snap{sid}_messages"][a:b].tolist()) == sorted(m[2] for m in want.messages)
        checked += 1
    assert checked
