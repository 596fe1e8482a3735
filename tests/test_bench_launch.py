"""bench.py launches its own ranks: ``--gpus N`` with no launcher around it
runs N processes (one per GPU; here gloo on CPU) and reports n_gpus = N; a
box with fewer visible GPUs fails fast instead of hanging in RCCL init."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, timeout=300):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args),
                          capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


def _json(stdout):
    lines = [l for l in stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, stdout  # rank 0 only
    return json.loads(lines[0])


def test_self_launch_two_ranks_cpu():
    r = _bench("--gpus", "2", "--device", "cpu", "--steps", "2", "--warmup", "1",
               "--batch", "1500")
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json(r.stdout)
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2+kvshard2"
    assert d["config"]["global_batch"] == 3000
    assert d["rank_ms_per_step_max"] >= d["rank_ms_per_step_min"] > 0
    w = d["wire_bytes_per_gpu_step"]
    assert w["c1"] > 0 and w["c2"] > 0 and w["c3"] > 0  # keys, pull reply, push crossed


def test_self_launch_linear_two_ranks_cpu():
    r = _bench("--gpus", "2", "--device", "cpu", "--steps", "2", "--warmup", "1",
               "--batch", "1500", "--model", "linear")
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json(r.stdout)
    assert d["n_gpus"] == 2 and d["vs_baseline"] is not None


def _load(d):
    import numpy as np
    assert all(f.endswith(".npy") for f in os.listdir(d))
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_cpu(tmp_path):
    """--dump-outputs: float .npy files from the timed learner and the probe,
    the same from run to run (seeded data), and --steps sets the timed steps."""
    import numpy as np
    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        r = _bench("--gpus", "1", "--device", "cpu", "--steps", "3", "--warmup", "1",
                   "--batch", "400", "--dim", "8", "--dump-outputs", str(d), *extra)
        assert r.returncode == 0, r.stderr[-3000:]
        j = _json(r.stdout)
        assert j["steps"] == 3 and j["ms_per_step"] > 0
        assert abs(j["value"] - 400 * 3 / (j["ms_per_step"] * 3 / 1000)) < 1e-6 * j["value"]
        dumps.append(_load(d))
    a, b = dumps
    assert sorted(a) == ["probe_V", "probe_cnt", "probe_found", "probe_pred", "probe_progress",
                         "probe_sq", "probe_w", "probe_z", "timed_cnt", "timed_found"]
    for f, x in a.items():
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), f
        assert np.array_equal(x, b[f]), f
    # one shard: every key of the minibatch is in the table, counted at least once
    for who in ("timed", "probe"):
        n = a[who + "_found"].shape[0]
        assert n > 0 and a[who + "_found"].all()
        assert a[who + "_cnt"].shape == (n,) and a[who + "_cnt"].min() >= 1
    assert a["probe_w"].shape == (n,) and a["probe_V"].shape == (n, 8)
    assert a["probe_V"].any() and a["probe_w"].any() and a["probe_pred"].shape == (400,)
    p = a["probe_progress"]  # the probe's 4 minibatches
    assert p[4] == 4 and p[5] == 4 * 400


def test_dump_outputs_two_ranks_cpu(tmp_path):
    """Every rank writes its own files; the probe and its prediction pass are
    collectives that only run with the option."""
    r = _bench("--gpus", "2", "--device", "cpu", "--steps", "2", "--warmup", "1",
               "--batch", "600", "--dim", "8", "--dump-outputs", str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    assert _json(r.stdout)["n_gpus"] == 2
    a = _load(tmp_path)
    assert len(a) == 20
    held = 0
    for rank in (0, 1):
        f = a["probe_found_rank%d" % rank]
        assert 0 < f.sum() < f.size  # this shard holds its share of the rank's keys
        assert a["probe_V_rank%d" % rank].shape == (f.size, 8)
        assert a["probe_pred_rank%d" % rank].shape == (600,)
        held += a["timed_found_rank%d" % rank].mean()
    assert 0.8 < held < 1.2  # two shards of about half the keys each


def test_dump_budget():
    """The sample is sized so that all files of all ranks stay under 64 MB."""
    import bench
    for dim in (0, 8, 64, 512, 4096):
        for ranks in (1, 2, 8, 64):
            rows = bench.dump_rows(dim, ranks)
            per_rank = 4 * (rows * (2 + 5 + dim) + 4 * rows) + 8 * 8
            assert rows >= 1 and (rows == 1 or ranks * per_rank <= 64 << 20), (dim, ranks)
    assert bench.dump_rows(64, 1) == 1 << 16


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1 << 20, 1000])
def test_model_sample_matches_checkpoint_gather_gpu(rows):
    """bench.model_sample on the device store (native find, vrow lookup, V
    slab rows wider than dim) against the checkpoint's gather of the whole
    table, key by key; a sample smaller than the key set is every k-th key."""
    import numpy as np
    import torch
    import bench
    from wormhole_amd import _native
    from wormhole_amd.config.schema import DifactoConfig, Embedding
    from wormhole_amd.data.synthetic import CRITEO_TB_CARD
    from wormhole_amd.kv.checkpoint import _gather, _numpy
    from wormhole_amd.models.difacto import DifactoLearner
    from wormhole_amd.parallel.comm import Comm

    dev = torch.device("cuda", 0)
    card = torch.tensor(CRITEO_TB_CARD, dtype=torch.int64, device=dev)
    lr = DifactoLearner(DifactoConfig(minibatch=3000, embedding=[Embedding(dim=5, threshold=2)]),
                        Comm(dev, init=False), dev, cap=1 << 18, vcap=1 << 14, seed=3)
    assert lr.store.vstride > 5  # the slab row is padded: [:, :dim] matters
    for s in range(3):
        keys, label, offset = _native.hip().synth_criteo(3000, 5, s, card)
        lr.process(keys, offset, None, label, 0, 0)
    lr.flush()
    got = {k: v.cpu().numpy() for k, v in bench.model_sample(lr.store, keys, rows).items()}
    uniq = np.unique(keys.cpu().numpy())
    if uniq.size > rows:
        uniq = uniq[::-(-uniq.size // rows)]
        assert uniq.size <= rows
    n = uniq.size
    snap = _numpy(_gather(lr.store, "difacto"))
    order = np.argsort(snap["keys"])
    at = order[np.searchsorted(snap["keys"][order], uniq)]
    assert np.array_equal(snap["keys"][at], uniq)  # the last minibatch was inserted
    assert got["found"].shape == (n,) and got["found"].all()
    for name in ("cnt", "w", "z", "sq"):
        assert np.array_equal(got[name], snap[name][at].astype(np.float32)), name
    vidx = np.cumsum(snap["has_v"]) - 1  # V rows of the snapshot follow its entries with one
    has = snap["has_v"][at]
    assert has.any() and not has.all()
    exp = np.zeros((n, 5), np.float32)
    exp[has] = snap["V"][vidx[at][has]]
    assert got["V"].shape == (n, 5) and np.array_equal(got["V"], exp)
    # a key the table does not hold
    miss = bench.model_sample(lr.store, torch.tensor([(1 << 62) + 12345], device=dev), rows)
    assert float(miss["found"].sum()) == 0 and float(miss["V"].abs().sum()) == 0


def test_too_few_gpus_fails_fast():
    import torch
    n = torch.cuda.device_count()
    r = _bench("--gpus", str(max(n + 1, 2)), "--steps", "1", "--warmup", "0", timeout=120)
    assert r.returncode == 2
    assert "visible" in r.stderr and "only %d device" % n in r.stderr
