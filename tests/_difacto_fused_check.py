"""Helper of test_difacto_fused_gpu.py: the minibatches of the fused-update
tests, the by-key model dump, and, run as a script in a fresh process started
with WH_DETERMINISTIC=1 (the mode is read once per process), the bit-for-bit
comparison of the native DiFacto step with and without the fused V update
(csrc/bind/fm_ops.cc fused_v; fm.hip k_bwd_v<G, true>). Hash localize
and ordered partials make the whole step repeatable there, and both variants
call the same kv_device.h adagrad4 with fixed roundings, so every key's cnt,
w, z, sq, V row and VG row must be the same bits. Prints OK.

The big minibatch (make_batch): ROWS rows of 6 ids -- one key in every row
(more than 64 x 64 occurrences: the chunk emitter's second expansion round),
one key of exactly 64 occurrences (the largest single chunk) and one of 65
(the smallest multi-chunk key), 300 keys of 1-4 occurrences, and a random
tail that differs from step to step. small_batch: fewer than 1024 unique keys
(one tile of the open)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)

ROWS = 4200
PER_ROW = 6
THRESHOLD = 2  # embedding threshold: a key of >= 3 occurrences gets its row in its first open
N_SMALL = 300  # keys of 1-4 occurrences, 75 of each
_ID_ALL, _ID_64, _ID_65, _ID_SMALL, _ID_TAIL = 1, 2, 3, 1000, 100_000
TAIL_POOL = 6000


def _key_of(ids):
    k = np.atleast_1d(np.asarray(ids, dtype=np.uint64)) * np.uint64(0x9E3779B97F4A7C15)
    return ((k & np.uint64((1 << 62) - 1)) + np.uint64(7)).astype(np.int64)


def make_batch(step, rows=ROWS):
    g = np.random.default_rng([41, step])
    ids = np.empty((rows, PER_ROW), dtype=np.int64)
    ids[:, 0] = _ID_ALL
    free = (rows * (PER_ROW - 1))
    fill = np.empty(free, dtype=np.int64)
    planted = [np.full(64, _ID_64), np.full(65, _ID_65)]
    for j in range(N_SMALL):
        planted.append(np.full(1 + j % 4, _ID_SMALL + j))
    planted = np.concatenate(planted)
    fill[:planted.size] = planted
    fill[planted.size:] = _ID_TAIL + g.integers(0, TAIL_POOL, free - planted.size)
    ids[:, 1:] = fill[g.permutation(free)].reshape(rows, PER_ROW - 1)
    b = types.SimpleNamespace()
    b.rows = rows
    b.keys = torch.from_numpy(_key_of(ids.reshape(-1)))
    b.off = torch.arange(rows + 1, dtype=torch.int64) * PER_ROW
    b.label = torch.from_numpy((g.random(rows) < 0.3).astype(np.float32))
    b.key_all, b.key_64, b.key_65 = (int(_key_of(i)[0]) for i in (_ID_ALL, _ID_64, _ID_65))
    b.small_keys = _key_of(_ID_SMALL + np.arange(N_SMALL))
    return b


def small_batch(step, rows=150):
    """U < 1024: ids of the big batch's small and tail ranges, 4 per row."""
    g = np.random.default_rng([43, step])
    ids = np.where(g.random((rows, 4)) < 0.5, _ID_SMALL + g.integers(0, N_SMALL, (rows, 4)),
                   _ID_TAIL + g.integers(0, 200, (rows, 4)))
    b = types.SimpleNamespace()
    b.rows = rows
    b.keys = torch.from_numpy(_key_of(ids.reshape(-1)))
    b.off = torch.arange(rows + 1, dtype=torch.int64) * 4
    b.label = torch.from_numpy((g.random(rows) < 0.3).astype(np.float32))
    return b


def check_structure(b):
    """The conditions the tests rely on (not measurements), on a big batch."""
    keys, cnt = np.unique(b.keys.numpy(), return_counts=True)
    of = dict(zip(keys.tolist(), cnt.tolist()))
    assert of[b.key_all] == b.rows and b.rows > 64 * 64
    assert of[b.key_64] == 64 and of[b.key_65] == 65
    U = keys.size
    assert U % 1024 != 0 and U > 2 * 1024, U  # three or more tiles, the last one partial
    # embedded from the first open on (count > THRESHOLD at once), so every
    # training step runs them through the backward's V chunks
    small = [of[int(k)] for k in b.small_keys]
    assert all(1 <= c <= 4 for c in small)
    assert sum(c > THRESHOLD for c in small) >= 100
    assert min(of[b.key_64], of[b.key_65], of[b.key_all]) > THRESHOLD
    return U


def five_steps():
    """big, small, big, small, big"""
    return [make_batch(0), small_batch(0), make_batch(1), small_batch(1), make_batch(2)]


def train(fused, batches, dim, dev):
    from wormhole_amd.config.schema import DifactoConfig, Embedding
    from wormhole_amd.models.difacto import DifactoLearner
    from wormhole_amd.parallel.comm import Comm
    os.environ["WH_DIFACTO_NATIVE"] = "1"
    os.environ["WH_DIFACTO_FUSED_V"] = "1" if fused else "0"
    conf = DifactoConfig(embedding=[Embedding(dim=dim, threshold=THRESHOLD)], lambda_l1=0.01,
                         l1_shrk=False, max_concurrency=2, fixed_bytes=0)
    lr = DifactoLearner(conf, Comm(dev, init=False), dev, cap=1 << 16, vcap=1 << 14, seed=5)
    assert lr._nat is not None and lr._nat.direct and lr._nat.fused_v == fused
    dv = [(b.keys.to(dev), b.off.to(dev), b.label.to(dev)) for b in batches]
    for s, (k, o, l) in enumerate(dv):
        nb = (dv[s + 1][0], dv[s + 1][1], None) if s + 1 < len(dv) else None
        lr.process(k, o, None, l, 0, 0, next_batch=nb)
    lr.flush()
    return lr


def model_by_key(lr):
    """The store's occupied slots sorted by key: keys, cnt, w, z, sq, has-row
    flags [n] and the V / VG rows [n, vstride] (zeros without a row)."""
    st = lr.store
    occ = st.occupied().long()
    keys = st.keys[occ.to(st.keys.device)].cpu()
    order = torch.argsort(keys)
    pick = lambda t: t[occ.to(t.device)].cpu()[order]  # noqa: E731
    m = types.SimpleNamespace()
    m.keys = keys[order]
    m.cnt, m.w, m.z, m.sq = pick(st.cnt), pick(st.w), pick(st.z), pick(st.sq)
    vrow = pick(st.vrow).long()
    m.has = vrow >= 0
    V, VG = st.V.cpu(), st.VG.cpu()
    m.V = torch.zeros(keys.numel(), V.shape[1])
    m.VG = torch.zeros(keys.numel(), V.shape[1])
    m.V[m.has] = V[vrow[m.has]]
    m.VG[m.has] = VG[vrow[m.has]]
    return m


def check_rows(m, b):
    """The planted keys have an embedding row after training."""
    def has(key):
        hit = (m.keys == key).nonzero()
        assert hit.numel() == 1, key
        return bool(m.has[int(hit)])
    assert has(b.key_64), "the 64-occurrence key has no embedding row"
    assert has(b.key_65), "the 65-occurrence key has no embedding row"
    assert has(b.key_all), "the every-row key has no embedding row"
    small = torch.isin(m.keys, torch.from_numpy(b.small_keys))
    assert int((small & m.has).sum()) >= 100, int((small & m.has).sum())


def bits(t):
    return t.contiguous().view(torch.int32)


def main():
    assert os.environ.get("WH_DETERMINISTIC") == "1", "run with WH_DETERMINISTIC=1"
    dev = torch.device("cuda", 0)
    batches = five_steps()
    for b in batches[::2]:
        check_structure(b)
    ma, mb = (model_by_key(train(f, batches, 8, dev)) for f in (True, False))
    check_rows(ma, batches[0])
    assert torch.equal(ma.keys, mb.keys), "key sets differ"
    assert torch.equal(ma.cnt, mb.cnt) and torch.equal(ma.has, mb.has), "cnt / row allocation"
    for name in ("w", "z", "sq", "V", "VG"):
        a, c = bits(getattr(ma, name)), bits(getattr(mb, name))
        diff = (a != c).reshape(a.shape[0], -1).any(1)
        print("  %-2s keys that differ: %d of %d" % (name, int(diff.sum()), a.shape[0]))
        assert not bool(diff.any()), "%s differs, first at key %d" % (
            name, int(ma.keys[int(diff.nonzero()[0])]))
    assert float(ma.VG.abs().sum()) > 0 and int(ma.has.sum()) > 500
    print("OK")


if __name__ == "__main__":
    main()
