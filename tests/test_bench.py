"""bench.py --dump-outputs on the host: file names, dtype, the size cap and its seeded sample.  No GPU needed: a
stand-in handler answers the four calls dump_outputs makes."""
import os

import numpy as np

import bench


class _Handler:
    """n_white / n_yolk particles whose every field holds the particle index (plus a per-field, per-type offset),
    so that a written sample tells which particles it took"""

    def __init__(self, n_batches, n_white, n_yolk):
        self.n_batches, self.counts = n_batches, (n_white, n_yolk)

    def list_ids(self):
        return list(range(1, self.n_batches + 1))

    def get_positions(self, ids):
        ids = np.asarray(ids, dtype=np.float64)
        return ids + 0.25, ids - 0.25

    def get_n_particles(self):
        return self.counts

    def download(self, which, field):
        return np.arange(self.counts[which], dtype=np.float64) + 1e7 * bench.DUMP_FIELDS.index(field) + 0.5 * which


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_writes_every_particle_under_the_cap(tmp_path):
    h = _Handler(6, 40, 12)
    bench.dump_outputs(h, str(tmp_path), bench.DUMP_BYTES)
    got = _load(str(tmp_path))
    assert sorted(got) == sorted(["batch_x", "batch_y"] + ["%s_%s" % (t, f) for t in ("white", "yolk") for f in bench.DUMP_FIELDS])
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["batch_x"], np.arange(1, 7) + 0.25) and np.array_equal(got["batch_y"], np.arange(1, 7) - 0.25)
    for w, t in ((0, "white"), (1, "yolk")):
        for f in bench.DUMP_FIELDS:
            assert np.array_equal(got["%s_%s" % (t, f)], h.download(w, f))


def test_dump_above_the_cap_is_one_fixed_sample(tmp_path):
    h = _Handler(100, 30000, 7000)
    budget = 400 << 10  # room for ~12k of the 37k particles
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(h, a, budget, "rank0_")
    bench.dump_outputs(h, b, budget, "rank0_")
    assert sum(os.path.getsize(os.path.join(a, n)) for n in os.listdir(a)) <= budget
    got, again = _load(a), _load(b)
    assert sorted(got) == sorted(again) and all(np.array_equal(got[k], again[k]) for k in got)
    for w, t in ((0, "white"), (1, "yolk")):
        sel = (got["rank0_%s_x" % t] - 0.5 * w).astype(np.int64)  # field x holds the particle index
        assert 0 < sel.size < h.counts[w] and np.all(np.diff(sel) > 0)
        for f in bench.DUMP_FIELDS:
            assert np.array_equal(got["rank0_%s_%s" % (t, f)], h.download(w, f)[sel])
