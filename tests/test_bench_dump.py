"""CPU: what bench.py --dump-outputs writes (bench.dump_outputs), with stand-in beads: float64 arrays of the last timed step, all files
together within DUMP_MAX_BYTES, a larger per-atom output sampled at the same seeded atoms every time.  The option on the GPU:
tests/test_gpu_bench_ranks.py."""
import os

import numpy as np

import bench
from mpmcxx_amd import energy


class Bead:
    def __init__(self, n, seed, polar=True):
        rng = np.random.default_rng(seed)
        self.n, self.polar = n, polar
        self.mu, self.e = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))

    def dipoles(self):
        if not self.polar:
            raise energy.MpmcError(-1, "mpmc_get_dipoles: no polarization evaluation has run")
        return self.mu, self.e, np.zeros((self.n, 3))


def per_bead(b):
    return [{k: float(10 * i + j) for j, k in enumerate(bench.BEAD_TERMS)} for i in range(b)]


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_every_atom_of_every_bead_below_the_cap(tmp_path):
    beads = [Bead(50, s) for s in range(3)]
    files = bench.dump_outputs(str(tmp_path), -12.5, [1.0, 2.0, 3.0, 4.0], per_bead(3), beads, [0, 1, 2])
    got = load(tmp_path)
    assert sorted(files) == sorted(f"{k}.npy" for k in got)
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["potential"] == -12.5 and got["observables"].tolist() == [1.0, 2.0, 3.0, 4.0] and got["bead_ids"].tolist() == [0, 1, 2]
    assert got["bead_energies"].shape == (3, len(bench.BEAD_TERMS)) and got["bead_energies"][2, 1] == 21.0
    assert got["dipole_atoms"].tolist() == list(range(50))
    assert np.array_equal(got["bead_dipoles"], np.stack([b.mu for b in beads]))
    assert np.array_equal(got["bead_static_field"], np.stack([b.e for b in beads]))


def test_larger_output_is_a_fixed_sample_within_the_cap(tmp_path, monkeypatch):
    cap = 200_000
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", cap)
    beads = [Bead(4000, s) for s in range(4)]  # 4 x 4000 x 48 bytes of per-atom arrays: about four times the cap
    runs = []
    for k in range(2):
        d = str(tmp_path / str(k))
        bench.dump_outputs(d, 1.0, np.zeros(4), per_bead(4), beads, range(4))
        assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= cap
        runs.append(load(d))
    a, b = runs
    idx = a["dipole_atoms"].astype(np.int64)
    assert 0 < len(idx) < 4000 and np.all(np.diff(idx) > 0) and np.array_equal(a["dipole_atoms"], b["dipole_atoms"])
    assert np.array_equal(a["bead_dipoles"], np.stack([bd.mu[idx] for bd in beads]))
    assert np.array_equal(a["bead_static_field"], b["bead_static_field"])


def test_no_per_atom_arrays_without_polarization(tmp_path):
    files = bench.dump_outputs(str(tmp_path), 1.0, np.zeros(4), per_bead(2), [Bead(10, 0, polar=False), Bead(10, 1, polar=False)], [0, 1])
    assert files == ["bead_energies.npy", "bead_ids.npy", "observables.npy", "potential.npy"]
