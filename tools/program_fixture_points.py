"""The query points of the scene-program SDF fixtures (tests/golden/programs_sdf.npz): a pure-integer generator, so the
fixture stores only results and the tests rebuild the same points bit for bit on any machine.

Point j of tree i: three splitmix64 outputs of the counter (i << 32) + 3j + c, reduced to integers in [-3 * 2^20,
3 * 2^20) and scaled by 2^-20 -- exact binary64 values in [-3, 3), negative coordinates included.
Used by tools/gen_program_golden.py and by the tests; numpy only."""
import hashlib

import numpy as np


def _splitmix64(x):
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def fixture_points(tree: int, n: int) -> np.ndarray:
    """(n, 3) float64 points of fixture tree `tree`."""
    counter = (np.uint64(tree) << np.uint64(32)) + np.arange(3 * n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = _splitmix64(counter)
    v = (z % np.uint64(6 << 20)).astype(np.int64) - (3 << 20)
    return (v.astype(np.float64) / float(1 << 20)).reshape(n, 3)


def sha256_f64(a) -> bytes:
    """sha256 over the little-endian binary64 bytes of `a` (the fixture's check of all results of a tree)."""
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).digest()
