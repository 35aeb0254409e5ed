#!/usr/bin/env python3
"""Generates tests/golden/ref_prims.npz: known answers of the reference's own xxhash.c / log2.c / popcnt.c.

Needs oracle/_ref/libbftref_prims.so, which build() compiles only where the reference sources are present.  The stored
vectors let tests/test_oracle_pins.py check the oracle's primitives everywhere else.  Inputs are seeded; re-running
reproduces the file.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import oracle as O  # noqa: E402

SEEDS = [0, 1, 1804289383, 846930886, 2 ** 63 + 5]  # the last two of survey_pins.json's default_seeds among them
LENGTHS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 31, 32, 33, 63, 64, 65, 100, 257]
IDS = list(range(0, 70000, 7)) + [63, 64, 4095, 4096, 2 ** 18 - 1, 2 ** 18, 2 ** 24, 10 ** 8]


def main():
    O.build()
    ref = O.ref_prims()
    if ref is None:
        raise SystemExit("oracle/_ref/libbftref_prims.so is not built: run build() where the reference sources are present")
    rng = np.random.default_rng(7)
    data, out = [], np.zeros((len(SEEDS), len(LENGTHS)), dtype=np.uint64)
    for i, seed in enumerate(SEEDS):
        for j, ln in enumerate(LENGTHS):
            d = rng.integers(0, 256, ln, dtype=np.uint8)
            data.append(d)
            out[i, j] = ref.BFT_HASH_XXH64(d.tobytes(), ln, seed)
    ids = np.array(IDS, dtype=np.uint32)
    nb = np.array([ref.get_nb_bytes_power2_annot(int(i)) for i in ids], dtype=np.int32)
    rev = np.frombuffer(bytes((C.c_uint8 * 256).in_dll(ref, "rev")), dtype=np.uint8)
    pop = np.frombuffer(bytes((C.c_uint8 * 256).in_dll(ref, "POPCOUNT_8bit")), dtype=np.uint8)
    np.savez_compressed(os.path.join(HERE, "ref_prims.npz"), xxh_seeds=np.array(SEEDS, dtype=np.uint64),
                        xxh_lengths=np.array(LENGTHS, dtype=np.int32), xxh_data=np.concatenate(data), xxh64=out,
                        nb_ids=ids, nb_bytes=nb, rev=rev, popcount8=pop)
    print("wrote", os.path.join(HERE, "ref_prims.npz"))


if __name__ == "__main__":
    main()
