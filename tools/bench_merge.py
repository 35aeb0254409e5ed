#!/usr/bin/env python3
"""Merging two indexes (merging_BFT, include/merge.h:14) through bft_gpu_merge on the config-3 collection (100 genomes, k = 27, workloads.PanGenome),
built as two handles split by genome 50 / 50 and 99 / 1, beside the route without it: one fresh build of all the (k-mer, genome) pairs.
Per split: wall ms of the synchronous call (median of the repetitions after one warm call) with the co-ranked placement ("merge_place" 1) and with
the search of an insertion build ("merge_place" 0), the stage split of the last call of each (build_stages: the placement stage is the line
"merge: k-mers placed"), and the ms of bft_gpu_build over all pairs inserted genome by genome into a fresh handle (the insertion itself excluded,
as tools/bench_subgraph.py does; the same median after one warm build).  The sources keep their sorted tables ("compact_table" 0).  Each merge is checked against the fresh build: k-mers, pairs, colour sets, genomes.
usage: bench_merge.py [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from bloomfiltertrie_amd import BFT, workloads as W  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
k = 27
dev = torch.device("cuda", 0)
pan = W.PanGenome(100, 2_000_000, 0.01, 4242, dev)
stream = torch.cuda.current_stream().cuda_stream


def handle(first, last):
    """genomes first .. last - 1 of the collection as genomes 0 .. of a handle, built"""
    t = BFT(k)
    for gid in range(first, last):
        packed = W.pack_windows(pan.genome(gid), k)
        t.insert_kmers_dev_async(packed.data_ptr(), packed.shape[0], gid - first, stream)
        del packed
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t.build()
    return t, (time.perf_counter() - t0) * 1e3


handle(0, pan.n)[0].close()  # warm, as for the merges: the cache of device blocks
fresh = []
for _ in range(reps):
    whole, ms = handle(0, pan.n)
    fresh.append(ms)
    want = whole.info()
    whole.close()
fresh.sort()
fresh_ms = fresh[len(fresh) // 2]
print(json.dumps({"case": "fresh build of all pairs", "build_ms": round(fresh_ms, 3), "kmers": want["kmers"], "pairs": want["pairs"],
                  "colorsets": want["colorsets"]}), flush=True)

for n_a in (pan.n // 2, pan.n - 1):
    a, _ = handle(0, n_a)
    b, _ = handle(n_a, pan.n)
    for t in (a, b):
        t.set_option("compact_table", 0)  # the sorted tables stay resident: the merge is timed, not their way back from the k-mer hash
    a.set_option("build_stages", 1)
    row = {"case": f"{n_a} / {pan.n - n_a}", "kmers_a": a.info()["kmers"], "kmers_b": b.info()["kmers"], "fresh_build_ms": round(fresh_ms, 3)}
    for place, name in ((1, "coranked"), (0, "search")):
        a.set_option("merge_place", place)
        a.merge(b).close()  # warm: the cache of device blocks, the sources' tables
        times = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = a.merge(b)
            times.append((time.perf_counter() - t0) * 1e3)
            info = out.info()
            stages = out.build_stages()
            out.close()
        for f in ("kmers", "pairs", "colorsets", "genomes"):
            assert info[f] == want[f], (f, info[f], want[f])
        times.sort()
        row[f"merge_{name}_ms"] = round(times[len(times) // 2], 3)
        row[f"place_{name}_ms"] = round(sum(ms for nm, ms, _ in stages if nm.startswith("merge: k-mers placed")), 3)
        row[f"place_{name}_gb_per_s"] = round(sum(by for nm, _, by in stages if nm.startswith("merge: k-mers placed")) / 1e6 / max(row[f"place_{name}_ms"], 1e-9), 1)
        row[f"stages_{name}"] = [(nm, round(ms, 3)) for nm, ms, _ in stages]
    print(json.dumps(row), flush=True)
    a.close()
    b.close()
