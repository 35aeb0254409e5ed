#!/usr/bin/env python3
"""Insertion from sequences (bft_gpu_insert_sequences_dev, csrc/bft_ingest.hip) on the config-3 genome set (100 genomes = one 2 Mbp ancestor with
1 % SNPs each, k = 27, workloads.PanGenome), generated on the GPU: one resident ASCII sequence per genome, one call per genome, ids ascending.
Three routes fill the insertion log of a fresh handle, alternating inside every repetition:
  stream   insert_sequences_dev, min_abundance 0 (every window appended)
  count    insert_sequences_dev, min_abundance 2 (windows sorted and counted per genome; a genome of near-unique k-mers keeps almost nothing)
  kmers    bft_gpu_insert_kmers_dev on the same windows ALREADY PACKED (B bytes each) -- the route the library had before, which leaves out what it
           costs to cut the k-mers; the stream path reads B - 1 fewer bytes per k-mer and writes the same log rows
Per route: the wall time of the 100 calls (a host clock around calls that each end in a stream synchronisation) as the median of the repetitions,
positions/s, the bytes the algorithm needs (stream: 1 byte of ASCII + 8 W of log row per position; kmers: B + 8 W; count: 1 + 8 W of keys written,
read and written again by each of the sort's passes is NOT included -- only the 1 + 8 W) and, from one more pass with "timing" on, the GPU time of the
library's launches.  The stream route's log is then built and held against the kmers route's (same k-mer and pair counts).
usage: bench_ingest.py [--tiny] [--reps N] [--out file.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from bloomfiltertrie_amd import BFT, workloads as W  # noqa: E402

tiny = "--tiny" in sys.argv
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else (2 if tiny else 7)
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
k = 27
B, Wd = (2 * k + 7) // 8, (2 * k + 63) // 64
n_genomes, glen = (3, 20_000) if tiny else (100, 2_000_000)
dev = torch.device("cuda", 0)
pan = W.PanGenome(n_genomes, glen, 0.01, 4242, dev)
ascii_of = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
off = torch.tensor([0, glen], dtype=torch.int64, device=dev)
seqs, packed = [], []
for g in range(n_genomes):
    codes = pan.genome(g)
    seqs.append(ascii_of[codes.long()].contiguous())
    packed.append(W.pack_windows(codes, k))
    del codes
torch.cuda.synchronize()
positions = n_genomes * (glen - k + 1)
st = torch.cuda.current_stream().cuda_stream


def fill(route, timing=False):
    """a fresh handle filled by one route: (wall seconds of the calls, GPU ms of the library's launches or None, the handle, appended pairs)"""
    t = BFT(k)
    if timing:
        t.set_option("timing", 1)
        t.kernel_time()
    appended = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for g in range(n_genomes):
        if route == "kmers":
            t.insert_kmers_dev(packed[g].data_ptr(), packed[g].shape[0], g)
            appended += packed[g].shape[0]
        else:
            s = t.insert_sequences_dev(seqs[g].data_ptr(), off.data_ptr(), 1, glen, g, canonical=False, min_abundance=0 if route == "stream" else 2, stream=st)
            assert s["positions"] == glen - k + 1 and s["skipped"] == 0 and (route != "stream" or s["appended"] == s["positions"])
            appended += s["appended"]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, (t.kernel_time()[0] if timing else None), t, appended


routes = ("stream", "count", "kmers")
for r in routes:  # warm-up of every shape: code objects, scratch of the cache
    fill(r)[2].close()
wall = {r: [] for r in routes}
for _ in range(reps):
    for r in routes:
        dt, _, t, _ = fill(r)
        wall[r].append(dt)
        t.close()
res = {"workload": f"{n_genomes} genomes x {glen} nt, k = {k}: the insertion log filled from resident ASCII sequences (stream / count) and from packed k-mers",
       "tiny": tiny, "positions": positions, "reps": reps}
alg = {"stream": positions * (1 + 8 * Wd), "count": positions * (1 + 8 * Wd), "kmers": positions * (B + 8 * Wd)}
handles = {}
for r in routes:
    _, kms, t, appended = fill(r, timing=True)
    handles[r] = t
    med = statistics.median(wall[r])
    res[r] = {"wall_ms_median": round(med * 1e3, 3), "wall_ms_min": round(min(wall[r]) * 1e3, 3), "wall_ms_max": round(max(wall[r]) * 1e3, 3),
              "G_positions_per_s": round(positions / med / 1e9, 3), "algorithmic_bytes": alg[r], "GBps_algorithmic": round(alg[r] / med / 1e9, 1),
              "kernel_ms": round(kms, 3), "appended": appended}
res["stream_over_kmers_wall"] = round(res["stream"]["wall_ms_median"] / res["kmers"]["wall_ms_median"], 3)
res["expectation_stream_no_slower_than_kmers"] = bool(res["stream"]["wall_ms_median"] <= res["kmers"]["wall_ms_median"])
for r in ("stream", "kmers"):
    handles[r].build()
a, b = handles["stream"].info(), handles["kmers"].info()
res["ground_truth_ok"] = bool(a["kmers"] == b["kmers"] and a["pairs"] == b["pairs"] and a["kmers"] > 0)
for t in handles.values():
    t.close()
line = json.dumps(res)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
