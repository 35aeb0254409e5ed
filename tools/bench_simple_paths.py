#!/usr/bin/env python3
"""Simple paths (extract_simple_paths_to_disk / extract_simple_core_paths_to_disk, reference src/snippets.c:115-603) through
bft_gpu_simple_paths_dev on two indexes: config 3 (100 genomes, k = 27, workloads.PanGenome) and config 5 (k = 63, 2000 variants of one
20 kbp ancestor).  Per threshold (t = 0 and the core threshold (int)(0.9 * genomes)): GPU time per stage ("build_stages": events between the
stages of one call, bytes its algorithm reads and writes), the whole call between HIP events after a warm-up call of the same shape, paths,
characters, the longest path and stored k-mers per second.  One JSON line per (index, threshold).
usage: bench_simple_paths.py [reps] [--skip5]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from bloomfiltertrie_amd import BFT, synth as S, workloads as W  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 5
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream


def measure(name, t, genomes):
    n_kmers = int(t.info()["kmers"])
    for thr in (0, int(0.9 * genomes)):
        cnt = torch.zeros(3, dtype=torch.int64, device=dev)
        t.simple_paths_dev(0, 0, 0, 0, cnt.data_ptr(), min_shared=thr, stream=st)  # the sizes first
        torch.cuda.synchronize()
        n_paths, n_chars, longest = (int(v) for v in cnt.cpu().tolist())
        off = torch.zeros(n_paths + 1, dtype=torch.int64, device=dev)
        seq = torch.zeros(max(n_chars, 1), dtype=torch.uint8, device=dev)
        call = lambda: t.simple_paths_dev(off.data_ptr(), seq.data_ptr(), n_paths, n_chars, cnt.data_ptr(), min_shared=thr, stream=st)
        call()  # warm-up of the timed shape
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / reps
        t.set_option("build_stages", 1)
        call()
        stages = [{"stage": nm, "ms": round(sms, 4), "alg_bytes": by, "GB/s": round(by / sms / 1e6, 1) if sms > 0 else None} for nm, sms, by in t.build_stages()]
        t.set_option("build_stages", 0)
        # spot check: every path is at least k characters, the offsets ascend and end at n_chars
        o = off.cpu()
        assert int(o[0]) == 0 and int(o[-1]) == n_chars and bool(((o[1:] - o[:-1]) >= t.k).all())
        print(json.dumps({"index": name, "k": t.k, "genomes": genomes, "kmers": n_kmers, "min_shared": thr, "paths": n_paths, "chars": n_chars,
                          "longest": longest, "ms": round(ms, 3), "kmers_per_s": round(n_kmers / (ms / 1e3), 1), "stages": stages}), flush=True)


def config3():
    pan = W.PanGenome(100, 2_000_000, 0.01, 4242, dev)
    t = BFT(27)
    W.build_index(t, pan, 27)
    return t, 100


def config5(genomes=2000, length=20000, k=63):
    anc = S.random_genome(length, 77)
    t = BFT(k)
    for g in range(genomes):
        t.insert_kmers(S.distinct(S.kmers_of(S.mutate(anc, 0.01, 5000 + g), k)), g)
    t.build()
    return t, genomes


t0 = time.perf_counter()
t, g = config3()
print(json.dumps({"index": "config3", "setup_s": round(time.perf_counter() - t0, 1)}), flush=True)
measure("config3", t, g)
t.close()
if "--skip5" not in sys.argv:
    t0 = time.perf_counter()
    t, g = config5()
    print(json.dumps({"index": "config5", "setup_s": round(time.perf_counter() - t0, 1)}), flush=True)
    measure("config5", t, g)
    t.close()
