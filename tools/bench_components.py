#!/usr/bin/env python3
"""Connected components (get_nb_connected_component, reference src/snippets.c:605-960) through bft_gpu_components_dev on two indexes: config 3
(100 genomes, k = 27, workloads.PanGenome) and config 5 (k = 63, 2000 variants of one 20 kbp ancestor).  Per form (the whole graph, the sub-graph
of {0}, the sub-graph of the first half of the genomes): the whole call between HIP events (labels and sizes written) after a warm-up call of the
same shape, GPU time per stage ("build_stages": events between the stages of one call, bytes its algorithm reads and writes), components,
members, the largest component and stored k-mers per second.  One JSON line per (index, form).
usage: bench_components.py [reps] [--skip5]"""
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
    lab = torch.zeros(max(n_kmers, 1), dtype=torch.int32, device=dev)
    for form, ids in (("whole", ()), ("{0}", (0,)), ("first half", tuple(range(genomes // 2)))):
        cnt = torch.zeros(3, dtype=torch.int64, device=dev)
        t.components_dev(0, 0, 0, cnt.data_ptr(), genome_ids=ids, stream=st)  # the sizes first
        torch.cuda.synchronize()
        n_comp, n_members, largest = (int(v) for v in cnt.cpu().tolist())
        sz = torch.zeros(max(n_comp, 1), dtype=torch.int64, device=dev)
        call = lambda: t.components_dev(lab.data_ptr(), sz.data_ptr(), n_comp, cnt.data_ptr(), genome_ids=ids, stream=st)
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
        # spot check: the sizes add up to the members, the largest is their maximum, as many labelled rows as members
        s = sz.cpu()[:n_comp]
        assert int(s.sum()) == n_members and (n_comp == 0 or int(s.max()) == largest)
        assert int((lab.cpu()[:n_kmers] != -1).sum()) == n_members
        print(json.dumps({"index": name, "k": t.k, "genomes": genomes, "kmers": n_kmers, "ids": form, "components": n_comp, "members": n_members,
                          "largest": largest, "ms": round(ms, 3), "kmers_per_s": round(n_kmers / (ms / 1e3), 1), "stages": stages}), flush=True)


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
# the simple-path count of the same index, for comparison (the same successor search)
cnt = torch.zeros(3, dtype=torch.int64, device=dev)
t.simple_paths_dev(0, 0, 0, 0, cnt.data_ptr(), stream=st)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(reps):
    t.simple_paths_dev(0, 0, 0, 0, cnt.data_ptr(), stream=st)
e1.record()
torch.cuda.synchronize()
print(json.dumps({"index": "config3", "simple_paths_count_ms": round(e0.elapsed_time(e1) / reps, 3)}), flush=True)
t.close()
if "--skip5" not in sys.argv:
    t0 = time.perf_counter()
    t, g = config5()
    print(json.dumps({"index": "config5", "setup_s": round(time.perf_counter() - t0, 1)}), flush=True)
    measure("config5", t, g)
    t.close()
