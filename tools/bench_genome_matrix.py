#!/usr/bin/env python3
"""The genome-by-genome shared k-mer matrix (bft_gpu_genome_matrix_dev) on two indexes: config 3 (100 genomes, k = 27, workloads.PanGenome) and
config 5 (k = 63, 2000 variants of one 20 kbp ancestor).  Per index, one JSON line with
  * the device form on each road ("test_genome_matrix_road" 1 sparse, 2 dense) and as the cost model chooses (0; the road it took is reported): GPU time
    between HIP events with the output resident (median and spread of `reps` calls after a warm-up call), the GPU time and algorithmic bytes of
    each stage ("build_stages");
  * the ratio sparse / dense beside the two costs the model weighs (pair updates, digit steps x 64 x Gpad^2 / 2 multiply-adds): what BFT_GM_PAIR_COST
    (csrc/bft_genome_matrix.h) is set from;
  * the host form, wall clock, copy back included;
  * the route a caller had before this call, wall clock: bft_gpu_extract (every k-mer and colour-set id to the host), bft_gpu_colorset per colour
    set, the product in numpy.
Both roads and the old route are asserted to give the same matrix.
usage: bench_genome_matrix.py [reps] [--skip5]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from bloomfiltertrie_amd import BFT, _lib, synth as S, workloads as W  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 7
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream


def timed(call):
    """median / min / max GPU ms of `reps` calls, each between its own pair of events, after one warm-up call"""
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def staged(t, call):
    t.set_option("build_stages", 1)
    call()
    torch.cuda.synchronize()
    out = [{"stage": nm, "ms": round(ms, 4), "alg_bytes": by, "GB/s": round(by / ms / 1e6, 1) if ms > 0 else None} for nm, ms, by in t.build_stages()]
    t.set_option("build_stages", 0)
    return out


def road_taken(t):
    out = (C.c_uint32 * 2)()
    _lib.check(_lib.load().bft_gpu_test_genome_matrix_state(t._h, 0, out))
    return {1: "sparse", 2: "dense"}.get(int(out[0]), "none")


def old_route(t, genomes):
    """what a caller did before: everything to the host, one bft_gpu_colorset per set, numpy"""
    t0 = time.perf_counter()
    _, cs = t.extract()
    n_sets = int(t.info()["colorsets"])
    B = np.zeros((n_sets, genomes), dtype=np.float64)  # (float64: BLAS; every sum is an integer below 2^53)
    sizes = np.zeros(n_sets, dtype=np.int64)
    for c in range(n_sets):
        ids = t.colorset(c)
        B[c, ids] = 1.0
        sizes[c] = len(ids)
    usage = np.bincount(cs, minlength=n_sets).astype(np.float64)
    m = (B.T * usage) @ B
    return time.perf_counter() - t0, m.astype(np.uint64), sizes, usage


def measure(name, t, genomes):
    info = t.info()
    n, n_sets = int(info["kmers"]), int(info["colorsets"])
    out = {"index": name, "k": t.k, "genomes": genomes, "kmers": n, "colorsets": n_sets, "reps": reps}
    d = torch.zeros(genomes * genomes, dtype=torch.int64, device=dev)
    call = lambda: t.genome_matrix_dev(d.data_ptr(), genomes * genomes, stream=st)
    got = {}
    for road, key in ((1, "sparse"), (2, "dense"), (0, "auto")):
        t.set_option("test_genome_matrix_road", road)
        r = timed(call)
        r["stages"] = staged(t, call)
        r["road"] = road_taken(t)
        got[key] = d.cpu().numpy().astype(np.uint64).reshape(genomes, genomes).copy()
        out[key] = r
        print(json.dumps({"index": name, "road": key, "took": r["road"], "ms": r["ms"]}), flush=True)  # (progress: the full line follows)
    t0 = time.perf_counter()
    host = t.genome_matrix()
    out["host_form_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    wall, old, sizes, usage = old_route(t, genomes)
    out["old_route_wall_ms"] = round(wall * 1e3, 1)
    for key, m in got.items():
        assert np.array_equal(m, old), key
    assert np.array_equal(host, old)
    # what the cost model weighs
    gpad = (genomes + 15) // 16 * 16
    pad = (-n_sets) % 64
    w = np.concatenate([usage.astype(np.int64), np.zeros(pad, dtype=np.int64)]).reshape(-1, 64)
    digit_steps = sum(int(((w >> (7 * dg)) & 127).any(axis=1).sum()) for dg in range(5))
    pairs = int((sizes * (sizes + 1) // 2)[usage > 0].sum())
    out["pair_updates"] = pairs
    out["dense_macs"] = digit_steps * 64 * gpad * gpad // 2
    out["sparse_over_dense_ms"] = round(out["sparse"]["ms"] / out["dense"]["ms"], 3)
    out["macs_per_pair_update_at_equal_time"] = round(out["dense_macs"] / max(pairs, 1) * out["sparse"]["ms"] / out["dense"]["ms"], 1)
    print(json.dumps(out), flush=True)


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
