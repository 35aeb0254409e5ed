#!/usr/bin/env python3
"""Colour-set algebra over groups of k-mers (intersection_annotations / union_annotations / sym_difference_annotations, reference src/bft.c:421-613)
through bft_gpu_combine_colors_dev on two indexes: config 3 (100 genomes, k = 27, workloads.PanGenome) and config 5 (k = 63, 2000 variants of one
20 kbp ancestor).  Three shapes of groups per index: reads (100 consecutive k-mers of a genome each), pairs (2 consecutive k-mers each) and one group
per 6-nt prefix (every stored k-mer, grouped by bft_gpu_query_prefixes' offsets).  Per index and shape, one JSON line with
  * the three ops through the device form, rows + counts + found resident: GPU time between HIP events (median and spread of `reps` calls after a
    warm-up call of the same shape), the stages of one call ("build_stages");
  * the bytes the algorithm must move: the batch, one line of the k-mer hash per k-mer, one dictionary row per run of equal colour sets inside a group,
    one output row per group -- and those bytes over the median time;
  * the route that exists without these calls, wall clock: bft_gpu_query_color_rows_dev (a row per k-mer), the copy to the host, a numpy reduction per
    group; its rows are checked to equal the new call's, op by op.
usage: bench_setops.py [reps] [--skip5] [--tiny]      (--tiny: two small indexes of the same kinds, to try the tool out in seconds)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from bloomfiltertrie_amd import BFT, synth as S, workloads as W  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 7
tiny = "--tiny" in sys.argv
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream
OPS = ("and", "or", "symdiff")


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
    out = [{"stage": nm, "ms": round(ms, 4), "alg_bytes": by} for nm, ms, by in t.build_stages()]
    t.set_option("build_stages", 0)
    return out


def host_reduce(rows, off, op):
    """the reduction a caller writes today: rows uint8 [n, rb] on the host, one group at a time through reduceat (empty groups: zero rows)"""
    ng = len(off) - 1
    out = np.zeros((ng, rows.shape[1]), dtype=np.uint8)
    size = np.diff(off.astype(np.int64))
    full = np.nonzero(size > 0)[0]
    if len(full) == 0:
        return out
    starts = off[full].astype(np.int64)
    # (reduceat runs to the next start: the groups are contiguous here, which every shape of this tool is)
    any_ = np.bitwise_or.reduceat(rows, starts, axis=0)
    all_ = np.bitwise_and.reduceat(rows, starts, axis=0)
    out[full] = all_ if op == "and" else any_ if op == "or" else np.where((size[full] == 1)[:, None], any_, any_ & ~all_)
    return out


def measure(index, shape, t, dq, off):
    n, ng = dq.shape[0], len(off) - 1
    genomes = int(t.info()["genomes"])
    rb = (genomes + 7) // 8
    doff = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    rows = torch.zeros((ng, rb), dtype=torch.uint8, device=dev)
    counts = torch.zeros(ng, dtype=torch.int32, device=dev)
    found = torch.zeros(ng, dtype=torch.int32, device=dev)
    # runs of equal colour sets inside the groups: a dictionary row has to be read once per run
    _, _, sets = t.query_rows(dq.cpu().numpy())
    heads = np.ones(n, dtype=bool)
    heads[1:] = sets[1:] != sets[:-1]
    heads[off[:-1][off[:-1] < n].astype(np.int64)] = True
    runs = int(heads[sets != 0xFFFFFFFF].sum())
    out = {"index": index, "shape": shape, "k": t.k, "genomes": genomes, "kmers_in_batch": n, "groups": ng, "row_bytes": rb, "runs": runs, "reps": reps,
           "alg_bytes": n * t.nb + n * 64 + runs * ((rb + 3) // 4 * 4) + ng * (rb + 8) + (ng + 1) * 8}
    new_rows = {}
    for op in OPS:
        call = lambda: t.combine_colors_dev(dq.data_ptr(), n, doff.data_ptr(), ng, op, 0, rows.data_ptr(), counts.data_ptr(), found.data_ptr(), stream=st)
        r = timed(call)
        r["GB/s"] = round(out["alg_bytes"] / r["ms"] / 1e6, 1) if r["ms"] > 0 else None
        if op == "and":
            r["stages"] = staged(t, call)
        new_rows[op] = rows.cpu().numpy().copy()
        assert (counts.cpu().numpy() == np.unpackbits(new_rows[op], axis=1).sum(axis=1)).all()
        out[op] = r
    # today's route: a row per k-mer, copied, reduced on the host
    bits = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
    per = torch.zeros((n, rb), dtype=torch.uint8, device=dev)
    scr = torch.zeros(n, dtype=torch.int32, device=dev)
    r = timed(lambda: t.query_color_rows_dev(dq.data_ptr(), n, bits.data_ptr(), per.data_ptr(), scr.data_ptr(), stream=st))
    out["old_route"] = {"color_rows_dev": r, "rows_bytes": n * rb}
    t0 = time.perf_counter()
    host_rows = per.cpu().numpy()
    out["old_route"]["copy_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    for op in OPS:
        t0 = time.perf_counter()
        red = host_reduce(host_rows, off, op)
        out["old_route"][f"reduce_{op}_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        assert red.tobytes() == new_rows[op].tobytes(), (index, shape, op)
    print(json.dumps(out), flush=True)


def shapes(index, t, windows):
    """windows: the packed k-mers of one genome in genome order, on the device"""
    n = (min(windows.shape[0], 200_000 if tiny else 20_000_000) // 100) * 100
    dq = windows[:n].contiguous()
    measure(index, "reads_of_100", t, dq, np.arange(0, n + 1, 100, dtype=np.uint64))
    measure(index, "pairs", t, dq, np.arange(0, n + 1, 2, dtype=np.uint64))
    codes = ((np.arange(4096)[:, None] >> (2 * np.arange(6)[::-1])) & 3).astype(np.uint8)
    prefixes = ["".join("ACGT"[c] for c in row) for row in codes]
    off, km, _, _ = t.query_prefixes(prefixes)
    measure(index, "one_group_per_6nt_prefix", t, torch.from_numpy(km).to(dev), off.astype(np.uint64))


def config3():
    pan = W.PanGenome(8 if tiny else 100, 50_000 if tiny else 2_000_000, 0.01, 4242, dev)
    t = BFT(27)
    W.build_index(t, pan, 27)
    return t, W.pack_windows(pan.genome(0), 27)


def config5(genomes=2000, length=20000, k=63):
    if tiny:
        genomes, length = 40, 5000
    anc = S.random_genome(length, 77)
    t = BFT(k)
    for g in range(genomes):
        t.insert_kmers(S.distinct(S.kmers_of(S.mutate(anc, 0.01, 5000 + g), k)), g)
    t.build()
    return t, torch.from_numpy(S.kmers_of(S.mutate(anc, 0.01, 5000), k)).to(dev)


for name, make in (("config3", config3), ("config5", config5)):
    if name == "config5" and "--skip5" in sys.argv:
        continue
    t0 = time.perf_counter()
    t, windows = make()
    print(json.dumps({"index": name, "setup_s": round(time.perf_counter() - t0, 1)}), flush=True)
    shapes(name, t, windows)
    t.close()
