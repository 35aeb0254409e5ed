#!/usr/bin/env python3
"""Pan-genome k-mer classes (extract_core_kmers / extract_dispensable_kmers / extract_singleton_kmers, reference src/snippets.c:10-106) through
bft_gpu_kmers_by_count(_dev) and bft_gpu_pangenome_stats(_dev) on two indexes: config 3 (100 genomes, k = 27, workloads.PanGenome) and config 5
(k = 63, 2000 variants of one 20 kbp ancestor).  Per index, one JSON line with
  * the statistics call and the three classes (packed k-mers + ASCII + rows) through the device forms: GPU time between HIP events with the outputs
    resident (median and spread of `reps` calls after a warm-up call of the same shape), the GPU time and algorithmic bytes of each stage
    ("build_stages"), the bytes over the time, and the size of the dictionary's offsets (the target of the two dependent gathers);
  * the host forms, wall clock, copies back included;
  * the route a caller had before these calls, wall clock: bft_gpu_extract (every k-mer and colour-set id to the host), bft_gpu_colorset per colour
    set, classification in numpy; its classes and spectrum are checked against the new calls'.
A third line sets the statistics call on an index where one colour set owns over 90 % of the rows beside an index of the same size whose rows
are spread evenly over 255 colour sets: the pair that shows what the hot counter costs.
usage: bench_pangenome.py [reps] [--skip5]"""
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


def stats_dev(t, genomes):
    sp = torch.zeros(genomes + 1, dtype=torch.int64, device=dev)
    to = torch.zeros(genomes, dtype=torch.int64, device=dev)
    pr = torch.zeros(genomes, dtype=torch.int64, device=dev)
    call = lambda: t.pangenome_stats_dev(sp.data_ptr(), to.data_ptr(), pr.data_ptr(), genomes + 1, stream=st)
    r = timed(call)
    r["stages"] = staged(t, call)
    return r, sp.cpu().numpy().astype(np.uint64)


def old_route(t, genomes):
    """what a caller did before: everything to the host, one bft_gpu_colorset per set, numpy"""
    t0 = time.perf_counter()
    km, cs = t.extract()
    sizes = np.array([len(t.colorset(c)) for c in range(int(t.info()["colorsets"]))], dtype=np.int64)
    count = sizes[cs]
    classes = {"core": km[count == genomes], "dispensable": km[count < genomes], "singleton": km[count == 1]}
    spectrum = np.bincount(count, minlength=genomes + 1)
    return time.perf_counter() - t0, classes, spectrum


def measure(name, t, genomes):
    info = t.info()
    n, n_sets = int(info["kmers"]), int(info["colorsets"])
    out = {"index": name, "k": t.k, "genomes": genomes, "kmers": n, "colorsets": n_sets, "cs_off_bytes": 4 * (n_sets + 1), "reps": reps}
    out["stats_dev"], spectrum = stats_dev(t, genomes)
    t0 = time.perf_counter()
    host_spectrum = t.pangenome_stats()[0]
    out["stats_host_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    assert host_spectrum.tolist() == spectrum.tolist() and int(spectrum.sum()) == n
    ranges = {"core": (genomes, genomes), "dispensable": (0, genomes - 1), "singleton": (1, 1)}
    host = {}
    for cls, (lo, hi) in ranges.items():
        cnt = torch.zeros(1, dtype=torch.int64, device=dev)
        t.kmers_by_count_dev(lo, hi, 0, 0, 0, 0, cnt.data_ptr(), stream=st)  # the size first
        torch.cuda.synchronize()
        m = int(cnt.cpu()[0])
        dk = torch.zeros((max(m, 1), t.nb), dtype=torch.uint8, device=dev)
        da = torch.zeros((max(m, 1), t.k + 1), dtype=torch.uint8, device=dev)
        dr = torch.zeros(max(m, 1), dtype=torch.int32, device=dev)
        call = lambda: t.kmers_by_count_dev(lo, hi, dk.data_ptr(), da.data_ptr(), dr.data_ptr(), m, cnt.data_ptr(), stream=st)
        r = timed(call)
        r["selected"] = m
        r["stages"] = staged(t, call)
        # the bytes the passes move: the selection reads tcol and two gathered offsets and writes a slot per row; the emission reads two slots per row
        # and, per selected row, reads the key and writes packed k-mer, ASCII and row
        W8 = 8 * ((2 * t.k + 63) // 64)
        r["alg_bytes"] = n * (4 + 8 + 4) + n * 4 + m * (W8 + t.nb + t.k + 1 + 4)
        r["GB/s"] = round(r["alg_bytes"] / r["ms"] / 1e6, 1)
        t0 = time.perf_counter()
        packed, _ = t.kmers_by_count(lo, hi)
        r["host_form_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        host[cls] = packed
        out[cls] = r
        del dk, da, dr
    wall, classes, old_spectrum = old_route(t, genomes)
    out["old_route_wall_ms"] = round(wall * 1e3, 1)  # (all three classes and the spectrum from one extract)
    assert old_spectrum.tolist() == spectrum.tolist()
    for cls in ranges:
        assert classes[cls].tobytes() == host[cls].tobytes(), cls
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


def hot_and_even(k=27, length=4_000_000):
    """one colour set over 90 % of the rows / 255 colour sets of equal shares, over the same k-mers"""
    base = torch.from_numpy(S.distinct(S.kmers_of(S.random_genome(length, 31), k))).to(dev)
    rng = torch.Generator(device=dev)
    rng.manual_seed(5)
    res = {"index": "hot_vs_even", "k": k, "reps": reps}
    for shape in ("hot", "even"):
        t = BFT(k)
        for g in range(8):
            # hot: genomes 0 and 1 carry 97 % of the k-mers each (both: 94 %), the other six 0.2 % each; even: every genome carries half of them
            share = 0.5 if shape == "even" else 0.97 if g < 2 else 0.002
            keep = torch.rand(len(base), generator=rng, device=dev) < share
            part = base[keep].contiguous()
            t.insert_kmers_dev_async(part.data_ptr(), part.shape[0], g, st)
            torch.cuda.synchronize()
        t.build()
        r, spectrum = stats_dev(t, 8)
        _, cs = t.extract()
        share = float(np.bincount(cs).max()) / len(cs)
        res[shape] = {"kmers": int(t.info()["kmers"]), "colorsets": int(t.info()["colorsets"]), "largest_set_share": round(share, 4), **r}
        t.close()
    print(json.dumps(res), flush=True)


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
hot_and_even()
