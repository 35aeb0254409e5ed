#!/usr/bin/env python3
"""Sub-graph builds (create_cdbg_from_bft_kmers, src/bft.c:1353-1464) through bft_gpu_subgraph_dev on the config-3 index (100 genomes, k = 27,
workloads.PanGenome), beside the from-scratch build of the same (k-mer, genome) pairs:
  1 %    a random 1 % of the stored k-mers (resident, shuffled)
  25 %   every stored k-mer whose first nucleotide is A: query_prefixes_dev straight into subgraph_dev on one stream, no host copy
  100 %  every stored k-mer (shuffled)
Per case: wall ms of the call (synchronous: the new handle is whole when it returns; median of the repetitions), k-mers/s of the batch, the
stage split of the last call (build_stages), and the ms of bft_gpu_build over the same pairs inserted genome by genome into a fresh handle.
Each sub-graph is checked: its k-mer count against the subset, its pair count against the from-scratch build's.
usage: bench_subgraph.py [reps]"""
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
nb = (2 * k + 7) // 8
dev = torch.device("cuda", 0)
pan = W.PanGenome(100, 2_000_000, 0.01, 4242, dev)
t = BFT(k)
keys, _ = W.build_index(t, pan, k)
allk = W.union_of(keys)  # sorted distinct int64 keys = the packed k-mers
n_kmers = allk.numel()
t.set_option("build_stages", 1)
s = torch.cuda.current_stream()
gen = torch.Generator(device=dev).manual_seed(7)


def timed(fn):
    best = []
    sub = None
    for _ in range(reps):
        if sub is not None:
            sub.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sub, absent = fn()
        best.append((time.perf_counter() - t0) * 1e3)
    best.sort()
    return best[len(best) // 2], sub, absent


def fresh_build(subset_keys):
    f = BFT(k)
    for gid in range(pan.n):
        g = keys[gid]
        sel = g[torch.isin(g, subset_keys)]
        if sel.numel():
            f.insert_kmers_dev(W.packed_of(sel, k).data_ptr(), sel.numel(), gid)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f.build()
    ms = (time.perf_counter() - t0) * 1e3
    info = f.info()
    f.close()
    return ms, info


def report(name, n_batch, ms, sub, absent, subset_keys):
    info = sub.info()
    fms, finfo = fresh_build(subset_keys)
    assert info["kmers"] == subset_keys.numel() == finfo["kmers"] and absent == 0, (info, finfo, absent)
    assert info["pairs"] == finfo["pairs"] and info["colorsets"] == finfo["colorsets"], (info, finfo)
    stages = [(nm, round(st_ms, 3)) for nm, st_ms, _ in sub.build_stages()]
    print(json.dumps({"case": name, "batch": n_batch, "kmers": info["kmers"], "pairs": info["pairs"], "colorsets": info["colorsets"],
                      "subgraph_ms": round(ms, 3), "kmers_per_s": n_batch / (ms * 1e-3), "fresh_build_ms": round(fms, 3), "stages": stages}), flush=True)


# 1 %
perm = torch.randperm(n_kmers, device=dev, generator=gen)
sub_keys = allk[perm[: n_kmers // 100]]
packed = W.packed_of(sub_keys, k).contiguous()
ms, sub, absent = timed(lambda: t.subgraph_dev(packed.data_ptr(), packed.shape[0], stream=s.cuda_stream))
report("1%", packed.shape[0], ms, sub, absent, torch.sort(sub_keys).values)
sub.close()

# 25 %: the prefix "A" (nucleotide 0 at bits 0-1) through query_prefixes_dev into subgraph_dev
pref = torch.zeros(nb, dtype=torch.uint8, device=dev)
lens = torch.ones(1, dtype=torch.uint8, device=dev)
off = torch.zeros(2, dtype=torch.int64, device=dev)
t.query_prefixes_dev(pref.data_ptr(), lens.data_ptr(), 1, off.data_ptr(), 0, 0, 0, 0, 0, s.cuda_stream)
torch.cuda.synchronize()
m = int(off[1].item())
dk = torch.empty(m * nb, dtype=torch.uint8, device=dev)


def prefix_then_subgraph():
    t.query_prefixes_dev(pref.data_ptr(), lens.data_ptr(), 1, off.data_ptr(), dk.data_ptr(), 0, 0, m, 0, s.cuda_stream)
    return t.subgraph_dev(dk.data_ptr(), m, stream=s.cuda_stream)


ms, sub, absent = timed(prefix_then_subgraph)
report("25% (prefix A)", m, ms, sub, absent, allk[(allk & 3) == 0])
sub.close()

# 100 %
packed = W.packed_of(allk[perm], k).contiguous()
ms, sub, absent = timed(lambda: t.subgraph_dev(packed.data_ptr(), packed.shape[0], stream=s.cuda_stream))
report("100%", packed.shape[0], ms, sub, absent, allk)
sub.close()
