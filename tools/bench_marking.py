#!/usr/bin/env python3
"""Vertex marking (set_marking / set_flag_kmer / get_flag_kmer and the traversals' marks, reference src/bft.c:686-765, src/snippets.c:605-812)
through the resident bft_gpu_marks_* calls on the config-3 index (100 genomes, k = 27, workloads.PanGenome), each beside a number of the same run:
  - set (one flag), set (a flag per k-mer), get and test-and-set of a resident batch of stored k-mers drawn with repetition (10^8 by default), beside
    the two resident queries of the same batch there are: presence (the k-mer hash) and colour rows (the row lookup the marks use, plus a row gather);
  - fill, counts and select over the whole flag array;
  - a first reach from one seed (union-find + painting) beside bft_gpu_components_dev, and a second reach with the same key, which finds the forest
    on the handle (its seed is painted by then: lookup, seeding and the painting pass, no union-find).
One JSON line per measurement.  usage: bench_marking.py [batch k-mers] [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bloomfiltertrie_amd import BFT, workloads as W  # noqa: E402

n_batch = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda", 0)
st = torch.cuda.current_stream().cuda_stream


def timed(call, n=reps, before=None):
    """ms per call between HIP events, after one warm-up call; `before` (untimed) restores the state in front of every call"""
    if before:
        before()
    call()
    torch.cuda.synchronize()
    total = 0.0
    for _ in range(n):
        if before:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1)
    return total / n


def line(what, ms, n=None, **kw):
    out = {"index": "config3", "what": what, "ms": round(ms, 3)}
    if n:
        out["kmers_per_s"] = round(n / (ms / 1e3), 1)
    out.update(kw)
    print(json.dumps(out), flush=True)


t0 = time.perf_counter()
pan = W.PanGenome(100, 2_000_000, 0.01, 4242, dev)
t = BFT(27)
W.build_index(t, pan, 27)
n_kmers = int(t.info()["kmers"])
print(json.dumps({"index": "config3", "kmers": n_kmers, "setup_s": round(time.perf_counter() - t0, 1)}), flush=True)

stored = torch.from_numpy(t.extract()[0]).to(dev)
batch = stored[torch.randint(0, n_kmers, (n_batch,), device=dev)].contiguous()
flags = torch.randint(0, 4, (n_batch,), dtype=torch.uint8, device=dev)
out8 = torch.zeros(n_batch, dtype=torch.uint8, device=dev)
bits = torch.zeros((n_batch + 63) // 64 * 8, dtype=torch.uint8, device=dev)
t.set_marking()

# the neighbours of the batch calls
line("query_presence_dev (k-mer hash)", timed(lambda: t.query_presence_dev(batch.data_ptr(), n_batch, bits.data_ptr(), st)), n_batch)
rowbytes = (100 + 7) // 8
crow = torch.zeros(n_batch * rowbytes, dtype=torch.uint8, device=dev)
scr = torch.zeros(n_batch, dtype=torch.int32, device=dev)
line("query_color_rows_dev (row lookup + row gather)",
     timed(lambda: t.query_color_rows_dev(batch.data_ptr(), n_batch, bits.data_ptr(), crow.data_ptr(), scr.data_ptr(), st)), n_batch)
del crow, scr

line("marks_set_dev, one flag", timed(lambda: t.set_flags_dev(batch.data_ptr(), n_batch, flag=2, stream=st)), n_batch)
line("marks_set_dev, a flag per k-mer", timed(lambda: t.set_flags_dev(batch.data_ptr(), n_batch, d_flags_ptr=flags.data_ptr(), stream=st)), n_batch)
line("marks_get_dev", timed(lambda: t.get_flags_dev(batch.data_ptr(), n_batch, out8.data_ptr(), stream=st)), n_batch)
ms = timed(lambda: t.test_and_set_dev(batch.data_ptr(), n_batch, 0, 1, out8.data_ptr(), stream=st), before=lambda: t.fill_flags_dev(0, stream=st))
line("marks_test_and_set_dev (every flag 0 before)", ms, n_batch, winners=int(out8.sum().item()))

cnt4 = torch.zeros(4, dtype=torch.int64, device=dev)
line("marks_fill_dev", timed(lambda: t.fill_flags_dev(1, stream=st)), n_kmers)
line("marks_counts_dev", timed(lambda: t.flag_counts_dev(cnt4.data_ptr(), stream=st)), n_kmers, counts=cnt4.cpu().tolist())
nsel = torch.zeros(1, dtype=torch.int64, device=dev)
sel = torch.zeros(n_kmers, dtype=torch.int32, device=dev)
line("marks_select_dev (rows of every k-mer)", timed(lambda: t.select_flagged_dev(0b0010, 0, 0, sel.data_ptr(), n_kmers, nsel.data_ptr(), stream=st)), n_kmers,
     selected=int(nsel.item()))

# reach: the union-find of the whole graph beside bft_gpu_components_dev, then a reach that finds the forest
ccnt = torch.zeros(3, dtype=torch.int64, device=dev)
line("components_dev (count only)", timed(lambda: t.components_dev(0, 0, 0, ccnt.data_ptr(), stream=st)), n_kmers, components=int(ccnt[0].item()))
seed = stored[n_kmers // 2:n_kmers // 2 + 1].contiguous()
rcnt = torch.zeros(3, dtype=torch.int64, device=dev)
new = torch.zeros(1, dtype=torch.uint8, device=dev)
ms = timed(lambda: t.reach_dev(seed.data_ptr(), 1, new.data_ptr(), rcnt.data_ptr(), stream=st), before=lambda: t.fill_flags_dev(0, stream=st))
line("marks_reach_dev, first (forest built)", ms, n_kmers, painted=int(rcnt[0].item()))
# (the last timed reach left the forest of (through 0, no ids) on the handle and everything it reaches painted: the same call again keeps the key,
# skips the union-find and paints nothing)
ms = timed(lambda: t.reach_dev(seed.data_ptr(), 1, new.data_ptr(), rcnt.data_ptr(), stream=st))
line("marks_reach_dev, second (forest on the handle, seed already painted)", ms, n_kmers, painted=int(rcnt[0].item()))
t.close()
