#!/usr/bin/env python3
"""Batched prefix matching (prefix_matching, src/bft.c:1087-1147) through bft_gpu_query_prefixes_dev on the config-3 index (100 genomes,
k = 27, workloads.PanGenome): resident prefixes and lengths, offsets / k-mers / rows / colour sets in HBM, HIP events around the calls after a
warm-up call of the same shape.
  (a) lookup-bound: 10^7 prefixes of length k - 1 taken from stored k-mers (at most 4 matches each) -> M prefixes/s
  (b) output-bound: the 256 prefixes of length 4 -> every stored k-mer once; GB/s of the bytes the answer needs (the table and the colour
      set per k-mer read once, k-mer + row + colour set written per match) and of the bytes the kernels move (the 4 candidate rows per
      match the length-4 filter reads in two passes, plus the emit) -- to be set beside tools/microbench/stream's copy rate
Each batch is checked against ground truth (the inserted k-mers): match counts of every prefix, and the k-mers of a slice.
usage: bench_prefix.py [n_prefixes_a] [reps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from bloomfiltertrie_amd import BFT, workloads as W  # noqa: E402

na = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
k = 27
nb = (2 * k + 7) // 8
dev = torch.device("cuda", 0)
pan = W.PanGenome(100, 2_000_000, 0.01, 4242, dev)
t = BFT(k)
keys, _ = W.build_index(t, pan, k)
allk = W.union_of(keys)  # sorted distinct int64 keys: nucleotide j at bits 2j
n_kmers = allk.numel()
st = torch.cuda.current_stream().cuda_stream


def run(pref, lens):
    n = lens.numel()
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    need = torch.zeros(1, dtype=torch.int64, device=dev)
    t.query_prefixes_dev(pref.data_ptr(), lens.data_ptr(), n, off.data_ptr(), 0, 0, 0, 0, need.data_ptr(), st)  # the size first
    torch.cuda.synchronize()
    m = int(need.item())
    km = torch.zeros((max(m, 1), nb), dtype=torch.uint8, device=dev)
    rows = torch.zeros(max(m, 1), dtype=torch.int32, device=dev)
    cs = torch.zeros(max(m, 1), dtype=torch.int32, device=dev)
    call = lambda: t.query_prefixes_dev(pref.data_ptr(), lens.data_ptr(), n, off.data_ptr(), km.data_ptr(), rows.data_ptr(), cs.data_ptr(), m,
                                        need.data_ptr(), st)
    call()  # warm-up of the timed shape
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, off, km[:m], rows[:m], cs[:m], m


def counts_truth(masked_sorted, q):
    return torch.searchsorted(masked_sorted, q, right=True) - torch.searchsorted(masked_sorted, q, right=False)


def slice_ok(off, km, rows, qmask, mask, n_check):
    """prefixes [0, n_check): every k-mer is stored and starts with its prefix, rows ascend inside a prefix"""
    end = int(off[n_check].item())
    if end == 0:
        return True
    cnt = (off[1:n_check + 1] - off[:n_check])
    owner = torch.repeat_interleave(torch.arange(n_check, device=dev), cnt)
    kk = W.keys_of(km[:end])
    ok = bool(W.member(allk, kk).all().item()) and bool(((kk & mask) == qmask[owner]).all().item())
    same = owner[1:] == owner[:-1]
    r = rows[:end].to(torch.int64)
    return ok and bool((r[1:][same] > r[:-1][same]).all().item())


# (a) 10^7 prefixes of length k - 1 from stored k-mers
g = torch.Generator(device=dev)
g.manual_seed(7)
idx = torch.randint(0, n_kmers, (na,), generator=g, device=dev)
qa = allk[idx]
mask_a = (1 << (2 * (k - 1))) - 1
pref_a = W.packed_of(qa, k)
lens_a = torch.full((na,), k - 1, dtype=torch.uint8, device=dev)
ms_a, off_a, km_a, rows_a, cs_a, m_a = run(pref_a, lens_a)
masked = torch.sort(allk & mask_a).values
ok_a = bool(((off_a[1:] - off_a[:-1]) == counts_truth(masked, qa & mask_a)).all().item()) and slice_ok(off_a, km_a, rows_a, qa & mask_a, mask_a, 20000)

# (b) the 256 prefixes of length 4: the whole table
qb = torch.arange(256, dtype=torch.int64, device=dev)
pref_b = torch.zeros((256, nb), dtype=torch.uint8, device=dev)
pref_b[:, 0] = qb.to(torch.uint8)
lens_b = torch.full((256,), 4, dtype=torch.uint8, device=dev)
ms_b, off_b, km_b, rows_b, cs_b, m_b = run(pref_b.contiguous(), lens_b)
ok_b = m_b == n_kmers and bool(((off_b[1:] - off_b[:-1]) == torch.bincount(allk & 255, minlength=256)).all().item())
ok_b = ok_b and slice_ok(off_b, km_b, rows_b, qb, 255, 16)
need_bytes = n_kmers * (8 + 4) + m_b * (nb + 4 + 4)  # table + colour set per k-mer read once; k-mer, row, colour set written
moved_bytes = 2 * 4 * n_kmers * 8 + m_b * (8 + 4) + m_b * (nb + 4 + 4)  # two passes over 4 candidates per match, emit's reads, the writes
print(json.dumps({
    "workload": "config-3 index (100 genomes, k = 27): bft_gpu_query_prefixes_dev, resident in and out",
    "kmers": n_kmers,
    "a_prefixes": na, "a_length": k - 1, "a_matches": m_a, "a_ms": round(ms_a, 3), "a_M_prefixes_per_s": round(na / ms_a / 1e3, 1),
    "b_prefixes": 256, "b_length": 4, "b_matches": m_b, "b_ms": round(ms_b, 3),
    "b_GBps_needed_bytes": round(need_bytes / ms_b / 1e6, 1), "b_GBps_moved_bytes": round(moved_bytes / ms_b / 1e6, 1),
    "reps": reps, "ground_truth_ok": bool(ok_a and ok_b)}))
