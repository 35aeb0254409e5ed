"""CPU-side tests of sub-graph builds (no GPU): the k_sg_* kernels are found and keep to registers, the new entry points are declared and
exported by libbft_gpu.so and libbft.so, and NULL arguments are refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess
import sys

from bloomfiltertrie_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_subgraph_kernels_use_no_scratch():
    """Every k_sg_* kernel (every key width / id width): no scratch memory, no vector register spilled to it."""
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_sg_"], capture_output=True, text=True).stdout
    seen = set()
    for line in out.splitlines()[1:]:
        if not line.strip():
            continue
        vgpr, sgpr, vspill, sspill, scratch, lds, maxwg, name = line.split(None, 7)
        m = re.search(r"(k_sg_[a-z]+)", name)
        if not m:
            continue
        seen.add(m.group(1))
        assert int(vspill) == 0 and int(scratch) == 0, line
    assert seen == {"k_sg_compact", "k_sg_scatter", "k_sg_mark", "k_sg_remap", "k_sg_dict"}, seen


def test_subgraph_symbols_are_declared_and_exported():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name in ("bft_gpu_subgraph", "bft_gpu_subgraph_dev"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert {"bft_gpu_subgraph", "bft_gpu_subgraph_dev"} <= set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))
    compat = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bft", "bft.h")).read(), flags=re.S)
    assert re.search(r"\bBFT\s*\*\s*create_cdbg_from_bft_kmers\s*\(\s*BFT_kmer\s*\*\*\s*bft_kmers\s*,\s*uint32_t\s+nb_bft_kmers\s*,\s*BFT\s*\*\s*bft\s*,\s*bool\s+add_colors\s*\)\s*;", compat)
    assert re.search(r"\bvoid\s+add_id_genomes\s*\(\s*BFT_kmer\s*\*\s*bft_kmer\s*,\s*BFT_annotation\s*\*\s*bft_annot\s*,\s*BFT\s*\*\s*bft\s*,\s*uint32_t\s*\*\s*list_id_genomes\s*\)\s*;", compat)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    assert re.search(r" T create_cdbg_from_bft_kmers$", out, flags=re.M) and re.search(r" T add_id_genomes$", out, flags=re.M)
    hdr_text = open(os.path.join(ROOT, "include", "bft", "bft.h")).read()
    not_provided = hdr_text[hdr_text.index("Not provided"):hdr_text.index("*/", hdr_text.index("Not provided"))]
    assert "create_cdbg_from_bft_kmers" not in not_provided and "add_id_genomes" not in not_provided


def test_null_arguments_are_refused_before_any_device_work():
    lib = _lib.load()
    out = C.c_void_p()
    absent = C.c_uint64()
    buf = (C.c_uint8 * 16)()
    assert lib.bft_gpu_subgraph(None, buf, 1, 1, C.byref(absent), C.byref(out)) == -1  # BFT_GPU_E_ARG
    assert lib.bft_gpu_subgraph(C.c_void_p(1), buf, 1, 1, C.byref(absent), None) == -1
    assert lib.bft_gpu_subgraph_dev(None, buf, 1, 0, None, C.byref(out), None) == -1
    assert lib.bft_gpu_subgraph_dev(C.c_void_p(1), buf, 1, 0, None, None, None) == -1
    assert lib.bft_gpu_subgraph(C.c_void_p(1), None, 1, 1, None, C.byref(out)) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
