"""CPU-side tests of the pan-genome k-mer classes (no GPU): the k_pg_* kernels of bft_pangenome.hip are found and keep to registers at every key
width, the four entry points are declared and exported by libbft_gpu.so, the class snippets by libbft.so with the reference's signatures, and NULL
arguments are refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess
import sys

from bloomfiltertrie_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_pg_emit", "k_pg_usage", "k_pg_dict"}
ABI = ("bft_gpu_kmers_by_count", "bft_gpu_kmers_by_count_dev", "bft_gpu_pangenome_stats", "bft_gpu_pangenome_stats_dev")
CALLBACKS = ("extract_core_kmers", "extract_dispensable_kmers", "extract_singleton_kmers")


def test_pangenome_kernels_use_no_scratch():
    """Every k_pg_* kernel (every key width of the emission, both forms of the dictionary pass): no scratch memory, no vector register spilled."""
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_pg_"], capture_output=True, text=True).stdout
    seen, widths, dicts = set(), set(), set()
    for line in out.splitlines()[1:]:
        if not line.strip():
            continue
        vgpr, sgpr, vspill, sspill, scratch, lds, maxwg, name = line.split(None, 7)
        m = re.search(r"(k_pg_[a-z]+)(<(\w+)>)?", name)
        if not m or m.group(1) not in KERNELS:
            continue
        seen.add(m.group(1))
        if m.group(1) == "k_pg_emit":
            widths.add(int(m.group(3)))
        if m.group(1) == "k_pg_dict":
            dicts.add(m.group(3))
        assert int(vspill) == 0 and int(scratch) == 0, line
    assert seen == KERNELS, seen
    assert widths == {1, 2, 3, 4}, widths
    assert dicts == {"true", "false"}, dicts


def test_pangenome_symbols_are_declared_and_exported():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name in ABI:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(ABI) <= set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))


def test_class_snippets_are_exported_with_the_reference_signatures():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bft", "snippets_pangenome.h")).read(), flags=re.S)
    # (the reference's include/snippets.h:38-41)
    for fn in CALLBACKS:
        assert re.search(r"\bsize_t\s+" + fn + r"\s*\(\s*BFT_kmer\s*\*\s*kmer\s*,\s*BFT\s*\*\s*graph\s*,\s*va_list\s+args\s*\)\s*;", code), fn
    assert re.search(r"\bvoid\s+extract_pangenome_kmers_to_disk\s*\(\s*BFT\s*\*\s*graph\s*,\s*char\s*\*\s*filename_output\s*,\s*BFT_func_ptr\s+f\s*\)\s*;", code)
    assert set(re.findall(r"\b([a-zA-Z_]\w*)\s*\([^()]*\)\s*;", code)) == set(CALLBACKS) | {"extract_pangenome_kmers_to_disk"}
    snippets = open(os.path.join(ROOT, "include", "bft", "snippets.h")).read()
    assert '#include "snippets_pangenome.h"' in snippets
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    for fn in CALLBACKS + ("extract_pangenome_kmers_to_disk",):
        assert re.search(r" T " + fn + "$", out, flags=re.M), fn
    # (the callbacks are told apart by address: libbft.so must take them from its GOT, not bind them to itself)
    dyn = subprocess.check_output(["readelf", "-d", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    assert "SYMBOLIC" not in dyn
    # <bft/snippets.h> alone compiles as C, and declares the four
    subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"],
                   input=b"#include <bft/snippets.h>\nBFT_func_ptr f[3] = {extract_core_kmers, extract_dispensable_kmers, extract_singleton_kmers};\n"
                         b"void (*g)(BFT*, char*, BFT_func_ptr) = extract_pangenome_kmers_to_disk;\nint main(void) { return 0; }\n", check=True)


def test_null_arguments_are_refused_before_any_device_work():
    lib = _lib.load()
    n = C.c_uint64()
    cnt = (C.c_uint64 * 1)()
    assert lib.bft_gpu_kmers_by_count(None, 1, 1, None, None, None, 0, C.byref(n)) == -1  # BFT_GPU_E_ARG
    assert lib.bft_gpu_kmers_by_count(C.c_void_p(1), 1, 1, None, None, None, 0, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
    assert lib.bft_gpu_kmers_by_count_dev(None, 1, 1, None, None, None, 0, cnt, None) == -1
    assert lib.bft_gpu_kmers_by_count_dev(C.c_void_p(1), 1, 1, None, None, None, 0, None, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
    assert lib.bft_gpu_pangenome_stats(None, None, None, None, 0) == -1
    assert lib.bft_gpu_pangenome_stats_dev(None, None, None, None, 0, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
