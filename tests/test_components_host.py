"""CPU-side tests of connected components (no GPU): the k_cc_* kernels of bft_components.hip are found and keep to registers at every key
width, the new entry points are declared and exported by libbft_gpu.so, the traversal snippets by libbft.so with the reference's signatures,
and bad arguments are refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from bloomfiltertrie_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_cc_sets", "k_cc_init", "k_cc_hook", "k_cc_flatten", "k_cc_label", "k_cc_count", "k_cc_sizes"}


def test_component_kernels_use_no_scratch():
    """Every k_cc_* kernel (every key width): no scratch memory, no vector register spilled to it."""
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_cc_"], capture_output=True, text=True).stdout
    seen, hooks = set(), set()
    for line in out.splitlines()[1:]:
        if not line.strip():
            continue
        vgpr, sgpr, vspill, sspill, scratch, lds, maxwg, name = line.split(None, 7)
        m = re.search(r"(k_cc_[a-z]+)(<(\d)>)?", name)
        if not m or m.group(1) not in KERNELS:
            continue
        seen.add(m.group(1))
        if m.group(1) == "k_cc_hook":
            hooks.add(int(m.group(3)))
        assert int(vspill) == 0 and int(scratch) == 0 and int(lds) == 0, line
    assert seen == KERNELS, seen
    assert hooks == {1, 2, 3, 4}, hooks


def test_component_symbols_are_declared_and_exported():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name in ("bft_gpu_components", "bft_gpu_components_dev"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert {"bft_gpu_components", "bft_gpu_components_dev"} <= set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))


def test_traversal_snippets_are_exported_with_the_reference_signatures():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bft", "snippets_traversal.h")).read(), flags=re.S)
    for fn in ("BFS", "BFS_subgraph", "DFS", "DFS_subgraph"):
        assert re.search(r"\bsize_t\s+" + fn + r"\s*\(\s*BFT_kmer\s*\*\s*kmer\s*,\s*BFT\s*\*\s*graph\s*,\s*va_list\s+args\s*\)\s*;", code), fn
    assert re.search(r"\bbool\s+is_in_subgraph\s*\(\s*BFT_kmer\s*\*\s*kmer\s*,\s*BFT\s*\*\s*graph\s*,\s*int\s+nb_id_genomes\s*,\s*const\s+va_list\s+args\s*\)\s*;", code)
    assert re.search(r"\bvoid\s+get_nb_connected_component\s*\(\s*BFT\s*\*\s*graph\s*,\s*\.\.\.\s*\)\s*;", code)
    assert '#include "snippets_traversal.h"' in open(os.path.join(ROOT, "include", "bft", "snippets.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    for fn in ("BFS", "BFS_subgraph", "DFS", "DFS_subgraph", "is_in_subgraph", "get_nb_connected_component"):
        assert re.search(r" T " + fn + "$", out, flags=re.M), fn
    # (the traversals are told apart by address: libbft.so must take them from its GOT, not bind them to itself)
    dyn = subprocess.check_output(["readelf", "-d", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    assert "SYMBOLIC" not in dyn
    subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"],
                   input=b"#include <bft/snippets.h>\nint main(void) { return 0; }\n", check=True)


def test_bad_arguments_are_refused_before_any_device_work():
    lib = _lib.load()
    cnt = np.zeros(3, dtype=np.uint64)
    ids = np.array([1, 2], dtype=np.uint32)
    dup = np.array([2, 2], dtype=np.uint32)
    down = np.array([2, 1], dtype=np.uint32)
    assert lib.bft_gpu_components(None, None, 0, None, 0, None, 0, cnt.ctypes.data) == -1  # BFT_GPU_E_ARG
    assert lib.bft_gpu_components(C.c_void_p(1), None, 0, None, 0, None, 0, None) == -1
    assert lib.bft_gpu_components(C.c_void_p(1), None, 2, None, 0, None, 0, cnt.ctypes.data) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
    assert lib.bft_gpu_components(C.c_void_p(1), dup.ctypes.data, 2, None, 0, None, 0, cnt.ctypes.data) == -1
    assert lib.bft_gpu_components(C.c_void_p(1), down.ctypes.data, 2, None, 0, None, 0, cnt.ctypes.data) == -1
    assert "increasing" in lib.bft_gpu_last_error().decode()
    assert lib.bft_gpu_components_dev(None, None, 0, None, None, 0, cnt.ctypes.data, None) == -1
    assert lib.bft_gpu_components_dev(C.c_void_p(1), None, 0, None, None, 0, None, None) == -1
    assert lib.bft_gpu_components_dev(C.c_void_p(1), ids.ctypes.data, 0, None, None, 0, None, None) == -1
    assert lib.bft_gpu_components_dev(C.c_void_p(1), dup.ctypes.data, 2, None, None, 0, cnt.ctypes.data, None) == -1
    assert "increasing" in lib.bft_gpu_last_error().decode()
