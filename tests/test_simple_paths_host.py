"""CPU-side tests of simple paths (no GPU): the k_sp_* kernels are found and keep to registers, the new entry points are declared and exported
by libbft_gpu.so, the snippets by libbft.so with the reference's signatures, and NULL arguments are refused before anything touches a device."""
import ctypes as C
import os
import re
import subprocess
import sys

from bloomfiltertrie_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_sp_buckets", "k_sp_degrees", "k_sp_links", "k_sp_jump", "k_sp_ends", "k_sp_offsets", "k_sp_spell"}


def test_simple_path_kernels_use_no_scratch():
    """Every k_sp_* kernel (every key width): no scratch memory, no vector register spilled to it."""
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_sp_"], capture_output=True, text=True).stdout
    seen = set()
    for line in out.splitlines()[1:]:
        if not line.strip():
            continue
        vgpr, sgpr, vspill, sspill, scratch, lds, maxwg, name = line.split(None, 7)
        m = re.search(r"(k_sp_[a-z]+)", name)
        if not m:
            continue
        seen.add(m.group(1))
        assert int(vspill) == 0 and int(scratch) == 0, line
    assert seen == KERNELS, seen


def test_simple_path_symbols_are_declared_and_exported():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name in ("bft_gpu_simple_paths", "bft_gpu_simple_paths_dev"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert {"bft_gpu_simple_paths", "bft_gpu_simple_paths_dev"} <= set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))


def test_snippets_are_exported_with_the_reference_signatures():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    path = os.path.join(ROOT, "include", "bft", "snippets.h")
    text = open(path).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    # (the reference's include/snippets.h: void extract_simple_paths_to_disk(BFT* graph, char* filename_output); and the core form)
    assert re.search(r"\bvoid\s+extract_simple_paths_to_disk\s*\(\s*BFT\s*\*\s*graph\s*,\s*char\s*\*\s*filename_output\s*\)\s*;", code)
    assert re.search(r"\bvoid\s+extract_simple_core_paths_to_disk\s*\(\s*BFT\s*\*\s*graph\s*,\s*double\s+core_ratio\s*,\s*char\s*\*\s*filename_output\s*\)\s*;", code)
    assert set(re.findall(r"\b([a-zA-Z_]\w*)\s*\([^()]*\)\s*;", code)) == {"extract_simple_paths_to_disk", "extract_simple_core_paths_to_disk"}
    for absent in ("extract_simple_paths", "extract_core_simple_paths", "extract_core_kmers", "BFS", "DFS", "get_nb_connected_component"):
        assert absent in text  # (named as not provided)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    assert re.search(r" T extract_simple_paths_to_disk$", out, flags=re.M) and re.search(r" T extract_simple_core_paths_to_disk$", out, flags=re.M)
    # the header compiles on its own, as C
    subprocess.run(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), "-"],
                   input=b"#include <bft/snippets.h>\nint main(void) { return 0; }\n", check=True)


def test_null_arguments_are_refused_before_any_device_work():
    lib = _lib.load()
    n1, n2 = C.c_uint64(), C.c_uint64()
    cnt = (C.c_uint64 * 3)()
    assert lib.bft_gpu_simple_paths(None, 0, None, None, 0, 0, C.byref(n1), C.byref(n2)) == -1  # BFT_GPU_E_ARG
    assert lib.bft_gpu_simple_paths(C.c_void_p(1), 0, None, None, 0, 0, None, C.byref(n2)) == -1
    assert lib.bft_gpu_simple_paths(C.c_void_p(1), 0, None, None, 0, 0, C.byref(n1), None) == -1
    assert lib.bft_gpu_simple_paths_dev(None, 0, None, None, 0, 0, cnt, None) == -1
    assert lib.bft_gpu_simple_paths_dev(C.c_void_p(1), 0, None, None, 0, 0, None, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
