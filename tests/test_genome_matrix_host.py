"""CPU-side tests of the genome-by-genome shared k-mer matrix (no GPU): the four entry points are declared, exported and bound, the test hooks are
exported and bound but not declared, every k_gm_* kernel of bft_genome_matrix.hip keeps to registers and one of them is the matrix-core kernel, NULL
arguments are refused before anything touches a device, and BFT.genome_distances' metrics on hand-made matrices."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from bloomfiltertrie_amd import BFT, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_gm_usage_ids", "k_gm_weights", "k_gm_plan", "k_gm_sparse", "k_gm_clear", "k_gm_bits", "k_gm_dense_mfma"}
ABI = ("bft_gpu_genome_matrix", "bft_gpu_genome_matrix_dev", "bft_gpu_genome_matrix_colorsets", "bft_gpu_genome_matrix_colorsets_dev")
HOOKS = ("bft_gpu_test_genome_matrix", "bft_gpu_test_genome_matrix_state")


def test_genome_matrix_kernels_use_no_scratch_and_one_is_the_mfma_kernel():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_gm_"], capture_output=True, text=True).stdout
    seen, sparse = set(), set()
    for line in out.splitlines()[1:]:
        if not line.strip():
            continue
        vgpr, sgpr, vspill, sspill, scratch, lds, maxwg, name = line.split(None, 7)
        m = re.search(r"(k_gm_[a-z_]+)(<(\w+)>)?", name)
        assert m and m.group(1) in KERNELS, line  # (a new k_gm_* kernel is named here)
        seen.add(m.group(1))
        if m.group(1) == "k_gm_sparse":
            sparse.add(m.group(3))
            assert (int(lds) > 0) == (m.group(3) == "true"), line  # the LDS triangle and the form without it
        assert int(vspill) == 0 and int(scratch) == 0, line
    assert seen == KERNELS, seen
    assert sparse == {"true", "false"}, sparse
    assert any("mfma" in k for k in seen)  # the marker in the kernel's name ...
    # ... and the instruction in the unit's code
    asm = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-o", "-",
                          os.path.join(_lib.CSRC, "bft_genome_matrix.hip")], capture_output=True, text=True, check=True).stdout
    body = asm[asm.index("k_gm_dense_mfma"):]
    assert "v_mfma_i32_16x16x64_i8" in body
    assert "ds_add_u64" in asm  # the sparse road's LDS triangle counts in 64 bits


def test_genome_matrix_symbols_are_declared_exported_and_bound():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    raw = open(_lib.HEADER).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ABI:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and name not in _lib.TEST_HOOKS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))
    assert set(ABI) | set(HOOKS) <= exported
    for name in HOOKS:
        assert name in _lib.TEST_HOOKS and name not in _lib.SIGNATURES
        assert name not in raw
    assert re.search(r"#define\s+BFT_GPU_GENOME_MATRIX_MAX_GENOMES\s+(\d+)u", hdr)
    assert int(re.search(r"#define\s+BFT_GPU_GENOME_MATRIX_MAX_GENOMES\s+(\d+)u", hdr).group(1)) >= 4200
    for method in ("genome_matrix", "genome_matrix_colorsets", "genome_matrix_dev", "genome_matrix_colorsets_dev", "genome_distances"):
        assert callable(getattr(BFT, method))


def test_null_arguments_are_refused_before_any_device_work():
    lib = _lib.load()
    g = C.c_uint32()
    buf = (C.c_uint64 * 4)()
    ids = (C.c_uint32 * 4)()
    one = C.c_void_p(1)  # (never dereferenced: the other argument is refused first)
    assert lib.bft_gpu_genome_matrix(None, 0, 1, buf, 4, C.byref(g)) == -1  # BFT_GPU_E_ARG
    assert lib.bft_gpu_genome_matrix(one, 0, 1, buf, 4, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
    assert lib.bft_gpu_genome_matrix_dev(None, 0, 1, buf, 4, None) == -1
    assert lib.bft_gpu_genome_matrix_dev(one, 0, 1, None, 4, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
    assert lib.bft_gpu_genome_matrix_colorsets(None, ids, 4, buf, 4, C.byref(g)) == -1
    assert lib.bft_gpu_genome_matrix_colorsets(one, ids, 4, buf, 4, None) == -1
    assert lib.bft_gpu_genome_matrix_colorsets(one, None, 4, buf, 4, C.byref(g)) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
    assert lib.bft_gpu_genome_matrix_colorsets_dev(None, ids, 4, buf, 4, None) == -1
    assert lib.bft_gpu_genome_matrix_colorsets_dev(one, ids, 4, None, 4, None) == -1
    assert lib.bft_gpu_genome_matrix_colorsets_dev(one, None, 4, buf, 4, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
    # the batch's size limit is checked before the handle is touched, too
    assert lib.bft_gpu_genome_matrix_colorsets(one, ids, 1 << 31, buf, 4, C.byref(g)) == -3  # BFT_GPU_E_LIMIT
    assert lib.bft_gpu_genome_matrix_colorsets_dev(one, ids, 1 << 31, buf, 4, None) == -3
    assert lib.bft_gpu_test_genome_matrix(None, ids, 1, 0, buf, 4, None) == -1
    assert lib.bft_gpu_test_genome_matrix(one, None, 1, 0, buf, 4, None) == -1
    assert lib.bft_gpu_test_genome_matrix(one, ids, 1, 0, None, 4, None) == -1
    assert lib.bft_gpu_test_genome_matrix(one, ids, 3, 0, buf, 4, None) == -1
    out = (C.c_uint32 * 2)()
    assert lib.bft_gpu_test_genome_matrix_state(None, 0, out) == -1
    assert lib.bft_gpu_test_genome_matrix_state(one, 0, None) == -1


def test_distances_on_hand_made_matrices():
    k = 27
    # genome 0 and 1 identical (10 k-mers), genome 2 disjoint from both (5), genome 3 empty, genome 4 shares 4 of its 8 with genome 0 and 1
    m = np.array([[10, 10, 0, 0, 4],
                  [10, 10, 0, 0, 4],
                  [0, 0, 5, 0, 0],
                  [0, 0, 0, 0, 0],
                  [4, 4, 0, 0, 8]], dtype=np.uint64)
    jac = BFT.distances_from_matrix(m, "jaccard", k)
    want = np.array([[1, 1, 0, 0, 4 / 14],
                     [1, 1, 0, 0, 4 / 14],
                     [0, 0, 1, 0, 0],
                     [0, 0, 0, 0, 0],  # the empty genome: an empty union with itself gives 0.0
                     [4 / 14, 4 / 14, 0, 0, 1]])
    assert jac.dtype == np.float64 and np.array_equal(jac, want)
    con = BFT.distances_from_matrix(m, "containment", k)
    assert np.array_equal(con, np.array([[1, 1, 0, 0, 0.4], [1, 1, 0, 0, 0.4], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0], [0.5, 0.5, 0, 0, 1]]))
    mash = BFT.distances_from_matrix(m, "mash", k)
    assert mash[0, 1] == 0.0 and mash[0, 0] == 0.0 and not np.signbit(mash[0, 1])  # identical genomes
    assert mash[0, 2] == 1.0 and mash[2, 0] == 1.0  # J = 0 gives 1.0
    assert mash[3, 3] == 1.0 and mash[3, 0] == 1.0  # the empty genome
    j = 4 / 14
    assert mash[0, 4] == pytest.approx(-math.log(2 * j / (1 + j)) / k, rel=1e-15)
    assert np.array_equal(mash, mash.T) and np.array_equal(jac, jac.T)
    # the cap at 1.0: with k = 1 a small J passes it
    assert BFT.distances_from_matrix(np.array([[100, 1], [1, 100]], dtype=np.uint64), "mash", 1)[0, 1] == 1.0
    assert BFT.distances_from_matrix(np.zeros((0, 0), dtype=np.uint64), "jaccard", k).shape == (0, 0)
    with pytest.raises(ValueError):
        BFT.distances_from_matrix(m, "hamming", k)
