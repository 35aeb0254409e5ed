"""CPU-side tests of the colour-set algebra (no GPU): the k_so_* kernels of bft_setops.hip are found and keep to registers, the four entry points are
declared and exported by libbft_gpu.so and the three annotation operations by libbft.so, a program that includes <bft/bft.h> and calls the three
operations and the three byte helpers compiles with -Wall -Werror as C and as C++ -- and runs: the operations work on host bytes alone, so their results
(the mode-0 byte image of cmp_annots) are checked here on hand-made annotations in all three modes --, and arguments the wrappers refuse before anything
touches a device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib
from bloomfiltertrie_amd.bft import BFT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"k_so_plan", "k_so_small", "k_so_wave", "k_so_split", "k_so_finish", "k_so_emit", "k_so_count"}
ABI = ("bft_gpu_combine_colors", "bft_gpu_combine_colors_dev", "bft_gpu_combine_colorsets", "bft_gpu_combine_colorsets_dev", "bft_gpu_debug_setops_plan")
OPS = ("intersection_annotations", "union_annotations", "sym_difference_annotations")

PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <bft/bft.h>

static BFT_annotation* make(const unsigned char* bytes, int n) {
    BFT_annotation* a = create_BFT_annotation();
    a->annot = (uint8_t*)malloc(n ? n : 1);
    memcpy(a->annot, bytes, n);
    a->size_annot = n;
    return a;
}
static void show(BFT_annotation* r) {
    if (r->annot_ext != NULL || r->annot_cplx != NULL) exit(4);
    printf("%d ", r->size_annot);
    for (int i = 0; i < r->size_annot; i++) printf("%02x", r->annot[i]);
    printf("\n");
    free_BFT_annotation(r);
}
int main(int argc, char** argv) {
    BFT bft;
    memset(&bft, 0, sizeof bft);
    bft.nb_genomes = atoi(argv[1]);
    /* {0, 3, 9} as a bitmap (mode 0: genome g at bit g + 2), {2 .. 9} as a range (mode 1), {3, 9, 70} as an id list (mode 2: 70 takes two bytes) */
    const unsigned char m0[2] = {0x24, 0x08}, m1[2] = {(2 << 2) | 1, (9 << 2) | 1}, m2[4] = {(3 << 2) | 2, (9 << 2) | 2, (1 << 2) | 2, (6 << 2) | 1};
    BFT_annotation *a = make(m0, 2), *b = make(m1, 2), *c = make(m2, 4);
    printf("%u %u %u\n", intersection_annots(0xF0, 0x3C), union_annots(0xF0, 0x3C), sym_difference_annots(0xF0, 0x3C));
    show(intersection_annotations(&bft, 1, a));
    show(intersection_annotations(&bft, 2, a, b));
    show(intersection_annotations(&bft, 3, a, b, c));
    show(union_annotations(&bft, 1, c));
    show(union_annotations(&bft, 3, a, b, c));
    show(sym_difference_annotations(&bft, 1, b));
    show(sym_difference_annotations(&bft, 2, a, b));
    show(sym_difference_annotations(&bft, 3, a, b, c));
    BFT_annotation* u = union_annotations(&bft, 2, a, c);
    show(intersection_annotations(&bft, 2, u, b)); /* a result as an argument */
    free_BFT_annotation(u);
    free_BFT_annotation(a);
    free_BFT_annotation(b);
    free_BFT_annotation(c);
    return 0;
}
"""


def _image(ids, genomes):
    """cmp_annots' result (src/annotation.c:2358-2551): mode 0, genome g at bit g + 2, MAX(CEIL(genomes + 2, 8), 1) bytes"""
    out = bytearray(max((genomes + 2 + 7) // 8, 1))
    for g in ids:
        if g < genomes:
            out[(g + 2) >> 3] |= 1 << ((g + 2) & 7)
    return f"{len(out)} {bytes(out).hex()}"


def test_setops_kernels_use_no_scratch():
    """Every k_so_* kernel (both row-width forms of the wavefront reductions): no scratch memory, no vector register spilled."""
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_so_"], capture_output=True, text=True).stdout
    seen, forms = set(), {"k_so_wave": set(), "k_so_split": set()}
    for line in out.splitlines()[1:]:
        if not line.strip():
            continue
        vgpr, sgpr, vspill, sspill, scratch, lds, maxwg, name = line.split(None, 7)
        m = re.search(r"(k_so_[a-z]+)(<(\w+)>)?", name)
        if not m or m.group(1) not in KERNELS:
            continue
        seen.add(m.group(1))
        if m.group(1) in forms:
            forms[m.group(1)].add(m.group(3))
        assert int(vspill) == 0 and int(scratch) == 0, line
    assert seen == KERNELS, seen
    assert forms == {"k_so_wave": {"true", "false"}, "k_so_split": {"true", "false"}}, forms


def test_setops_symbols_are_declared_and_exported():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name in ABI:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    for name, value in (("BFT_GPU_SETOP_AND", 0), ("BFT_GPU_SETOP_OR", 1), ("BFT_GPU_SETOP_SYMDIFF", 2)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", hdr), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(ABI) <= set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, "libbft.so")]).decode()
    for fn in OPS:
        assert re.search(r" T " + fn + "$", out, flags=re.M), fn
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bft", "bft.h")).read(), flags=re.S)
    for fn in OPS:  # (the reference's include/bft.h:112-114)
        assert re.search(r"\bBFT_annotation\s*\*\s*" + fn + r"\s*\(\s*BFT\s*\*\s*bft\s*,\s*uint32_t\s+nb_annotations\s*,\s*\.\.\.\s*\)\s*;", code), fn


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_a_program_with_the_six_calls_compiles_and_computes_on_the_host(lang, tmp_path):
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    src = tmp_path / ("prog.c" if lang == "c" else "prog.cpp")
    src.write_text(PROGRAM)
    exe = str(tmp_path / "prog")
    cc = ["gcc", "-std=gnu99"] if lang == "c" else ["g++", "-std=c++17"]
    subprocess.check_call(cc + ["-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src), "-L", _lib.CSRC, "-lbft",
                                f"-Wl,-rpath,{_lib.CSRC}", f"-Wl,-rpath-link,{_lib.CSRC}", "-Wl,-rpath-link,/opt/rocm/lib"])
    a, b, c = {0, 3, 9}, set(range(2, 10)), {3, 9, 70}
    for genomes in (10, 71, 6, 0):  # (6 and 0: ids at or past nb_genomes are dropped; the result is never shorter than a byte)
        r = subprocess.run([exe, str(genomes)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        want = [a, a & b, a & b & c, c, a | b | c, b, (a | b) - (a & b), (a | b | c) - (a & b & c), (a | c) & b]
        assert r.stdout.splitlines() == ["48 252 204"] + [_image(w, genomes) for w in want], genomes


def test_arguments_the_wrappers_refuse_without_a_device():
    lib = _lib.load()
    off = (C.c_uint64 * 3)(0, 1, 2)
    one = (C.c_uint8 * 64)()
    # NULL handle, NULL offsets, NULL batch, unknown op: refused before the handle is touched
    assert lib.bft_gpu_combine_colors(None, one, 2, off, 2, 0, 0, None, None, None) == -1
    assert "NULL" in lib.bft_gpu_last_error().decode()
    assert lib.bft_gpu_combine_colors(C.c_void_p(1), one, 2, None, 2, 0, 0, None, None, None) == -1
    assert lib.bft_gpu_combine_colors(C.c_void_p(1), None, 2, off, 2, 0, 0, None, None, None) == -1
    assert lib.bft_gpu_combine_colors(C.c_void_p(1), one, 2, off, 2, 3, 0, None, None, None) == -1
    assert "op" in lib.bft_gpu_last_error().decode()
    assert lib.bft_gpu_combine_colors_dev(None, one, 2, off, 2, 0, 0, None, None, None, None) == -1
    assert lib.bft_gpu_combine_colors_dev(C.c_void_p(1), one, 2, off, 2, -1, 0, None, None, None, None) == -1
    assert lib.bft_gpu_combine_colorsets(None, one, 2, off, 2, 0, None, None) == -1
    assert lib.bft_gpu_combine_colorsets(C.c_void_p(1), one, 2, off, 2, 9, None, None) == -1
    assert lib.bft_gpu_combine_colorsets_dev(None, one, 2, off, 2, 0, None, None, None) == -1
    # offsets that decrease, a last offset past the batch: before any device work
    bad = (C.c_uint64 * 3)(0, 2, 1)
    assert lib.bft_gpu_combine_colors(C.c_void_p(1), one, 2, bad, 2, 0, 0, None, None, None) == -1
    assert "decrease" in lib.bft_gpu_last_error().decode()
    far = (C.c_uint64 * 3)(0, 2, 3)
    assert lib.bft_gpu_combine_colorsets(C.c_void_p(1), one, 2, far, 2, 1, None, None) == -1
    assert "behind" in lib.bft_gpu_last_error().decode()
    # the Python wrappers' own checks
    assert [BFT._setop(x) for x in ("and", "or", "symdiff")] == [0, 1, 2]
    for op in ("xor", 0, None):
        with pytest.raises(ValueError):
            BFT._setop(op)
    assert BFT._group_off([0, 2, 2, 5], 5).dtype == np.uint64
    for off_, n in (([0, 3, 2], 5), ([0, 6], 5), ([], 5), ([[0, 1]], 5)):
        with pytest.raises(ValueError):
            BFT._group_off(off_, n)
