"""CPU-side tests of batched prefix matching (no GPU): the range rule the k_pm_* kernels share with the host (bft_prefix_range,
csrc/bft_walk.h) against brute force, the new entry points are declared and exported, and the kernels keep to registers."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from bloomfiltertrie_amd import _lib, synth as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (9, 10, 17, 27, 31, 36, 63, 64, 72, 80, 90, 126)


@pytest.fixture(scope="module")
def hostlib():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(os.path.join(_lib.CSRC, "libbft_hosttest.so"))
    lib.bft_hosttest_roundtrip.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    lib.bft_hosttest_prefix_range.restype = C.c_uint64
    lib.bft_hosttest_prefix_range.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return lib


def _tform_ints(hostlib, packed, k):
    W = (2 * k + 63) // 64
    out = np.zeros_like(packed)
    tf = np.zeros(len(packed) * W, dtype=np.uint64)
    hostlib.bft_hosttest_roundtrip(packed.ctypes.data, len(packed), k, out.ctypes.data, tf.ctypes.data)
    assert (out == packed).all()
    return [sum(int(w) << (64 * (W - 1 - j)) for j, w in enumerate(tf[i * W:(i + 1) * W])) for i in range(len(packed))]


def _ranges(hostlib, prefixes, lens, k):
    W = (2 * k + 63) // 64
    n = len(prefixes)
    lo = np.zeros(n * W, dtype=np.uint64)
    hi = np.zeros(n * W, dtype=np.uint64)
    fsh = np.zeros(n, dtype=np.int32)
    fval = np.zeros(n, dtype=np.uint32)
    lens = np.ascontiguousarray(lens, dtype=np.uint8)
    ok = hostlib.bft_hosttest_prefix_range(prefixes.ctypes.data, lens.ctypes.data, n, k, lo.ctypes.data, hi.ctypes.data, fsh.ctypes.data, fval.ctypes.data)
    to_int = lambda a, i: sum(int(w) << (64 * (W - 1 - j)) for j, w in enumerate(a[i * W:(i + 1) * W]))
    return ok, [(to_int(lo, i), to_int(hi, i), int(fsh[i]), int(fval[i])) for i in range(n)]


def _matches(rule, tf):
    lo, hi, fsh, fval = rule
    hit = (tf >= lo) & (tf <= hi)
    if fsh >= 0:
        hit &= ((tf >> fsh) & 3) == fval
    return hit.astype(bool)


@pytest.mark.parametrize("k", KS)
def test_range_rule_matches_brute_force(hostlib, k):
    """For every length 1..k: a k-mer's T-form lies in [lo, hi] and passes the filter exactly when its first len nucleotides are the
    prefix's.  The k-mers are the prefixes themselves, random ones, k-mers sharing a prefix with them and near misses of those (one
    nucleotide changed) and, for short k, all 4^5 heads in front of one prefix's tail; the prefixes carry garbage past their length."""
    rng = np.random.default_rng(k)
    n_pref = 6
    codes = rng.integers(0, 4, (n_pref, k), dtype=np.uint8)
    kmer_codes = [codes, rng.integers(0, 4, (40, k), dtype=np.uint8)]
    for p in codes:  # k-mers that share a prefix of many lengths with p, and near misses of them
        for cut in range(1, k + 1, max(1, k // 10)):
            c = rng.integers(0, 4, (3, k), dtype=np.uint8)
            c[:, :cut] = p[:cut]
            kmer_codes.append(c)
            if cut:
                d = c.copy()
                j = rng.integers(0, cut)
                d[:, j] = (d[:, j] + 1 + rng.integers(0, 3)) % 4
                kmer_codes.append(d)
    if k <= 10:  # exhaustive over the first 5 positions
        heads = np.array(np.meshgrid(*[np.arange(4, dtype=np.uint8)] * 5, indexing="ij")).reshape(5, -1).T
        e = np.repeat(codes[:1], len(heads), axis=0)
        e[:, :5] = heads
        kmer_codes.append(e)
    kc = np.concatenate(kmer_codes)
    kp = S.pack_codes(kc)
    tf = np.array(_tform_ints(hostlib, kp, k), dtype=object)
    for ln in range(1, k + 1):
        pc = codes.copy()
        pc[:, ln:] = rng.integers(0, 4, (n_pref, k - ln), dtype=np.uint8)  # garbage past the prefix: ignored
        pp = S.pack_codes(pc)
        ok, rules = _ranges(hostlib, pp, np.full(n_pref, ln), k)
        assert ok == n_pref
        for i in range(n_pref):
            want = (kc[:, :ln] == codes[i, :ln]).all(axis=1)
            got = _matches(rules[i], tf)
            assert (got == want).all(), (k, ln, i, np.nonzero(got != want)[0][:5])
            assert want.any()


@pytest.mark.parametrize("k", (9, 31, 126))
def test_range_rule_shapes(hostlib, k):
    """The three cases of the rule: m = 0 is one interval over the top 18 f bits, 0 < m with f < L filters block f's low 2 bits,
    and lengths that reach into the k % 9 remaining nucleotides are one interval again; lengths outside [1, k] match nothing."""
    L, R = k // 9, k % 9
    p = S.pack_codes(np.random.default_rng(1).integers(0, 4, (1, k), dtype=np.uint8))
    for ln in range(1, k + 1):
        _, [(lo, hi, fsh, fval)] = _ranges(hostlib, p, [ln], k)
        f, m = divmod(ln, 9)
        fixed = 18 * f if m == 0 else (18 * f + 2 * (m - 1) if f < L else 18 * L + 2 * m)
        assert hi - lo == (1 << (2 * k - fixed)) - 1, ln
        if m and f < L:
            assert fsh == 2 * R + 18 * (L - 1 - f) and 0 <= fval < 4
        else:
            assert fsh == -1
    for bad in (0, k + 1, 255):
        ok, _ = _ranges(hostlib, p, [bad], k)
        assert ok == 0


def test_prefix_symbols_are_declared_and_exported():
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    for name in ("bft_gpu_query_prefixes", "bft_gpu_query_prefixes_dev"):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert {"bft_gpu_query_prefixes", "bft_gpu_query_prefixes_dev"} <= set(re.findall(r" T (bft_gpu_[a-z_0-9]+)", out))
    compat = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bft", "bft.h")).read(), flags=re.S)
    assert re.search(r"\bbool\s+prefix_matching\s*\(\s*BFT\s*\*\s*bft\s*,\s*char\s*\*\s*prefix\s*,\s*BFT_func_ptr\s+f\s*,\s*\.\.\.\s*\)\s*;", compat)
    libbft = os.path.join(_lib.CSRC, "libbft.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", libbft]).decode()
    assert re.search(r" T prefix_matching$", out, flags=re.M)
    hdr_text = open(os.path.join(ROOT, "include", "bft", "bft.h")).read()
    not_provided = hdr_text[hdr_text.index("Not provided"):hdr_text.index("*/", hdr_text.index("Not provided"))]
    assert not re.search(r"\bprefix_matching\b", not_provided)  # (prefix_matching_custom stays out)


def test_prefix_kernels_use_no_scratch():
    """The k_pm_* kernels (every key width) keep to registers: no scratch memory, no vector register spilled to it."""
    subprocess.check_call(["make", "-C", _lib.CSRC, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_pm_"], capture_output=True, text=True).stdout
    seen = set()
    for line in out.splitlines()[1:]:
        if not line.strip():
            continue
        vgpr, sgpr, vspill, sspill, scratch, lds, maxwg, name = line.split(None, 7)
        m = re.search(r"(k_pm_[a-z]+)<(\d)", name)
        if not m:
            continue
        seen.add((m.group(1), int(m.group(2))))
        assert int(vspill) == 0 and int(scratch) == 0, line
    assert seen == {(kern, w) for kern in ("k_pm_bounds", "k_pm_count", "k_pm_emit") for w in (1, 2, 3, 4)}, seen
