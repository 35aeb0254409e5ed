"""ctypes binding of the C-ABI in include/bft_gpu.h (csrc/libbft_gpu.so).

There is no fallback: if the HIP library is missing or fails to load, importing the product API raises.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(CSRC, "libbft_gpu.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "bft_gpu.h")

_lib = None

# name -> (restype, argtypes); one entry per declaration in include/bft_gpu.h
_P = C.c_void_p
SIGNATURES = {
    "bft_gpu_last_error": (C.c_char_p, []),
    "bft_gpu_device_count": (C.c_int, []),
    "bft_gpu_version": (C.c_char_p, []),
    "bft_gpu_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_P)]),
    "bft_gpu_create_seeded": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "bft_gpu_free": (None, [_P]),
    "bft_gpu_cache_release": (C.c_uint64, []),
    "bft_gpu_add_genome": (C.c_int, [_P, C.c_char_p, C.POINTER(C.c_uint32)]),
    "bft_gpu_genome_name": (C.c_int, [_P, C.c_uint32, C.c_char_p, C.c_uint32]),
    "bft_gpu_insert_kmers": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32]),
    "bft_gpu_insert_kmers_dev": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32]),
    "bft_gpu_insert_kmers_dev_async": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, _P]),
    "bft_gpu_build": (C.c_int, [_P]),
    "bft_gpu_query_presence": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "bft_gpu_query_presence_dev": (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    "bft_gpu_query_colors": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "bft_gpu_query_colors_dev": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, C.c_uint64, _P, _P]),
    "bft_gpu_query_color_rows": (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    "bft_gpu_query_branching": (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    "bft_gpu_query_branching_dev": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P]),
    "bft_gpu_query_sequences": (C.c_int, [_P, C.c_char_p, _P, C.c_uint64, C.c_double, C.c_int, _P]),
    "bft_gpu_query_sequences_dev": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, C.c_double, C.c_int, _P, _P]),
    "bft_gpu_insert_sequences": (C.c_int, [_P, C.c_char_p, _P, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "bft_gpu_insert_sequences_dev": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), _P]),
    "bft_gpu_insert_sequence_file": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "bft_gpu_debug_ingest_plan": (C.c_int, [C.POINTER(C.c_uint64)]),
    "bft_gpu_debug_ingest_chunks": (C.c_int, [_P, C.c_uint64, C.c_int, C.c_uint64, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "bft_gpu_load_bft": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_P)]),
    "bft_gpu_write_bft": (C.c_int, [_P, C.c_char_p]),
    "bft_gpu_set_option": (C.c_int, [_P, C.c_char_p, C.c_int64]),
    "bft_gpu_debug_get_array": (C.c_int, [_P, C.c_char_p, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "bft_gpu_debug_color_rows_plan": (C.c_int, [C.c_uint32, C.c_int, C.POINTER(C.c_uint32)]),
    "bft_gpu_debug_prefix_plan": (C.c_int, [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]),
    "bft_gpu_debug_front_last": (C.c_int, [C.POINTER(C.c_uint32)]),
    "bft_gpu_debug_run_road": (C.c_int, [_P, C.POINTER(C.c_uint32)]),
    "bft_gpu_debug_run_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint32)]),
    "bft_gpu_debug_front_plan": (C.c_int, [C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]),
    "bft_gpu_query_color_rows_dev": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, _P]),
    "bft_gpu_info": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]),
    "bft_gpu_footprint": (C.c_int, [_P, C.POINTER(C.c_uint64), C.c_int]),
    "bft_gpu_kernel_time": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_int]),
    "bft_gpu_build_time": (C.c_int, [_P, C.POINTER(C.c_double), C.c_int]),
    "bft_gpu_build_stages": (C.c_int, [_P, C.c_char_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]),
    "bft_gpu_extract": (C.c_int, [_P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "bft_gpu_colorset": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "bft_gpu_query_rows": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P]),
    "bft_gpu_colorset_annot": (C.c_int, [_P, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "bft_gpu_query_prefixes": (C.c_int, [_P, _P, _P, C.c_uint64, _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "bft_gpu_query_prefixes_dev": (C.c_int, [_P, _P, _P, C.c_uint64, _P, _P, _P, _P, C.c_uint64, _P, _P]),
    "bft_gpu_subgraph": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(_P)]),
    "bft_gpu_subgraph_dev": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(_P), _P]),
    "bft_gpu_merge": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(_P)]),
    "bft_gpu_simple_paths": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "bft_gpu_simple_paths_dev": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint64, C.c_uint64, _P, _P]),
    "bft_gpu_unitigs": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "bft_gpu_unitigs_dev": (C.c_int, [_P, C.c_uint32, _P, _P, C.c_uint64, C.c_uint64, _P, _P]),
    "bft_gpu_bidirected_degrees": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "bft_gpu_bidirected_degrees_dev": (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    "bft_gpu_unitig_graph": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "bft_gpu_unitig_graph_dev": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _P, _P]),
    "bft_gpu_unitig_colors": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_int, _P, _P]),
    "bft_gpu_unitig_colors_dev": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_int, _P, _P, _P]),
    "bft_gpu_unitig_bubbles": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_uint64, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "bft_gpu_unitig_bubbles_dev": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_uint64, _P, C.c_uint64, _P, _P]),
    "bft_gpu_unitig_segment_of": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, _P, _P, C.c_uint64]),
    "bft_gpu_unitig_segment_of_dev": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, _P, _P, C.c_uint64, _P]),
    "bft_gpu_thread_sequences": (C.c_int, [_P, C.c_char_p, _P, C.c_uint64, _P, _P, C.c_uint64, _P, C.c_uint64, _P, _P, C.c_uint64, _P, _P, C.c_uint64, _P, C.c_uint64,
                                           C.POINTER(C.c_uint64)]),
    "bft_gpu_thread_sequences_dev": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, _P, _P, C.c_uint64, _P, C.c_uint64, _P, _P, C.c_uint64, _P, _P, C.c_uint64, _P,
                                               C.c_uint64, _P, _P]),
    "bft_gpu_components": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint64, _P, C.c_uint64, _P]),
    "bft_gpu_components_dev": (C.c_int, [_P, _P, C.c_uint32, _P, _P, C.c_uint64, _P, _P]),
    "bft_gpu_kmers_by_count": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "bft_gpu_kmers_by_count_dev": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_uint64, _P, _P]),
    "bft_gpu_pangenome_stats": (C.c_int, [_P, _P, _P, _P, C.c_uint32]),
    "bft_gpu_pangenome_stats_dev": (C.c_int, [_P, _P, _P, _P, C.c_uint32, _P]),
    "bft_gpu_genome_matrix": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint32)]),
    "bft_gpu_genome_matrix_dev": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.c_uint64, _P]),
    "bft_gpu_genome_matrix_colorsets": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.POINTER(C.c_uint32)]),
    "bft_gpu_genome_matrix_colorsets_dev": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, _P]),
    "bft_gpu_combine_colors": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_int, C.c_int, _P, _P, _P]),
    "bft_gpu_combine_colors_dev": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_int, C.c_int, _P, _P, _P, _P]),
    "bft_gpu_combine_colorsets": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_int, _P, _P]),
    "bft_gpu_combine_colorsets_dev": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, C.c_int, _P, _P, _P]),
    "bft_gpu_debug_setops_plan": (C.c_int, [C.POINTER(C.c_uint64)]),
    "bft_gpu_marks_begin": (C.c_int, [_P]),
    "bft_gpu_marks_end": (C.c_int, [_P]),
    "bft_gpu_marks_set": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint8, C.POINTER(C.c_uint64)]),
    "bft_gpu_marks_set_dev": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint8, _P, _P]),
    "bft_gpu_marks_get": (C.c_int, [_P, _P, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "bft_gpu_marks_get_dev": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P]),
    "bft_gpu_marks_test_and_set": (C.c_int, [_P, _P, C.c_uint64, C.c_uint8, C.c_uint8, _P, C.POINTER(C.c_uint64)]),
    "bft_gpu_marks_test_and_set_dev": (C.c_int, [_P, _P, C.c_uint64, C.c_uint8, C.c_uint8, _P, _P, _P]),
    "bft_gpu_marks_fill": (C.c_int, [_P, C.c_uint8]),
    "bft_gpu_marks_fill_dev": (C.c_int, [_P, C.c_uint8, _P]),
    "bft_gpu_marks_counts": (C.c_int, [_P, _P]),
    "bft_gpu_marks_counts_dev": (C.c_int, [_P, _P, _P]),
    "bft_gpu_marks_select": (C.c_int, [_P, C.c_uint32, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "bft_gpu_marks_select_dev": (C.c_int, [_P, C.c_uint32, _P, _P, _P, C.c_uint64, _P, _P]),
    "bft_gpu_marks_reach": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, C.c_uint8, C.c_uint8, C.c_int, _P, _P]),
    "bft_gpu_marks_reach_dev": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, C.c_uint8, C.c_uint8, C.c_int, _P, _P, _P]),
    "bft_gpu_marks_read": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "bft_gpu_marks_write": (C.c_int, [_P, _P, C.c_uint64]),
    "bft_gpu_image_size": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "bft_gpu_image_pack": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "bft_gpu_image_unpack": (C.c_int, [_P, C.c_uint64, C.c_int, C.POINTER(_P)]),
    "bft_gpu_group_shard": (C.c_int, [C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "bft_gpu_group_create": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(_P)]),
    "bft_gpu_group_free": (None, [_P]),
    "bft_gpu_group_size": (C.c_int, [_P]),
    "bft_gpu_group_query_presence": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "bft_gpu_group_query_color_rows": (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    "bft_gpu_group_query_branching": (C.c_int, [_P, _P, C.c_uint64, _P, _P]),
    "bft_gpu_group_member_device": (C.c_int, [_P, C.c_int]),
    "bft_gpu_group_member_footprint": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64), C.c_int]),
    "bft_gpu_group_member_info": (C.c_int, [_P, C.c_int, C.POINTER(C.c_uint64), C.c_int]),
    "bft_gpu_group_query_presence_dev": (C.c_int, [_P, _P, _P, _P, _P]),
    "bft_gpu_group_query_color_rows_dev": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "bft_gpu_group_query_branching_dev": (C.c_int, [_P, _P, _P, _P, _P, _P]),
}

# test hooks: exported by the library, not part of include/bft_gpu.h (csrc/bft_intern.hip; tests/test_gpu_intern_edges.py)
TEST_HOOKS = {
    # (d_seg_off, d_ids, nk, np, mode, narrow_w, distinct_hint, d_tcol, d_cs_off, cs_off_cap, d_cs_ids, cs_ids_cap, d_narrow, counts[5], hip_stream)
    "bft_gpu_test_intern": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.c_uint64, _P, _P, C.c_uint64, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P]),
    # csrc/bft_genome_matrix.hip; tests/test_gpu_genome_matrix.py: (h, d_weights, road, flush_sets, d_shared, cap, hip_stream) and (h, canary, out[2])
    "bft_gpu_test_genome_matrix": (C.c_int, [_P, _P, C.c_int, C.c_uint32, _P, C.c_uint64, _P]),
    "bft_gpu_test_genome_matrix_state": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint32)]),
}


def build_library(force=False):
    """hipcc --offload-arch=gfx950 build of csrc/ (cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC, "all"]
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(args, stdout=subprocess.DEVNULL)


def load():
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own HIP runtime; it must be the one this process initialises, otherwise torch later
    # reports "No HIP GPUs are available" next to an already-initialised system runtime.  torch is plumbing
    # (device memory, streams, torch.distributed), so load it first when it is installed.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = os.environ.get("BFT_GPU_LIB") or LIB_PATH  # tuning experiments only: another build of the same sources
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `make -C {CSRC}` (hipcc, gfx950). "
            "bloomfiltertrie_amd has no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in list(SIGNATURES.items()) + list(TEST_HOOKS.items()):
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


MERGE_APPEND = 0xFFFFFFFF  # BFT_GPU_MERGE_APPEND (include/bft_gpu.h; tests/test_union_cases_host.py holds the two together)


class BFTError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        msg = load().bft_gpu_last_error()
        raise BFTError(f"bft_gpu error {rc}: {msg.decode() if msg else ''}")
