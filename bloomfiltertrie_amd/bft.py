"""Host-side mirror of the reference interface for the batched path (include/bft.h, include/insertNode.h,
include/presenceNode.h of GuillaumeHolley/BloomFilterTrie), over the C-ABI of include/bft_gpu.h.

Names follow the reference: create_cdbg / insert_kmers_new_genome / insertKmers / is present / get_annotation +
get_list_id_genomes.  Batches are numpy uint8 arrays [n, CEIL(2k/8)] in the reference's packed layout
(bloomfiltertrie_amd.synth / src/fasta.c:3-53).
"""
import atexit
import ctypes as C
import os
import weakref

import numpy as np

from . import _lib
from .synth import ascii_to_packed, kmer_bytes

_LIVE = weakref.WeakSet()


@atexit.register
def _close_all():
    """Free every live handle before the interpreter (and the HIP runtime under it) is torn down."""
    for t in list(_LIVE):
        try:
            t.close()
        except Exception:
            pass


INGEST_STATS = ("positions", "skipped", "distinct", "appended")  # stats[4] of bft_gpu_insert_sequences
INFO_FIELDS = ["k", "kmers", "nodes", "ccs", "uc_rows", "child_nodes", "prefixes", "ccs_s4", "max_ccs_per_node",
               "pairs", "colorsets", "genomes", "image_bytes", "root_ccs", "root_uc_rows", "pending_pairs"]


class BFT:
    """One Bloom Filter Trie resident in the HBM of one MI355X (replaces BFT_Root, include/Node.h:96-122)."""

    def __init__(self, k, device=0, r1=0, r2=0, _handle=None):
        self._lib = _lib.load()
        h = C.c_void_p()
        if _handle is not None:
            h = _handle
        else:
            _lib.check(self._lib.bft_gpu_create_seeded(k, device, r1, r2, C.byref(h)))  # create_cdbg, include/bft.h:62
        self._h = h
        self.k = k
        self.nb = kmer_bytes(k)
        self.device = device
        self._named = 0  # genomes named through add_genome (the image's count covers those of a loaded or unpacked handle)
        _LIVE.add(self)

    @classmethod
    def load_bft(cls, path, device=0):
        """load_BFT (include/bft.h:176)."""
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.bft_gpu_load_bft(path.encode(), device, C.byref(h)))
        out = (C.c_uint64 * 16)()
        _lib.check(lib.bft_gpu_info(h, out, 16))
        return cls(int(out[0]), device=device, _handle=h)

    @classmethod
    def from_image(cls, d_blob_ptr, nbytes, device=0):
        """New index on `device` from an image blob resident in that GPU's memory (see image_pack)."""
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.bft_gpu_image_unpack(d_blob_ptr, nbytes, device, C.byref(h)))
        out = (C.c_uint64 * 16)()
        _lib.check(lib.bft_gpu_info(h, out, 16))
        return cls(int(out[0]), device=device, _handle=h)

    def image_size(self):
        """Bytes of the device blob that image_pack writes."""
        n = C.c_uint64()
        _lib.check(self._lib.bft_gpu_image_size(self._h, C.byref(n)))
        return int(n.value)

    def image_pack(self, d_blob_ptr, cap, stream=None):
        """Copy the built index (containers, k-mer table, colour sets, genome names) into one
        contiguous device buffer -- the payload of the broadcast that replicates the trie on the other GPUs."""
        _lib.check(self._lib.bft_gpu_image_pack(self._h, d_blob_ptr, cap, stream))

    def write_bft(self, path):
        """write_BFT (include/bft.h:175)."""
        _lib.check(self._lib.bft_gpu_write_bft(self._h, path.encode()))

    # -- lifecycle ----------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.bft_gpu_free(self._h)  # free_cdbg, include/bft.h:63
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, kmers):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint8)
        if kmers.ndim != 2 or kmers.shape[1] != self.nb:
            raise ValueError(f"expected packed k-mers of shape [n, {self.nb}], got {kmers.shape}")
        return kmers

    # -- insertion ----------------------------------------------------------------------------------------------
    def add_genome(self, name):
        """add_genomes_BFT_Root (include/CC.h:307-338)."""
        gid = C.c_uint32()
        _lib.check(self._lib.bft_gpu_add_genome(self._h, name.encode(), C.byref(gid)))
        self._named = max(self._named, gid.value + 1)
        return gid.value

    def insert_kmers(self, kmers, id_genome):
        """insertKmers(root, array_kmers, nb_kmers, id_genome, size_id_genome) (include/insertNode.h:26)."""
        kmers = self._chk(kmers)
        _lib.check(self._lib.bft_gpu_insert_kmers(self._h, kmers.ctypes.data, len(kmers), id_genome))

    def insert_kmers_dev(self, d_ptr, n, id_genome):
        _lib.check(self._lib.bft_gpu_insert_kmers_dev(self._h, d_ptr, n, id_genome))

    def insert_kmers_dev_async(self, d_ptr, n, id_genome, stream):
        """insert_kmers_dev, stream-ordered on the caller's HIP stream (raw handle; None / 0 = the null stream): returns at once."""
        _lib.check(self._lib.bft_gpu_insert_kmers_dev_async(self._h, d_ptr, n, id_genome, stream))

    def insert_kmers_new_genome(self, kmers_ascii, genome_name):
        """insert_kmers_new_genome(nb_kmers, kmers, genome_name, bft) (include/bft.h:72)."""
        gid = self.add_genome(genome_name)
        packed, valid = ascii_to_packed(kmers_ascii, self.k)
        if not valid.all():
            raise ValueError("k-mer with a character outside ACGTU (reference get_kmer/insert path exits, src/bft.c:239)")
        self.insert_kmers(packed, gid)
        return gid

    def insert_sequences(self, sequences, id_genome, canonical=False, min_abundance=0):
        """Every k-mer of a list of ASCII sequences into genome id_genome (bft_gpu_insert_sequences): windows with a character outside ACGTU are
        skipped, canonical=True inserts what query_sequences(canonical=True) looks up, min_abundance >= 1 keeps the k-mers seen at least that
        often in this call.  Returns the stats: positions, skipped, distinct (0 without counting), appended."""
        enc = [x.encode() if isinstance(x, str) else bytes(x) for x in sequences]
        off = np.zeros(len(enc) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(e) for e in enc])
        blob = b"".join(enc) + b"\0"
        st = (C.c_uint64 * 4)()
        _lib.check(self._lib.bft_gpu_insert_sequences(self._h, blob, off.ctypes.data, len(enc), int(canonical), int(min_abundance), id_genome, st))
        return dict(zip(INGEST_STATS, (int(x) for x in st)))

    def insert_sequences_dev(self, d_seqs_ptr, d_seq_off_ptr, n_seqs, total_chars, id_genome, canonical=False, min_abundance=0, stream=None):
        """Device-resident variant of insert_sequences (raw pointers; any alignment of the blob): runs on `stream` and synchronises it."""
        st = (C.c_uint64 * 4)()
        _lib.check(self._lib.bft_gpu_insert_sequences_dev(self._h, C.c_void_p(d_seqs_ptr or 0), C.c_void_p(d_seq_off_ptr or 0), n_seqs, total_chars, int(canonical),
                                                          int(min_abundance), id_genome, st, C.c_void_p(stream or 0)))
        return dict(zip(INGEST_STATS, (int(x) for x in st)))

    def insert_sequence_file(self, path, id_genome, canonical=False, min_abundance=0):
        """A plain-text FASTA or four-line FASTQ file into genome id_genome (bft_gpu_insert_sequence_file)."""
        st = (C.c_uint64 * 4)()
        _lib.check(self._lib.bft_gpu_insert_sequence_file(self._h, os.fsencode(path), int(canonical), int(min_abundance), id_genome, st))
        return dict(zip(INGEST_STATS, (int(x) for x in st)))

    def build(self):
        _lib.check(self._lib.bft_gpu_build(self._h))

    # -- queries ------------------------------------------------------------------------------------------------
    def query_presence(self, kmers):
        """Loop of src/file_io.c:726-768 over isKmerPresent: presence bitmap (bit i%8 of byte i//8)."""
        kmers = self._chk(kmers)
        bits = np.zeros((len(kmers) + 7) // 8, dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_query_presence(self._h, kmers.ctypes.data, len(kmers), bits.ctypes.data))
        return bits

    def query_presence_dev(self, d_kmers_ptr, n, d_bits_ptr, stream=None):
        """Device-resident variant: pointers into HBM (e.g. torch tensor .data_ptr()); asynchronous on `stream`."""
        _lib.check(self._lib.bft_gpu_query_presence_dev(self._h, d_kmers_ptr, n, d_bits_ptr, stream))

    def query_colors(self, kmers):
        """get_annotation + get_list_id_genomes per k-mer: (bits, offsets[n+1], ids)."""
        kmers = self._chk(kmers)
        n = len(kmers)
        bits = np.zeros((n + 7) // 8, dtype=np.uint8)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        cap = max(1024, 4 * n)
        while True:
            ids = np.zeros(cap, dtype=np.uint32)
            need = C.c_uint64()
            rc = self._lib.bft_gpu_query_colors(self._h, kmers.ctypes.data, n, bits.ctypes.data, offsets.ctypes.data,
                                                ids.ctypes.data, cap, C.byref(need))
            if rc == -6:  # BFT_GPU_E_NOSPACE
                cap = int(need.value)
                continue
            _lib.check(rc)
            return bits, offsets, ids[:int(need.value)]

    def query_rows(self, kmers):
        """What resultPresence holds for each k-mer (include/Node.h:60-92) as indexes: (bits, row in the stored k-mer
        table, colour-set id); 0xFFFFFFFF where absent."""
        kmers = self._chk(kmers)
        n = len(kmers)
        bits = np.zeros((n + 7) // 8, dtype=np.uint8)
        rows = np.zeros(n, dtype=np.uint32)
        sets = np.zeros(n, dtype=np.uint32)
        _lib.check(self._lib.bft_gpu_query_rows(self._h, kmers.ctypes.data, n, bits.ctypes.data, rows.ctypes.data, sets.ctypes.data))
        return bits, rows, sets

    def query_color_rows(self, kmers):
        """Fixed-width colour rows (the CSV row of src/file_io.c:744-765 before formatting)."""
        kmers = self._chk(kmers)
        n = len(kmers)
        self.build()  # the genome count is known once the image exists
        g = self.info()["genomes"]
        bits = np.zeros((n + 7) // 8, dtype=np.uint8)
        rows = np.zeros((n, (g + 7) // 8), dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_query_color_rows(self._h, kmers.ctypes.data, n, bits.ctypes.data, rows.ctypes.data))
        return bits, rows

    def query_colors_dev(self, d_kmers_ptr, n, d_bits_ptr, d_offsets_ptr, d_ids_ptr, ids_cap, d_needed_ptr=0, stream=None):
        """Device-resident id lists (bft_gpu_query_colors_dev): offsets (n + 1 uint64) and ids (uint32) in HBM, no synchronisation; when the
        ids number more than ids_cap only the first ids_cap of them are written (*d_needed_ptr says how many there are)."""
        _lib.check(self._lib.bft_gpu_query_colors_dev(self._h, C.c_void_p(d_kmers_ptr), n, C.c_void_p(d_bits_ptr), C.c_void_p(d_offsets_ptr),
                                                      C.c_void_p(d_ids_ptr or 0), ids_cap, C.c_void_p(d_needed_ptr or 0), C.c_void_p(stream or 0)))

    def query_color_rows_dev(self, d_kmers_ptr, n, d_bits_ptr, d_rows_ptr, d_scratch_u32_ptr, stream=None):
        """Device-resident colour rows (bft_gpu_query_color_rows_dev): n x CEIL(nb_genomes/8) bytes at d_rows_ptr, no synchronisation."""
        _lib.check(self._lib.bft_gpu_query_color_rows_dev(self._h, C.c_void_p(d_kmers_ptr), n, C.c_void_p(d_bits_ptr), C.c_void_p(d_rows_ptr),
                                                          C.c_void_p(d_scratch_u32_ptr), C.c_void_p(stream or 0)))

    def query_branching(self, kmers, with_counts=False):
        """-query_branching (src/file_io.c:897-1020): bit per k-mer, optionally (successors << 4) | predecessors."""
        kmers = self._chk(kmers)
        n = len(kmers)
        bits = np.zeros((n + 7) // 8, dtype=np.uint8)
        counts = np.zeros(n, dtype=np.uint8) if with_counts else None
        _lib.check(self._lib.bft_gpu_query_branching(self._h, kmers.ctypes.data, n, bits.ctypes.data,
                                                     counts.ctypes.data if with_counts else None))
        return (bits, counts) if with_counts else bits

    def query_branching_dev(self, d_kmers_ptr, n, d_bits_ptr, d_counts_ptr=None, stream=None):
        """Device-resident variant of query_branching: asynchronous on `stream`."""
        _lib.check(self._lib.bft_gpu_query_branching_dev(self._h, d_kmers_ptr, n, d_bits_ptr, d_counts_ptr, stream))

    def query_sequences(self, sequences, threshold, canonical=False):
        """query_sequence (include/bft.h:127) for a list of ASCII sequences: list of sorted genome-id lists."""
        enc = [x.encode() if isinstance(x, str) else bytes(x) for x in sequences]
        off = np.zeros(len(enc) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(e) for e in enc])
        blob = b"".join(enc) + b"\0"
        self.build()
        g = self.info()["genomes"]
        rows = np.zeros((len(enc), (g + 7) // 8), dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_query_sequences(self._h, blob, off.ctypes.data, len(enc), float(threshold), int(canonical),
                                                     rows.ctypes.data))
        unp = np.unpackbits(rows, axis=1, bitorder="little")[:, :g] if g else np.zeros((len(enc), 0), np.uint8)
        return [np.flatnonzero(r).tolist() for r in unp]

    def query_sequences_dev(self, d_seqs_ptr, d_seq_off_ptr, n_seqs, total_chars, threshold, d_rows_ptr, canonical=False, stream=None):
        """Device-resident variant of query_sequences (raw pointers; rows of CEIL(genomes/8) bytes): asynchronous on `stream`."""
        _lib.check(self._lib.bft_gpu_query_sequences_dev(self._h, d_seqs_ptr, d_seq_off_ptr, n_seqs, total_chars, float(threshold), int(canonical),
                                                         d_rows_ptr, stream))

    def set_option(self, name, value):
        _lib.check(self._lib.bft_gpu_set_option(self._h, name.encode(), int(value)))

    # -- introspection ------------------------------------------------------------------------------------------
    def info(self):
        out = (C.c_uint64 * 16)()
        _lib.check(self._lib.bft_gpu_info(self._h, out, 16))
        return dict(zip(INFO_FIELDS, [int(x) for x in out]))

    def kernel_time(self, reset=True):
        ms, n = C.c_double(), C.c_uint64()
        _lib.check(self._lib.bft_gpu_kernel_time(self._h, C.byref(ms), C.byref(n), 1 if reset else 0))
        return ms.value, n.value

    def build_time(self):
        out = (C.c_double * 25)()
        _lib.check(self._lib.bft_gpu_build_time(self._h, out, 25))
        return dict(zip(["gpu_sort_dedupe_ms", "color_intern_ms", "assemble_ms", "sort_redone_buckets", "derive_ms",
                         "query_wgs_per_cu", "tune_1wg_ms", "tune_2wg_ms", "query_probe_rows", "kmer_hash_lines", "kmer_hash_fill_ms",
                         "sort_max_bucket", "intern_exact_passes", "process_hipmalloc_ms", "root_tables", "tune_root_direct_ms", "tune_root_range_ms", "node_hash_keys", "node_hash_dropped", "tune_2wg768_ms",
                         "claims_static_launches", "kmer_hash_slots", "kmer_hash_dbits", "kmer_hash_maxd", "kmer_hash_overflow"], list(out)))

    def build_stages(self):
        """[(stage name, GPU ms, algorithmic bytes)] of the last build (set_option("build_stages", 1) before it)."""
        n = C.c_int()
        _lib.check(self._lib.bft_gpu_build_stages(self._h, None, 0, None, None, 0, C.byref(n)))
        if n.value == 0:
            return []
        names = C.create_string_buffer(256 * n.value)
        ms, by = (C.c_double * n.value)(), (C.c_double * n.value)()
        _lib.check(self._lib.bft_gpu_build_stages(self._h, names, len(names), ms, by, n.value, C.byref(n)))
        return list(zip(names.value.decode().split("\n")[:n.value], list(ms), list(by)))

    FOOTPRINT_FIELDS = ["kmer_table", "colorset_per_kmer", "colorset_dictionary", "containers", "flat_ccs", "root_tables", "node_prefix_hash", "kmer_hash",
                        "dictionary_bitmaps", "hash_table", "pair_store", "insertion_log"]

    def footprint(self):
        """Bytes in HBM per part of the handle (bft_gpu_footprint; src/printMemory.c:255 reports the reference's by container kind)."""
        out = (C.c_uint64 * 12)()
        _lib.check(self._lib.bft_gpu_footprint(self._h, out, 12))
        return dict(zip(self.FOOTPRINT_FIELDS, [int(x) for x in out]))

    def debug_array(self, name, dtype=np.uint8):
        n = C.c_uint64()
        _lib.check(self._lib.bft_gpu_debug_get_array(self._h, name.encode(), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_debug_get_array(self._h, name.encode(), out.ctypes.data, n.value, C.byref(n)))
        return out.view(dtype)

    def extract(self):
        n = C.c_uint64()
        _lib.check(self._lib.bft_gpu_extract(self._h, None, None, 0, C.byref(n)))
        kmers = np.zeros((n.value, self.nb), dtype=np.uint8)
        cs = np.zeros(n.value, dtype=np.uint32)
        _lib.check(self._lib.bft_gpu_extract(self._h, kmers.ctypes.data, cs.ctypes.data, n.value, C.byref(n)))
        return kmers, cs

    def colorset(self, cs):
        n = C.c_uint32()
        _lib.check(self._lib.bft_gpu_colorset(self._h, int(cs), None, 0, C.byref(n)))
        ids = np.zeros(n.value, dtype=np.uint32)
        _lib.check(self._lib.bft_gpu_colorset(self._h, int(cs), ids.ctypes.data, n.value, C.byref(n)))
        return ids.tolist()

    def colorset_annot(self, cs):
        """The colour set as the reference's annotation bytes (BFT_annotation::annot, src/bft.c:363-387)."""
        n = C.c_uint32()
        _lib.check(self._lib.bft_gpu_colorset_annot(self._h, int(cs), None, 0, C.byref(n)))
        out = np.zeros(max(1, n.value), dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_colorset_annot(self._h, int(cs), out.ctypes.data, n.value, C.byref(n)))
        return out[:n.value].tobytes()


    def _prefix_batch(self, prefixes, lengths):
        """ASCII prefixes (lengths = their lengths) or packed rows [n, nb] with lengths (one per row, or one for all) -> (packed, lengths)."""
        if lengths is None:
            prefixes = list(prefixes)
            lens = np.array([len(p) for p in prefixes], dtype=np.int64)
            if ((lens < 1) | (lens > self.k)).any():
                raise ValueError(f"prefix length outside [1, {self.k}] (reference prefix_matching exits, src/bft.c:1106-1107)")
            packed, valid = ascii_to_packed([(p if isinstance(p, str) else p.decode()) + "A" * (self.k - len(p)) for p in prefixes], self.k)
            if not valid.all():
                raise ValueError("prefix with a character outside ACGTU (reference prefix_matching exits, src/bft.c:1125-1126)")
            return packed, lens.astype(np.uint8)
        packed = self._chk(prefixes)
        lens = np.broadcast_to(np.asarray(lengths, dtype=np.int64), (len(packed),))
        if ((lens < 1) | (lens > self.k)).any():
            raise ValueError(f"prefix length outside [1, {self.k}]")
        return packed, np.ascontiguousarray(lens, dtype=np.uint8)

    def query_prefixes(self, prefixes, lengths=None):
        """prefix_matching (include/bft.h:135, src/bft.c:1087-1147) for a batch: the stored k-mers that start with each prefix.
        Returns (offsets [n + 1] uint64, kmers [m, nb] uint8, rows [m] uint32, colour sets [m] uint32); prefix i's matches are entries
        offsets[i]:offsets[i + 1], in ascending row order (the order of extract())."""
        packed, lens = self._prefix_batch(prefixes, lengths)
        n = len(packed)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        cap = max(1024, 4 * n)
        while True:
            kmers = np.zeros((cap, self.nb), dtype=np.uint8)
            rows = np.zeros(cap, dtype=np.uint32)
            sets = np.zeros(cap, dtype=np.uint32)
            need = C.c_uint64()
            rc = self._lib.bft_gpu_query_prefixes(self._h, packed.ctypes.data, lens.ctypes.data, n, offsets.ctypes.data, kmers.ctypes.data,
                                                  rows.ctypes.data, sets.ctypes.data, cap, C.byref(need))
            if rc == -6:  # BFT_GPU_E_NOSPACE
                cap = int(need.value)
                continue
            _lib.check(rc)
            m = int(need.value)
            return offsets, kmers[:m], rows[:m], sets[:m]

    def query_prefixes_dev(self, d_prefixes_ptr, d_lengths_ptr, n, d_offsets_ptr, d_kmers_ptr, d_rows_ptr, d_colorsets_ptr, cap, d_needed_ptr=0,
                           stream=None):
        """Device-resident prefix matching (bft_gpu_query_prefixes_dev): offsets (n + 1 uint64) always, the first `cap` matches into the
        outputs that are not 0, the number of matches at d_needed_ptr; no synchronisation.  A length outside [1, k] matches nothing."""
        _lib.check(self._lib.bft_gpu_query_prefixes_dev(self._h, C.c_void_p(d_prefixes_ptr), C.c_void_p(d_lengths_ptr), n, C.c_void_p(d_offsets_ptr),
                                                        C.c_void_p(d_kmers_ptr or 0), C.c_void_p(d_rows_ptr or 0), C.c_void_p(d_colorsets_ptr or 0),
                                                        cap, C.c_void_p(d_needed_ptr or 0), C.c_void_p(stream or 0)))

    def subgraph(self, kmers, colors=True):
        """create_cdbg_from_bft_kmers (include/bft.h:179, src/bft.c:1353-1464) on the GPU: a new BFT holding those of the packed k-mers this index
        stores, with their colour sets (colors) or all in one genome named after genome 0.  Duplicates collapse.  Returns (BFT, n_absent)."""
        kmers = self._chk(kmers)
        h = C.c_void_p()
        absent = C.c_uint64()
        _lib.check(self._lib.bft_gpu_subgraph(self._h, kmers.ctypes.data, len(kmers), 1 if colors else 0, C.byref(absent), C.byref(h)))
        return BFT(self.k, device=self.device, _handle=h), int(absent.value)

    def subgraph_dev(self, d_kmers_ptr, n, colors=True, stream=None):
        """The same on a device-resident batch (bft_gpu_subgraph_dev): d_kmers is read in order on `stream`.  Returns (BFT, n_absent)."""
        h = C.c_void_p()
        absent = C.c_uint64()
        _lib.check(self._lib.bft_gpu_subgraph_dev(self._h, C.c_void_p(d_kmers_ptr or 0), n, 1 if colors else 0, C.byref(absent), C.byref(h),
                                                  C.c_void_p(stream or 0)))
        return BFT(self.k, device=self.device, _handle=h), int(absent.value)

    def merge(self, other, id_base=None):
        """merging_BFT (include/merge.h:14) on the GPU: a new BFT holding every k-mer of this index and of `other`; genome g of `other` becomes genome
        id_base + g, a k-mer of both has the union of its two colour sets.  id_base None appends (this index's genome count); one below that count is
        the reference's overlap of the last and the first genome; 0 means the same genomes.  Both sources stay as they are (bft_gpu_merge)."""
        if id_base is None:
            id_base = _lib.MERGE_APPEND  # the count once pending insertions are built
        h = C.c_void_p()
        _lib.check(self._lib.bft_gpu_merge(self._h, other._h, int(id_base), C.byref(h)))
        return BFT(self.k, device=self.device, _handle=h)

    def simple_paths(self, min_shared=0):
        """extract_simple_paths_to_disk / extract_simple_core_paths_to_disk (reference snippets.h, src/snippets.c:115-603) on the GPU: the simple
        (non-branching) paths of the index as ASCII strings, in ascending row of their first k-mer.  min_shared = t: only k-mers of t genomes
        or more, joined where they share t or more (0: plain simple paths; bft_gpu_simple_paths defines the paths)."""
        n_paths, n_chars = C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.bft_gpu_simple_paths(self._h, int(min_shared), None, None, 0, 0, C.byref(n_paths), C.byref(n_chars)))
        offsets = np.zeros(n_paths.value + 1, dtype=np.uint64)
        seqs = np.zeros(max(1, n_chars.value), dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_simple_paths(self._h, int(min_shared), offsets.ctypes.data, seqs.ctypes.data, n_paths.value, n_chars.value,
                                                  C.byref(n_paths), C.byref(n_chars)))
        text = seqs[:n_chars.value].tobytes().decode()
        return [text[int(offsets[i]):int(offsets[i + 1])] for i in range(n_paths.value)]

    def simple_paths_dev(self, d_offsets_ptr, d_seqs_ptr, paths_cap, chars_cap, d_counts_ptr, min_shared=0, stream=None):
        """Device-resident simple paths (bft_gpu_simple_paths_dev): {n_paths, n_chars, longest} (3 uint64) at d_counts_ptr always, the offsets
        entries j <= paths_cap and the characters below chars_cap into the buffers that are not 0; no synchronisation."""
        _lib.check(self._lib.bft_gpu_simple_paths_dev(self._h, int(min_shared), C.c_void_p(d_offsets_ptr or 0), C.c_void_p(d_seqs_ptr or 0), paths_cap,
                                                      chars_cap, C.c_void_p(d_counts_ptr), C.c_void_p(stream or 0)))

    def unitigs(self, min_shared=0):
        """The canonical (bidirected) unitigs of a canonical index -- one built with insert_sequences(..., canonical=True) -- on the GPU
        (bft_gpu_unitigs defines them): maximal non-branching paths over k-mers and their reverse complements, each reported on one strand, in
        ascending id of their first oriented vertex.  min_shared = t as in simple_paths.  Returns (offsets: uint64 [n_paths + 1], in characters;
        seqs: uint8 [n_chars], ASCII ACGT): unitig i is seqs[offsets[i]:offsets[i + 1]].  An index that is not canonical raises (BFT_GPU_E_STATE)."""
        n_paths, n_chars = C.c_uint64(), C.c_uint64()
        _lib.check(self._lib.bft_gpu_unitigs(self._h, int(min_shared), None, None, 0, 0, C.byref(n_paths), C.byref(n_chars)))
        offsets = np.zeros(n_paths.value + 1, dtype=np.uint64)
        seqs = np.zeros(max(1, n_chars.value), dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_unitigs(self._h, int(min_shared), offsets.ctypes.data, seqs.ctypes.data, n_paths.value, n_chars.value,
                                             C.byref(n_paths), C.byref(n_chars)))
        return offsets, seqs[:n_chars.value]

    def unitigs_dev(self, d_offsets_ptr, d_seqs_ptr, paths_cap, chars_cap, d_counts_ptr, min_shared=0, stream=None):
        """Device-resident unitigs (bft_gpu_unitigs_dev): {n_paths, n_chars, longest, non-canonical rows} (4 uint64) at d_counts_ptr always, the
        offsets entries j <= paths_cap and the characters below chars_cap into the buffers that are not 0; no synchronisation."""
        _lib.check(self._lib.bft_gpu_unitigs_dev(self._h, int(min_shared), C.c_void_p(d_offsets_ptr or 0), C.c_void_p(d_seqs_ptr or 0), paths_cap,
                                                 chars_cap, C.c_void_p(d_counts_ptr), C.c_void_p(stream or 0)))

    def bidirected_degrees(self):
        """Bidirected degrees of every stored k-mer (bft_gpu_bidirected_degrees), on any index: (degrees: uint8 per row in the extract order,
        out(s, 0) << 4 | out(s, 1) over k-mers and reverse complements; the number of rows that are not canonical)."""
        bad = C.c_uint64()
        _lib.check(self._lib.bft_gpu_bidirected_degrees(self._h, None, 0, C.byref(bad)))  # (pending insertions are built: the row count is final)
        deg = np.zeros(int(self.info()["kmers"]), dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_bidirected_degrees(self._h, deg.ctypes.data if len(deg) else None, len(deg), C.byref(bad)))
        return deg, int(bad.value)

    def bidirected_degrees_dev(self, d_degrees_ptr, cap, d_noncanonical_ptr, stream=None):
        """Device-resident bidirected degrees (bft_gpu_bidirected_degrees_dev): the count of non-canonical rows (1 uint64) at d_noncanonical_ptr
        always, the degree bytes of the rows below cap at d_degrees_ptr when it is not 0; no synchronisation."""
        _lib.check(self._lib.bft_gpu_bidirected_degrees_dev(self._h, C.c_void_p(d_degrees_ptr or 0), cap, C.c_void_p(d_noncanonical_ptr),
                                                            C.c_void_p(stream or 0)))

    def unitig_graph(self, min_shared=0):
        """The compacted coloured graph of a canonical index on the GPU (bft_gpu_unitig_graph defines it): the unitigs plus one single-k-mer segment
        per branching k-mer, the links between oriented segments 2 * i + o, and the vertices 2 * row + o of every segment.  Returns (seg_off: uint64
        [n_segments + 1], in characters; seqs: uint8 ASCII; link_off: uint64 [2 * n_segments + 1], by oriented segment; links: uint32 target oriented
        segments; members: uint32, segment i from seg_off[i] - i * (k - 1) on).  An index that is not canonical raises (BFT_GPU_E_STATE)."""
        cnt = (C.c_uint64 * 6)()
        _lib.check(self._lib.bft_gpu_unitig_graph(self._h, int(min_shared), None, None, None, None, None, 0, 0, 0, 0, cnt))
        ns, nc, nl = int(cnt[0]), int(cnt[1]), int(cnt[4])
        nm = nc - ns * (self.k - 1)
        seg_off = np.zeros(ns + 1, dtype=np.uint64)
        link_off = np.zeros(2 * ns + 1, dtype=np.uint64)
        seqs = np.zeros(max(1, nc), dtype=np.uint8)
        links = np.zeros(max(1, nl), dtype=np.uint32)
        members = np.zeros(max(1, nm), dtype=np.uint32)
        _lib.check(self._lib.bft_gpu_unitig_graph(self._h, int(min_shared), seg_off.ctypes.data, seqs.ctypes.data, link_off.ctypes.data, links.ctypes.data,
                                                  members.ctypes.data, ns, nc, nl, nm, cnt))
        return seg_off, seqs[:nc], link_off, links[:nl], members[:nm]

    def unitig_graph_dev(self, d_seg_off_ptr, d_seqs_ptr, d_link_off_ptr, d_links_ptr, d_members_ptr, seg_cap, chars_cap, links_cap, members_cap,
                         d_counts_ptr, min_shared=0, stream=None):
        """Device-resident compacted graph (bft_gpu_unitig_graph_dev): {n_segments, n_chars, longest, non-canonical rows, n_links, singles} (6 uint64)
        at d_counts_ptr always, every output that is not 0 below its cap; no synchronisation."""
        _lib.check(self._lib.bft_gpu_unitig_graph_dev(self._h, int(min_shared), C.c_void_p(d_seg_off_ptr or 0), C.c_void_p(d_seqs_ptr or 0),
                                                      C.c_void_p(d_link_off_ptr or 0), C.c_void_p(d_links_ptr or 0), C.c_void_p(d_members_ptr or 0), seg_cap,
                                                      chars_cap, links_cap, members_cap, C.c_void_p(d_counts_ptr), C.c_void_p(stream or 0)))

    def unitig_colors(self, members, seg_off, op):
        """One colour row per segment of unitig_graph (bft_gpu_unitig_colors): op ("and" / "or" / "symdiff", as combine_colorsets) over the colour sets
        of the segment's members.  Returns (rows: uint8 [n_segments, ceil(genomes / 8)], bit g of a row = genome g; counts: uint32 genomes per row)."""
        code = self._setop(op)
        members = np.ascontiguousarray(members, dtype=np.uint32)
        seg_off = np.ascontiguousarray(seg_off, dtype=np.uint64)
        ns = max(0, len(seg_off) - 1)
        self.build()  # (pending genomes count in the row width)
        rb = (int(self.info()["genomes"]) + 7) // 8
        rows = np.zeros((ns, rb), dtype=np.uint8)
        counts = np.zeros(ns, dtype=np.uint32)
        _lib.check(self._lib.bft_gpu_unitig_colors(self._h, members.ctypes.data if len(members) else None, len(members), seg_off.ctypes.data if len(seg_off) else None,
                                                   ns, code, rows.ctypes.data if rows.size else None, counts.ctypes.data if ns else None))
        return rows, counts

    def unitig_colors_dev(self, d_members_ptr, n_members, d_seg_off_ptr, n_segments, op, d_rows_ptr, d_counts_ptr, stream=None):
        """Device-resident segment colours (bft_gpu_unitig_colors_dev): rows and / or counts into the buffers that are not 0; no synchronisation."""
        _lib.check(self._lib.bft_gpu_unitig_colors_dev(self._h, C.c_void_p(d_members_ptr or 0), n_members, C.c_void_p(d_seg_off_ptr or 0), n_segments, self._setop(op),
                                                       C.c_void_p(d_rows_ptr or 0), C.c_void_p(d_counts_ptr or 0), C.c_void_p(stream or 0)))

    def unitig_bubbles(self, graph, max_branch_chars=0):
        """Simple bubbles (variants) of a compacted graph on the GPU (bft_gpu_unitig_bubbles defines them): graph is the tuple unitig_graph returned.
        Returns (bubbles: uint32 [n, 6], rows {source A, sink Z, B_1 .. B_4} of oriented segments in ascending A, unused branches 0xFFFFFFFF;
        counts: uint64 [4] = {bubbles, branches, bubbles whose branches all have 2k - 1 characters, the longest branch in characters})."""
        seg_off, seqs, link_off, links = (np.ascontiguousarray(a, dtype=d) for a, d in zip(graph[:4], (np.uint64, np.uint8, np.uint64, np.uint32)))
        ns = max(0, len(seg_off) - 1)
        ptr = lambda a: a.ctypes.data if len(a) else None  # noqa: E731
        args = (ptr(seg_off), ptr(seqs), ptr(link_off), ptr(links), ns, len(links), int(max_branch_chars))
        counts = np.zeros(4, dtype=np.uint64)
        cnt = counts.ctypes.data_as(C.POINTER(C.c_uint64))
        _lib.check(self._lib.bft_gpu_unitig_bubbles(self._h, *args, None, 0, cnt))
        out = np.zeros((int(counts[0]), 6), dtype=np.uint32)
        if len(out):
            _lib.check(self._lib.bft_gpu_unitig_bubbles(self._h, *args, out.ctypes.data, len(out), cnt))
        return out, counts

    def unitig_bubbles_dev(self, d_seg_off_ptr, d_seqs_ptr, d_link_off_ptr, d_links_ptr, n_segments, n_links, d_bubbles_ptr, cap, d_counts_ptr,
                           max_branch_chars=0, stream=None):
        """Device-resident bubbles (bft_gpu_unitig_bubbles_dev) over device copies of unitig_graph's arrays: {bubbles, branches, substitution
        shapes, longest branch} (4 uint64) at d_counts_ptr always, the records below cap at d_bubbles_ptr when it is not 0; no synchronisation."""
        _lib.check(self._lib.bft_gpu_unitig_bubbles_dev(self._h, C.c_void_p(d_seg_off_ptr or 0), C.c_void_p(d_seqs_ptr or 0), C.c_void_p(d_link_off_ptr or 0),
                                                        C.c_void_p(d_links_ptr or 0), n_segments, n_links, int(max_branch_chars), C.c_void_p(d_bubbles_ptr or 0),
                                                        cap, C.c_void_p(d_counts_ptr), C.c_void_p(stream or 0)))

    def unitig_segment_of(self, graph):
        """The k-mer -> segment table of a compacted graph (bft_gpu_unitig_segment_of): graph is the tuple unitig_graph returned.  Returns (seg_of:
        uint32 per row in the extract order, 2 * segment + orientation of the stored strand; pos: uint32, the row's index inside its segment), both
        0xFFFFFFFF for a row in no segment."""
        seg_off = np.ascontiguousarray(graph[0], dtype=np.uint64)
        members = np.ascontiguousarray(graph[4], dtype=np.uint32)
        ns = max(0, len(seg_off) - 1)
        self.build()  # (the row count is final)
        n = int(self.info()["kmers"])
        seg_of, pos = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        _lib.check(self._lib.bft_gpu_unitig_segment_of(self._h, members.ctypes.data if len(members) else None, len(members), seg_off.ctypes.data if len(seg_off) else None,
                                                       ns, seg_of.ctypes.data if n else None, pos.ctypes.data if n else None, n))
        return seg_of, pos

    def unitig_segment_of_dev(self, d_members_ptr, n_members, d_seg_off_ptr, n_segments, d_seg_of_ptr, d_pos_ptr, cap, stream=None):
        """Device-resident k-mer -> segment table (bft_gpu_unitig_segment_of_dev): the entries of the rows below cap into the buffers that are not 0;
        no synchronisation."""
        _lib.check(self._lib.bft_gpu_unitig_segment_of_dev(self._h, C.c_void_p(d_members_ptr or 0), n_members, C.c_void_p(d_seg_off_ptr or 0), n_segments,
                                                           C.c_void_p(d_seg_of_ptr or 0), C.c_void_p(d_pos_ptr or 0), cap, C.c_void_p(stream or 0)))

    def bubbles(self, min_shared=0, max_branch_chars=0, colors=False):
        """The variants of a canonical index in one call: unitig_graph(min_shared) -> unitig_bubbles, and with colors unitig_colors("and").  Returns one
        dict per bubble, in the order of unitig_bubbles: "source", "sink" and "branches" (oriented segments 2 * i + o of the graph at min_shared),
        "alleles" (the string of every branch as the bubble reads it: reverse-complemented for o = 1) and, with colors, "genomes": per branch the sorted
        ids of the genomes that hold every k-mer of the allele."""
        graph = self.unitig_graph(min_shared)
        seg_off, seqs = graph[0], graph[1]
        recs, _ = self.unitig_bubbles(graph, max_branch_chars)
        rows = self.unitig_colors(graph[4], seg_off, "and")[0] if colors and len(recs) else None
        text = seqs.tobytes().decode()
        comp = str.maketrans("ACGT", "TGCA")

        def spelled(b):
            s = text[int(seg_off[b >> 1]):int(seg_off[(b >> 1) + 1])]
            return s if b & 1 == 0 else s.translate(comp)[::-1]

        out = []
        for rec in recs.tolist():
            branches = [b for b in rec[2:] if b != 0xFFFFFFFF]
            item = {"source": rec[0], "sink": rec[1], "branches": branches, "alleles": [spelled(b) for b in branches]}
            if colors:
                item["genomes"] = [np.flatnonzero(np.unpackbits(rows[b >> 1], bitorder="little")).tolist() for b in branches]
            out.append(item)
        return out

    def thread_sequences(self, sequences, graph, seg_of=None):
        """Where a list of ASCII sequences runs in a compacted graph (bft_gpu_thread_sequences defines the walks): graph is the tuple unitig_graph
        returned, seg_of the pair unitig_segment_of(graph) returned (computed here when None).  Returns (walks: uint64 [n, 4], rows {sequence, first
        position p0, positions n_w, index q0 of the first position in the first step}; walk_off: uint64 [n + 1] offsets into steps; steps: uint32
        oriented segments 2 * i + o; counts: uint64 [8] = {walks, steps, positions, invalid, absent from the index, in no segment, breaks between
        located neighbours, non-canonical rows}).  An index that is not canonical raises (BFT_GPU_E_STATE)."""
        enc = [x.encode() if isinstance(x, str) else bytes(x) for x in sequences]
        off = np.zeros(len(enc) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(e) for e in enc])
        blob = b"".join(enc) + b"\0"
        if seg_of is None:
            seg_of = self.unitig_segment_of(graph)
        sg, ps = (np.ascontiguousarray(a, dtype=np.uint32) for a in seg_of)
        seg_off, link_off, links = (np.ascontiguousarray(graph[i], dtype=d) for i, d in ((0, np.uint64), (2, np.uint64), (3, np.uint32)))
        ns = max(0, len(seg_off) - 1)
        ptr = lambda a: a.ctypes.data if len(a) else None  # noqa: E731
        args = (blob, off.ctypes.data, len(enc), ptr(sg), ptr(ps), len(sg), ptr(seg_off), ns, ptr(link_off), ptr(links), len(links))
        counts = np.zeros(8, dtype=np.uint64)
        cnt = counts.ctypes.data_as(C.POINTER(C.c_uint64))
        _lib.check(self._lib.bft_gpu_thread_sequences(self._h, *args, None, None, 0, None, 0, cnt))
        nw, nst = int(counts[0]), int(counts[1])
        walks = np.zeros((nw, 4), dtype=np.uint64)
        walk_off = np.zeros(nw + 1, dtype=np.uint64)
        steps = np.zeros(nst, dtype=np.uint32)
        if nw:
            _lib.check(self._lib.bft_gpu_thread_sequences(self._h, *args, walks.ctypes.data, walk_off.ctypes.data, nw, steps.ctypes.data, nst, cnt))
        return walks, walk_off, steps, counts

    def thread_sequences_dev(self, d_seqs_ptr, d_seq_off_ptr, n_seqs, total_chars, d_seg_of_ptr, d_pos_ptr, n_rows, d_seg_off_ptr, n_segments, d_link_off_ptr,
                             d_links_ptr, n_links, d_walks_ptr, d_walk_off_ptr, walks_cap, d_steps_ptr, steps_cap, d_counts_ptr, stream=None):
        """Device-resident threading (bft_gpu_thread_sequences_dev) over device copies of the sequences, unitig_graph's arrays and unitig_segment_of's
        table: the 8 uint64 counts at d_counts_ptr always, walks (4 uint64 each) and walk_off entries (walks_cap + 1 at the most) below walks_cap, steps
        below steps_cap, each into the buffer that is not 0; no synchronisation."""
        v = lambda x: C.c_void_p(x or 0)  # noqa: E731
        _lib.check(self._lib.bft_gpu_thread_sequences_dev(self._h, v(d_seqs_ptr), v(d_seq_off_ptr), n_seqs, total_chars, v(d_seg_of_ptr), v(d_pos_ptr), n_rows,
                                                          v(d_seg_off_ptr), n_segments, v(d_link_off_ptr), v(d_links_ptr), n_links, v(d_walks_ptr), v(d_walk_off_ptr),
                                                          walks_cap, v(d_steps_ptr), steps_cap, v(d_counts_ptr), v(stream)))

    def thread(self, sequences, min_shared=0):
        """The walks of a list of sequences over the compacted graph of a canonical index in one call: unitig_graph(min_shared) -> unitig_segment_of ->
        thread_sequences.  Returns one dict per walk, in the call's order: "sequence" (its index in the list), "start" and "end" (the characters
        [start, end) of the sequence the walk covers), "path" (oriented segments 2 * i + o of the graph at min_shared), "path_start" and "path_end"
        (the same characters on the path: its segments spelled with k - 1 overlap)."""
        graph = self.unitig_graph(min_shared)
        walks, walk_off, steps, _ = self.thread_sequences(sequences, graph)
        out = []
        for (s, p0, nw, q0), a, b in zip(walks.tolist(), walk_off[:-1].tolist(), walk_off[1:].tolist()):
            span = nw + self.k - 1
            out.append({"sequence": s, "start": p0, "end": p0 + span, "path": steps[a:b].tolist(), "path_start": q0, "path_end": q0 + span})
        return out

    def components(self, genome_ids=()):
        """get_nb_connected_component (reference snippets.h, src/snippets.c:605-960) on the GPU: the connected components of the index, or of the
        sub-graph of k-mers that carry every genome id of genome_ids (strictly increasing; bft_gpu_components defines them).  Returns
        (labels: uint32 per row in the extract order, 0xFFFFFFFF for a non-member; sizes: uint64 per component, numbered by smallest row)."""
        ids = np.ascontiguousarray(genome_ids, dtype=np.uint32)
        pids = ids.ctypes.data if len(ids) else None
        counts = np.zeros(3, dtype=np.uint64)
        _lib.check(self._lib.bft_gpu_components(self._h, pids, len(ids), None, 0, None, 0, counts.ctypes.data))
        labels = np.zeros(int(self.info()["kmers"]), dtype=np.uint32)
        sizes = np.zeros(int(counts[0]), dtype=np.uint64)
        _lib.check(self._lib.bft_gpu_components(self._h, pids, len(ids), labels.ctypes.data, len(labels), sizes.ctypes.data, len(sizes),
                                                counts.ctypes.data))
        return labels, sizes

    def components_dev(self, d_labels_ptr, d_sizes_ptr, sizes_cap, d_counts_ptr, genome_ids=(), stream=None):
        """Device-resident components (bft_gpu_components_dev): {n_components, n_members, largest} (3 uint64) at d_counts_ptr always, the labels
        of every row and the sizes below sizes_cap into the buffers that are not 0; no synchronisation."""
        ids = np.ascontiguousarray(genome_ids, dtype=np.uint32)
        _lib.check(self._lib.bft_gpu_components_dev(self._h, ids.ctypes.data if len(ids) else None, len(ids), C.c_void_p(d_labels_ptr or 0),
                                                    C.c_void_p(d_sizes_ptr or 0), sizes_cap, C.c_void_p(d_counts_ptr), C.c_void_p(stream or 0)))

    def kmers_by_count(self, min_count, max_count, ascii=False):
        """extract_core_kmers / extract_dispensable_kmers / extract_singleton_kmers (reference snippets.h, src/snippets.c:10-106) on the GPU: the
        stored k-mers carried by min_count .. max_count genomes, in ascending row order (the order of extract()).  Core: both = the number of
        genomes; dispensable: 0 .. genomes - 1; singleton: 1 .. 1.  Returns (kmers, rows): kmers packed uint8 [n, nb], or with ascii=True a list
        of strings; rows uint32 [n]."""
        lo, hi = int(min_count), int(max_count)
        n = C.c_uint64()
        _lib.check(self._lib.bft_gpu_kmers_by_count(self._h, lo, hi, None, None, None, 0, C.byref(n)))
        m = int(n.value)
        rows = np.zeros(m, dtype=np.uint32)
        if ascii:
            out = np.zeros((m, self.k + 1), dtype=np.uint8)
            _lib.check(self._lib.bft_gpu_kmers_by_count(self._h, lo, hi, None, out.ctypes.data, rows.ctypes.data, m, C.byref(n)))
            if m and out[:, self.k].any():
                raise _lib.BFTError("bft_gpu_kmers_by_count: an ASCII k-mer is not NUL-terminated")
            return [r.tobytes().decode() for r in out[:, :self.k]], rows
        out = np.zeros((m, self.nb), dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_kmers_by_count(self._h, lo, hi, out.ctypes.data, None, rows.ctypes.data, m, C.byref(n)))
        return out, rows

    def kmers_by_count_dev(self, min_count, max_count, d_kmers_ptr, d_ascii_ptr, d_rows_ptr, cap, d_count_ptr, stream=None):
        """Device-resident k-mer classes (bft_gpu_kmers_by_count_dev): the number of selected k-mers (uint64) at d_count_ptr always, the first `cap`
        of them into the buffers that are not 0 (packed nb bytes each; ASCII k + 1 bytes each, NUL included; rows uint32); no synchronisation."""
        _lib.check(self._lib.bft_gpu_kmers_by_count_dev(self._h, int(min_count), int(max_count), C.c_void_p(d_kmers_ptr or 0), C.c_void_p(d_ascii_ptr or 0),
                                                        C.c_void_p(d_rows_ptr or 0), cap, C.c_void_p(d_count_ptr), C.c_void_p(stream or 0)))

    def pangenome_stats(self):
        """(spectrum, genome_total, genome_private), uint64 (bft_gpu_pangenome_stats): spectrum[c] = stored k-mers carried by exactly c genomes
        (c = 0 .. genomes), genome_total[g] = k-mers whose colour set holds g, genome_private[g] = k-mers whose colour set is {g}."""
        self.build()  # the genome count is known once the image exists; a genome named since (add_genome without k-mers) counts too
        g = max(int(self.info()["genomes"]), self._named)
        spectrum = np.zeros(g + 1, dtype=np.uint64)
        total = np.zeros(g, dtype=np.uint64)
        private = np.zeros(g, dtype=np.uint64)
        _lib.check(self._lib.bft_gpu_pangenome_stats(self._h, spectrum.ctypes.data, total.ctypes.data if g else None, private.ctypes.data if g else None, g + 1))
        return spectrum, total, private

    def pangenome_stats_dev(self, d_spectrum_ptr, d_genome_total_ptr, d_genome_private_ptr, cap, stream=None):
        """Device-resident statistics (bft_gpu_pangenome_stats_dev): uint64 counters, genomes + 1 / genomes / genomes entries, into the buffers
        that are not 0; cap = entries of room in the spectrum; no synchronisation."""
        _lib.check(self._lib.bft_gpu_pangenome_stats_dev(self._h, C.c_void_p(d_spectrum_ptr or 0), C.c_void_p(d_genome_total_ptr or 0),
                                                         C.c_void_p(d_genome_private_ptr or 0), cap, C.c_void_p(stream or 0)))

    # -- the genome-by-genome shared k-mer matrix (bft_gpu_genome_matrix*) and the distances computed from it ------------------------
    def _genome_matrix(self, call):
        g = C.c_uint32()
        _lib.check(call(None, 0, C.byref(g)))
        n = int(g.value)
        shared = np.zeros((n, n), dtype=np.uint64)
        _lib.check(call(shared.ctypes.data if n else None, n * n, C.byref(g)))
        return shared

    def genome_matrix(self, min_count=0, max_count=None):
        """uint64 [G, G] (bft_gpu_genome_matrix): shared[i, j] = stored k-mers whose colour set holds both genome i and genome j, restricted to the
        k-mers carried by min_count .. max_count genomes (None: no upper bound; 0, G - 1: the accessory genome).  Symmetric; the diagonal is
        pangenome_stats()[1] when nothing is restricted.  Exact."""
        lo, hi = int(min_count), 0xFFFFFFFF if max_count is None else int(max_count)
        return self._genome_matrix(lambda out, cap, g: self._lib.bft_gpu_genome_matrix(self._h, lo, hi, out, cap, g))

    def genome_matrix_colorsets(self, colorsets):
        """uint64 [G, G] (bft_gpu_genome_matrix_colorsets): the same matrix over a batch of colour-set ids (of query_rows, query_prefixes or
        extract), each id counted as often as it occurs; 0xFFFFFFFF (absent) is skipped, any other id past the dictionary raises."""
        cs = np.ascontiguousarray(colorsets, dtype=np.uint32)
        return self._genome_matrix(lambda out, cap, g: self._lib.bft_gpu_genome_matrix_colorsets(self._h, cs.ctypes.data if len(cs) else None, len(cs), out, cap, g))

    def genome_matrix_dev(self, d_shared_ptr, cap, min_count=0, max_count=None, stream=None):
        """Device-resident matrix (bft_gpu_genome_matrix_dev): G * G uint64 at d_shared_ptr (cap entries of room); no synchronisation."""
        _lib.check(self._lib.bft_gpu_genome_matrix_dev(self._h, int(min_count), 0xFFFFFFFF if max_count is None else int(max_count), C.c_void_p(d_shared_ptr or 0),
                                                       cap, C.c_void_p(stream or 0)))

    def genome_matrix_colorsets_dev(self, d_colorsets_ptr, n, d_shared_ptr, cap, stream=None):
        """Device-resident matrix over n colour-set ids (uint32) at d_colorsets_ptr (bft_gpu_genome_matrix_colorsets_dev): ids past the dictionary
        are skipped; no synchronisation."""
        _lib.check(self._lib.bft_gpu_genome_matrix_colorsets_dev(self._h, C.c_void_p(d_colorsets_ptr or 0), n, C.c_void_p(d_shared_ptr or 0), cap,
                                                                 C.c_void_p(stream or 0)))

    @staticmethod
    def distances_from_matrix(shared, metric, k):
        """float64 [G, G] from a shared k-mer matrix, S = shared[i, j], n_i = shared[i, i]: "jaccard" = S / (n_i + n_j - S), 0.0 for an empty
        union; "containment"[i, j] = S / n_i, 0.0 for n_i = 0; "mash" = -ln(2 J / (1 + J)) / k, capped at 1.0 and 1.0 for J = 0."""
        if metric not in ("jaccard", "containment", "mash"):
            raise ValueError(f"unknown metric {metric!r}")
        s = np.asarray(shared).astype(np.float64)
        n = np.diag(s)
        if metric == "containment":
            den = np.repeat(n[:, None], len(n), axis=1)
        else:
            den = n[:, None] + n[None, :] - s
        out = np.zeros_like(s)
        np.divide(s, den, out=out, where=den > 0)
        if metric == "mash":
            j = out
            out = np.ones_like(j)
            pos = j > 0
            out[pos] = np.minimum(1.0, -np.log(2.0 * j[pos] / (1.0 + j[pos])) / k)
            out[out == 0] = 0.0  # (-0.0 for J = 1)
        return out

    def genome_distances(self, metric="jaccard", min_count=0, max_count=None):
        """float64 [G, G] computed in numpy from genome_matrix(min_count, max_count): see distances_from_matrix."""
        if metric not in ("jaccard", "containment", "mash"):
            raise ValueError(f"unknown metric {metric!r}")
        return self.distances_from_matrix(self.genome_matrix(min_count, max_count), metric, self.k)

    # -- colour-set algebra over groups (bft_gpu_combine_*: intersection / union / sym_difference of annotations, batched) -------
    SETOPS = {"and": 0, "or": 1, "symdiff": 2}

    @classmethod
    def _setop(cls, op):
        if op not in cls.SETOPS:
            raise ValueError(f"op must be one of {sorted(cls.SETOPS)}, not {op!r}")
        return cls.SETOPS[op]

    @staticmethod
    def _group_off(group_off, n):
        """The offsets as a contiguous uint64 array, checked as the library checks them (nb_groups + 1 entries, not decreasing, the last within n)."""
        off = np.ascontiguousarray(group_off, dtype=np.uint64)
        if off.ndim != 1 or len(off) == 0:
            raise ValueError("group_off must hold nb_groups + 1 offsets")
        if (off[1:] < off[:-1]).any():
            raise ValueError("group offsets must not decrease")
        if len(off) > 1 and int(off[-1]) > n:
            raise ValueError("the last group ends behind the batch")
        return off

    def combine_colors(self, kmers, group_off, op="and", skip_absent=False):
        """intersection_annotations / union_annotations / sym_difference_annotations (include/bft.h:112-114) for groups of k-mers, reduced on the GPU
        (bft_gpu_combine_colors): group g is kmers[group_off[g]:group_off[g + 1]].  Returns (rows uint8 [groups, CEIL(genomes / 8)], counts uint32
        [groups] = genomes per row, found uint32 [groups] = members of the group the index stores).  An absent k-mer is the empty set, or is
        left out of its group with skip_absent."""
        code = self._setop(op)
        kmers = self._chk(kmers)
        off = self._group_off(group_off, len(kmers))
        ng = len(off) - 1
        self.build()  # the genome count is known once the image exists
        g = self.info()["genomes"]
        rows = np.zeros((ng, (g + 7) // 8), dtype=np.uint8)
        counts = np.zeros(ng, dtype=np.uint32)
        found = np.zeros(ng, dtype=np.uint32)
        _lib.check(self._lib.bft_gpu_combine_colors(self._h, kmers.ctypes.data, len(kmers), off.ctypes.data, ng, code, 1 if skip_absent else 0,
                                                    rows.ctypes.data, counts.ctypes.data, found.ctypes.data))
        return rows, counts, found

    def combine_colorsets(self, colorsets, group_off, op="and"):
        """The same over colour-set ids (query_rows, extract, query_prefixes hand them out; 0xFFFFFFFF = an absent k-mer, the empty set):
        (rows, counts) of bft_gpu_combine_colorsets."""
        code = self._setop(op)
        cs = np.ascontiguousarray(colorsets, dtype=np.uint32)
        if cs.ndim != 1:
            raise ValueError("colorsets must be a flat array of ids")
        off = self._group_off(group_off, len(cs))
        ng = len(off) - 1
        self.build()
        g = self.info()["genomes"]
        rows = np.zeros((ng, (g + 7) // 8), dtype=np.uint8)
        counts = np.zeros(ng, dtype=np.uint32)
        _lib.check(self._lib.bft_gpu_combine_colorsets(self._h, cs.ctypes.data, len(cs), off.ctypes.data, ng, code, rows.ctypes.data, counts.ctypes.data))
        return rows, counts

    def combine_colors_dev(self, d_kmers_ptr, n, d_group_off_ptr, nb_groups, op, skip_absent, d_rows_ptr, d_counts_ptr, d_found_ptr, stream=None):
        """Device-resident form (bft_gpu_combine_colors_dev): offsets uint64, rows nb_groups x CEIL(genomes / 8) bytes, counts / found uint32, into the
        buffers that are not 0; no synchronisation."""
        _lib.check(self._lib.bft_gpu_combine_colors_dev(self._h, C.c_void_p(d_kmers_ptr or 0), n, C.c_void_p(d_group_off_ptr or 0), nb_groups, self._setop(op),
                                                        1 if skip_absent else 0, C.c_void_p(d_rows_ptr or 0), C.c_void_p(d_counts_ptr or 0),
                                                        C.c_void_p(d_found_ptr or 0), C.c_void_p(stream or 0)))

    def combine_colorsets_dev(self, d_colorsets_ptr, n, d_group_off_ptr, nb_groups, op, d_rows_ptr, d_counts_ptr, stream=None):
        """Device-resident form over colour-set ids (bft_gpu_combine_colorsets_dev); no synchronisation."""
        _lib.check(self._lib.bft_gpu_combine_colorsets_dev(self._h, C.c_void_p(d_colorsets_ptr or 0), n, C.c_void_p(d_group_off_ptr or 0), nb_groups,
                                                           self._setop(op), C.c_void_p(d_rows_ptr or 0), C.c_void_p(d_counts_ptr or 0), C.c_void_p(stream or 0)))

    # -- vertex marking (bft_gpu_marks_*: set_marking / set_flag_kmer / get_flag_kmer and the traversals' marks) -------
    def set_marking(self):
        """set_marking (include/bft.h:143): the graph is locked (no insertion, no build) and every stored k-mer gets a flag, 0 at first; on a graph
        that is already marking nothing changes."""
        _lib.check(self._lib.bft_gpu_marks_begin(self._h))

    def unset_marking(self):
        """unset_marking (include/bft.h:144): the flags are released and the graph unlocked."""
        _lib.check(self._lib.bft_gpu_marks_end(self._h))

    @staticmethod
    def _flag_args(flag_or_array, n):
        """(flags array or None, single flag) of a set_flags call"""
        if np.ndim(flag_or_array) == 0:
            f = int(flag_or_array)
            if not 0 <= f <= 255:
                raise ValueError("a flag is 0, 1, 2 or 3")
            return None, f
        flags = np.ascontiguousarray(flag_or_array, dtype=np.uint8)
        if flags.shape != (n,):
            raise ValueError(f"expected one flag per k-mer ({n}), got {flags.shape}")
        return flags, 0

    def set_flags(self, kmers, flag_or_array):
        """set_flag_kmer for a batch: one flag (0..3) for every k-mer, or an array with one flag per k-mer.  Returns the number of absent k-mers
        (they are ignored)."""
        kmers = self._chk(kmers)
        flags, flag = self._flag_args(flag_or_array, len(kmers))
        absent = C.c_uint64()
        _lib.check(self._lib.bft_gpu_marks_set(self._h, kmers.ctypes.data, len(kmers), flags.ctypes.data if flags is not None else None, flag, C.byref(absent)))
        return int(absent.value)

    def set_flags_dev(self, d_kmers_ptr, n, flag=0, d_flags_ptr=None, d_absent_ptr=None, stream=None):
        """Device-resident set (bft_gpu_marks_set_dev): one flag, or one byte per k-mer at d_flags_ptr; no synchronisation."""
        _lib.check(self._lib.bft_gpu_marks_set_dev(self._h, C.c_void_p(d_kmers_ptr), n, C.c_void_p(d_flags_ptr or 0), int(flag), C.c_void_p(d_absent_ptr or 0),
                                                   C.c_void_p(stream or 0)))

    def get_flags(self, kmers):
        """get_flag_kmer for a batch: uint8 per k-mer, 0..3, or 0xFF for an absent k-mer."""
        kmers = self._chk(kmers)
        out = np.zeros(len(kmers), dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_marks_get(self._h, kmers.ctypes.data, len(kmers), out.ctypes.data, None))
        return out

    def get_flags_dev(self, d_kmers_ptr, n, d_flags_out_ptr, d_absent_ptr=None, stream=None):
        _lib.check(self._lib.bft_gpu_marks_get_dev(self._h, C.c_void_p(d_kmers_ptr), n, C.c_void_p(d_flags_out_ptr), C.c_void_p(d_absent_ptr or 0), C.c_void_p(stream or 0)))

    def test_and_set(self, kmers, expect, flag):
        """A k-mer moves to `flag` only if it holds `expect`; uint8 per batch entry: 1 for the one entry that moved its k-mer, 0 otherwise."""
        kmers = self._chk(kmers)
        won = np.zeros(len(kmers), dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_marks_test_and_set(self._h, kmers.ctypes.data, len(kmers), int(expect), int(flag), won.ctypes.data, None))
        return won

    def test_and_set_dev(self, d_kmers_ptr, n, expect, flag, d_won_ptr, d_absent_ptr=None, stream=None):
        _lib.check(self._lib.bft_gpu_marks_test_and_set_dev(self._h, C.c_void_p(d_kmers_ptr), n, int(expect), int(flag), C.c_void_p(d_won_ptr),
                                                            C.c_void_p(d_absent_ptr or 0), C.c_void_p(stream or 0)))

    def fill_flags(self, flag):
        """Every stored k-mer gets `flag`."""
        _lib.check(self._lib.bft_gpu_marks_fill(self._h, int(flag)))

    def fill_flags_dev(self, flag, stream=None):
        _lib.check(self._lib.bft_gpu_marks_fill_dev(self._h, int(flag), C.c_void_p(stream or 0)))

    def flag_counts(self):
        """uint64[4]: stored k-mers per flag value."""
        counts = np.zeros(4, dtype=np.uint64)
        _lib.check(self._lib.bft_gpu_marks_counts(self._h, counts.ctypes.data))
        return counts

    def flag_counts_dev(self, d_counts_ptr, stream=None):
        _lib.check(self._lib.bft_gpu_marks_counts_dev(self._h, C.c_void_p(d_counts_ptr), C.c_void_p(stream or 0)))

    def select_flagged(self, mask, ascii=False):
        """The k-mers whose flag is in the 4-bit mask (bit f: flag f), in ascending row order.  Returns (kmers, rows) as kmers_by_count."""
        mask = int(mask)
        n = C.c_uint64()
        _lib.check(self._lib.bft_gpu_marks_select(self._h, mask, None, None, None, 0, C.byref(n)))
        m = int(n.value)
        rows = np.zeros(m, dtype=np.uint32)
        if ascii:
            out = np.zeros((m, self.k + 1), dtype=np.uint8)
            _lib.check(self._lib.bft_gpu_marks_select(self._h, mask, None, out.ctypes.data, rows.ctypes.data, m, C.byref(n)))
            if m and out[:, self.k].any():
                raise _lib.BFTError("bft_gpu_marks_select: an ASCII k-mer is not NUL-terminated")
            return [r.tobytes().decode() for r in out[:, :self.k]], rows
        out = np.zeros((m, self.nb), dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_marks_select(self._h, mask, out.ctypes.data, None, rows.ctypes.data, m, C.byref(n)))
        return out, rows

    def select_flagged_dev(self, mask, d_kmers_ptr, d_ascii_ptr, d_rows_ptr, cap, d_count_ptr, stream=None):
        _lib.check(self._lib.bft_gpu_marks_select_dev(self._h, int(mask), C.c_void_p(d_kmers_ptr or 0), C.c_void_p(d_ascii_ptr or 0), C.c_void_p(d_rows_ptr or 0), cap,
                                                      C.c_void_p(d_count_ptr), C.c_void_p(stream or 0)))

    def reach(self, seeds, genome_ids=(), through=0, to=1, boundary=False):
        """Every eligible k-mer (flag `through`, colour set holding every id of genome_ids) connected to an eligible seed through eligible k-mers gets
        the flag `to`; boundary=True also marks what BFS_subgraph / DFS_subgraph look at (bft_gpu_marks_reach).  Returns (seed_new: uint8 per seed,
        1 for the lowest-index eligible seed of each component; counts: uint64 {eligible painted, boundary painted, seeds absent})."""
        seeds = self._chk(seeds)
        ids = np.ascontiguousarray(genome_ids, dtype=np.uint32)
        seed_new = np.zeros(len(seeds), dtype=np.uint8)
        counts = np.zeros(3, dtype=np.uint64)
        _lib.check(self._lib.bft_gpu_marks_reach(self._h, seeds.ctypes.data, len(seeds), ids.ctypes.data if len(ids) else None, len(ids), int(through), int(to),
                                                 1 if boundary else 0, seed_new.ctypes.data, counts.ctypes.data))
        return seed_new, counts

    def reach_dev(self, d_seeds_ptr, n_seeds, d_seed_new_ptr, d_counts_ptr, genome_ids=(), through=0, to=1, boundary=False, stream=None):
        ids = np.ascontiguousarray(genome_ids, dtype=np.uint32)
        _lib.check(self._lib.bft_gpu_marks_reach_dev(self._h, C.c_void_p(d_seeds_ptr), n_seeds, ids.ctypes.data if len(ids) else None, len(ids), int(through), int(to),
                                                     1 if boundary else 0, C.c_void_p(d_seed_new_ptr or 0), C.c_void_p(d_counts_ptr), C.c_void_p(stream or 0)))

    def read_flags(self):
        """The packed flag array: uint8, 4 rows per byte, row r in bits 2 (r % 4) .. + 1 of byte r // 4 (rows in the order of extract())."""
        n = C.c_uint64()
        _lib.check(self._lib.bft_gpu_marks_read(self._h, None, 0, C.byref(n)))
        out = np.zeros(int(n.value), dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_marks_read(self._h, out.ctypes.data if len(out) else None, len(out), C.byref(n)))
        return out

    def write_flags(self, packed):
        """The whole packed flag array in (the layout of read_flags)."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_marks_write(self._h, packed.ctypes.data if len(packed) else None, len(packed)))

    def genome_name(self, id_genome):
        """The name of genome id_genome (the reference's filenames[id_genome]; "genome_<id>" for an id that was never named)."""
        buf = C.create_string_buffer(4096)
        _lib.check(self._lib.bft_gpu_genome_name(self._h, int(id_genome), buf, len(buf)))
        return buf.value.decode()


class BFTGroup:
    """One built index replicated on several GPUs of this process; host batches are sharded over them (bft_gpu_group_*)."""

    def __init__(self, bft, devices):
        self._lib = _lib.load()
        self._bft = bft
        arr = (C.c_int * len(devices))(*devices)
        g = C.c_void_p()
        _lib.check(self._lib.bft_gpu_group_create(bft._h, bft.device, arr, len(devices), C.byref(g)))
        self._g = g
        self.nb = bft.nb

    def size(self):
        return self._lib.bft_gpu_group_size(self._g)

    def close(self):
        if self._g:
            self._lib.bft_gpu_group_free(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def query_presence(self, kmers):
        kmers = self._bft._chk(kmers)
        bits = np.zeros((len(kmers) + 7) // 8, dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_group_query_presence(self._g, kmers.ctypes.data, len(kmers), bits.ctypes.data))
        return bits

    def query_color_rows(self, kmers):
        kmers = self._bft._chk(kmers)
        n = len(kmers)
        rowbytes = (self._bft.info()["genomes"] + 7) // 8
        bits = np.zeros((n + 7) // 8, dtype=np.uint8)
        rows = np.zeros((n, rowbytes), dtype=np.uint8)
        _lib.check(self._lib.bft_gpu_group_query_color_rows(self._g, kmers.ctypes.data, n, bits.ctypes.data, rows.ctypes.data))
        return bits, rows

    def query_branching(self, kmers, with_counts=False):
        kmers = self._bft._chk(kmers)
        n = len(kmers)
        bits = np.zeros((n + 7) // 8, dtype=np.uint8)
        counts = np.zeros(n, dtype=np.uint8) if with_counts else None
        _lib.check(self._lib.bft_gpu_group_query_branching(self._g, kmers.ctypes.data, n, bits.ctypes.data, counts.ctypes.data if with_counts else None))
        return (bits, counts) if with_counts else bits

    # -- device-resident batches: one per slot, in the memory of that slot's GPU; only enqueues (bft_gpu_group_*_dev) --------------
    def member_device(self, i):
        return self._lib.bft_gpu_group_member_device(self._g, i)

    def member_footprint(self, i):
        out = (C.c_uint64 * 12)()
        _lib.check(self._lib.bft_gpu_group_member_footprint(self._g, i, out, 12))
        return dict(zip(BFT.FOOTPRINT_FIELDS, [int(x) for x in out]))

    def _ptrs(self, vals):
        # the C side indexes bft_gpu_group_size(g) entries of every array: a shorter list would be an out-of-bounds host read
        if len(vals) != self.size():
            raise ValueError(f"one entry per slot of the group expected ({self.size()}), got {len(vals)}")
        return (C.c_void_p * len(vals))(*[C.c_void_p(v) if v else None for v in vals])

    def _counts(self, n):
        if len(n) != self.size():
            raise ValueError(f"one batch size per slot of the group expected ({self.size()}), got {len(n)}")
        return (C.c_uint64 * len(n))(*n)

    def query_presence_dev(self, d_kmers, n, d_bits, streams=None):
        """d_kmers / d_bits / streams: device pointers (ints) per slot; n: k-mers per slot"""
        ns = self._counts(n)
        _lib.check(self._lib.bft_gpu_group_query_presence_dev(self._g, self._ptrs(d_kmers), ns, self._ptrs(d_bits), self._ptrs(streams) if streams else None))

    def query_color_rows_dev(self, d_kmers, n, d_bits, d_rows, d_scratch, streams=None):
        ns = self._counts(n)
        _lib.check(self._lib.bft_gpu_group_query_color_rows_dev(self._g, self._ptrs(d_kmers), ns, self._ptrs(d_bits), self._ptrs(d_rows), self._ptrs(d_scratch),
                                                                self._ptrs(streams) if streams else None))

    def query_branching_dev(self, d_kmers, n, d_bits, d_counts=None, streams=None):
        ns = self._counts(n)
        _lib.check(self._lib.bft_gpu_group_query_branching_dev(self._g, self._ptrs(d_kmers), ns, self._ptrs(d_bits), self._ptrs(d_counts) if d_counts else None,
                                                               self._ptrs(streams) if streams else None))


def shard(n, parts, i):
    """bft_gpu_group_shard: the contiguous 64-aligned slice [begin, end) of an n-query batch for part i of `parts`"""
    a, b = C.c_uint64(), C.c_uint64()
    _lib.check(_lib.load().bft_gpu_group_shard(n, parts, i, C.byref(a), C.byref(b)))
    return a.value, b.value


def cache_release():
    """bft_gpu_cache_release: the library's cache of released device blocks back to the HIP runtime; returns the bytes"""
    return int(_lib.load().bft_gpu_cache_release())


def create_cdbg(k, device=0):
    """create_cdbg(k, treshold_compression) (include/bft.h:62)."""
    return BFT(k, device)
